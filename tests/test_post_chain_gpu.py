"""render_sample's whole corrector chain on an MI355X -- beat_sync -> smooth -> keep_apart -> ground -> foot_lock -- held to the float64
restatements stage by stage, on the seeded cases of tests/chain_ref.py: N ("normal": 2 clips x 3 dancers x 60 frames with contact
channels), L ("long": 3 half-overlapping windows of 40 frames x 2 dancers, stitched to one song of 80 frames, contacts=None) and P
(N's export with one NaN in q and one +Inf in pos).

a. every kernel stage against its restatement run on the kernel's own inputs (the previous kernel stage's output words), under the
   checks and bounds of that stage's own GPU test, imported from it: no bound is set here;
b. all 32 subsets of the five attributes in both modes through render_sample against the writers called on the hand composition of
   the same stages: equal bytes;
c. the promises of render_sample's docstring on the final output, scored by the restatements and a float64 FK;
d. the poisoned case: non-finite floats and the stages' reports against the restatements, clips alone, untouched dancers;
e. a second run, equal bits.
Run with -s for the figures kept in profiles/post_chain.txt."""
import importlib
import os

import numpy as np
import pytest
import torch

import apart_ref as AR
import chain_ref as CH
import footlock_ref as FR
import ground_ref as GR
import group_ref as GRP
import metrics_ref as MR
import smooth_ref as SR
import test_apart_gpu as TA
import test_beatsync_gpu as TB
import test_footlock_gpu as TF
import test_ground_gpu as TG
import test_group_gpu as TGR
import test_metrics_gpu as TM
import test_smooth_gpu as TS
from tcdiff_amd import export as E
from tcdiff_amd.draw import write_draw_out
from tcdiff_amd.footlock import foot_lock
from tcdiff_amd.gltf import write_glb_out
from tcdiff_amd.group_metrics import group_metrics
from tcdiff_amd.metrics import beats_from_cond, motion_metrics

B = importlib.import_module("tcdiff_amd.beat_sync")               # the modules: the package's attributes of these names are the functions
S = importlib.import_module("tcdiff_amd.smooth")
P = importlib.import_module("tcdiff_amd.apart")
G = importlib.import_module("tcdiff_amd.ground")
pytestmark = pytest.mark.gpu
DEV = "cuda"
EPOCH = 7
CASES = ("N", "L")


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


@pytest.fixture(scope="module")
def diffusion():
    """render_sample of given samples asks nothing of the model (as tests/test_apart_gpu.py builds it)"""
    from tcdiff_amd import GaussianDiffusion
    d = GaussianDiffusion.__new__(GaussianDiffusion)
    torch.nn.Module.__init__(d)
    d.smpl = None
    return d


def exported(c, d):
    """the export launch on a case -> (the state (q, pos, poses, contacts) of device tensors, beats, parents, offsets)"""
    parents, offsets = d._skeleton(torch.device(DEV))
    state = E.export_poses(c.x.to(DEV), c.norm, c.mode, c.dn, parents=parents, offsets=offsets)
    beats = beats_from_cond(c.cond.to(DEV), state[2].shape[2], long=c.mode == "long")
    assert np.array_equal(host(beats), c.beats)
    return state, beats, parents, offsets


def kernels(state, beats, dn, on, parents, offsets, shift=False):
    """the stages of `on` called by hand, in render_sample's order and with its arguments -> ({stage: (inputs, result)}, final state);
    shift=True also asks keep_apart and ground for their shift planes (the same bits otherwise: tests/test_apart_gpu.py,
    tests/test_ground_gpu.py)"""
    q, pos, poses, contacts = state
    out = {}
    for name in CH.STAGES:
        if name not in on:
            continue
        inputs = (q, pos, poses, contacts)
        if name == "beat_sync":
            r = B.beat_sync(q, pos, beats, dn=dn, contacts=contacts, parents=parents, offsets=offsets, measure=False)
            q, pos, poses, contacts = r.q, r.pos, r.joints, r.contacts
        elif name == "smooth":
            r = S.smooth(q, pos, dn=dn, parents=parents, offsets=offsets, measure=False)
            q, pos, poses = r[:3]
        elif name == "keep_apart":
            r = P.keep_apart(pos, poses, dn=dn, parents=parents, return_shift=shift)
            pos, poses = r[:2]
        elif name == "ground":
            r = G.ground(pos, poses, contacts, dn=dn, floor=None, parents=parents, return_shift=shift)
            pos, poses = r[:2]
        else:
            r = foot_lock(q, pos, contacts, dn=dn, parents=parents, offsets=offsets)
            q, poses = r.q, r.joints
        out[name] = (inputs, r)
    return out, (q, pos, poses, contacts)


def as_state(t):
    q, pos, poses, contacts = (host(x) for x in t)
    return dict(q=q, pos=pos, joints=poses, contacts=contacts)


def fk64(q, pos, dn):
    return GR.fk64(SR.frames_of(q, dn), SR.frames_of(pos, dn))


def hold_stage(name, inputs, r, beats, dn, what):
    """one kernel stage against its restatement of the kernel's own inputs, by the checks of the stage's own GPU test -> the restatement"""
    q, pos, J, C = (host(x) for x in inputs)
    if name == "beat_sync":
        margin = CH.kin_margin(dict(speed=host(r.speed)))
        print(f"[post_chain] {what}: neighbouring smoothed speeds {margin:.3e} apart (relative, guard {CH.KIN_GUARD:g})")
        assert margin > CH.KIN_GUARD and int(r.anchors.min()) > 0 and not r.status.any()
        TB.check_against(r, q, pos, host(beats), dn, C, True, what)
        return None
    if name == "smooth":
        ref = TS.reference(q, pos, dn)
        TS.check_against(r, q, pos, dn, ref, what)
        assert float(r.max_rot_change.min()) > 0
        return ref
    if name == "keep_apart":
        ref = AR.keep_apart(pos, J, dn=dn, details=True)
        ok, why = AR.judge(ref)
        assert ok, why
        TA._compare(r, ref, pos, J, what)
        assert int(r.pushed.sum()) > 0
        return ref
    if name == "ground":
        ref = GR.ground(pos, J, C, dn=dn, details=True)
        ok, why = GR.judge(ref)
        assert ok, why
        TG._compare(r, ref, pos, J, what)
        assert float(r.max_shift.max()) > 0
        return ref
    ref = FR.foot_lock(q, pos, C, dn=dn)
    reach, still = CH.reach_margin(ref), ref["min_margin"]
    print(f"[post_chain] {what}: reach margin {reach:.3e} m (guard {CH.REACH_GUARD:g}), still margin {still:.3e} m (guard {CH.STILL_GUARD:g})")
    assert reach > CH.REACH_GUARD and (C is not None or still > CH.STILL_GUARD)
    TF.check_against(r, ref, what)
    got = host(r.q)
    P1 = fk64(got, pos, dn)
    pin, seen = CH.pin_error(P1, ref)
    fk = float(np.abs(host(r.joints) - P1).max())
    print(f"[post_chain] {what}: pinned joints within {pin:.3e} m of their anchors over {seen} frames (bound {FR.PIN_BOUND:g}), joints {fk:.2e} m from a "
          f"float64 FK (bound {SR.FK_BOUND:g})")
    assert seen > 0 and pin <= FR.PIN_BOUND and fk <= SR.FK_BOUND          # the joints: the bound tests/test_footlock_gpu.py check_purpose holds them to
    assert np.array_equal(got[:, :, TF.OTHERS].view(np.int32), q[:, :, TF.OTHERS].view(np.int32))
    assert bool((r.planted > 0).all(-1).any())
    return ref


# ---- a. stage by stage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CASES)
def test_every_kernel_stage_against_its_restatement_on_the_kernels_own_inputs(which, diffusion):
    c = CH.case(which)
    state, beats, parents, offsets = exported(c, diffusion)
    assert (state[3] is None) == (which == "L") and tuple(state[2].shape) == (c.clips, c.dn, c.T, 24, 3)
    stages, final = kernels(state, beats, c.dn, CH.STAGES, parents, offsets, shift=True)
    for name in CH.STAGES:
        inputs, r = stages[name]
        hold_stage(name, inputs, r, beats, c.dn, f"{which} {name}")


# ---- b. every subset, both modes, through render_sample ---------------------------------------------------------------------------------------------
def _files(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


@pytest.mark.parametrize("mask", range(32), ids=lambda m: "+".join(CH.SUBSETS[m]) or "none")
@pytest.mark.parametrize("which", CASES)
def test_render_sample_writes_what_the_hand_composition_writes(which, mask, diffusion, tmp_path):
    c, on = CH.case(which), CH.SUBSETS[mask]
    d = diffusion
    assert all(getattr(d, k) is False for k in CH.STAGES)
    draw = {"draw_out": str(tmp_path / "draw")} if mask == 31 else {}
    x = c.x.to(DEV)
    try:
        for k in on:
            setattr(d, k, True)
        d.render_sample(x, c.cond, c.norm, EPOCH, None, fk_out=str(tmp_path / "fk"), glb_out=str(tmp_path / "glb"), name=c.names, mode=c.mode,
                        required_dancer_num=c.dn, **draw)
    finally:
        for k in on:
            delattr(d, k)                                                  # back to the class attributes
    state, beats, parents, offsets = exported(c, d)
    _, (q, pos, poses, contacts) = kernels(state, beats, c.dn, on, parents, offsets)
    E.write_fk_out(str(tmp_path / "fk_hand"), c.mode, EPOCH, c.names, q, pos, poses)
    write_glb_out(str(tmp_path / "glb_hand"), c.mode, EPOCH, c.names, q, pos, c.dn, parents=parents, offsets=offsets)
    got, want = _files(tmp_path / "fk"), _files(tmp_path / "fk_hand")
    assert len(got) == c.clips and got == want
    got, want = _files(tmp_path / "glb"), _files(tmp_path / "glb_hand")
    assert len(got) == c.clips and got == want
    if draw:
        write_draw_out(str(tmp_path / "draw_hand"), c.mode, EPOCH, c.names, poses, contacts, render_len=512, parents=parents)
        got, want = _files(tmp_path / "draw"), _files(tmp_path / "draw_hand")
        assert len(got) == c.clips and got == want and all(v[:8] == b"\x89PNG\r\n\x1a\n" for v in got.values())
    if on:                                                                 # and not the plain export's
        E.write_fk_out(str(tmp_path / "fk_plain"), c.mode, EPOCH, c.names, *state[:3])
        assert _files(tmp_path / "fk") != _files(tmp_path / "fk_plain")


# ---- c. the promises on the final output ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CASES)
def test_the_final_output_keeps_the_promises_and_the_metric_launches_measure_it(which, diffusion):
    c = CH.case(which)
    state, beats, parents, offsets = exported(c, diffusion)
    stages, final = kernels(state, beats, c.dn, CH.STAGES, parents, offsets)
    inputs, r = stages["foot_lock"]
    lock = FR.foot_lock(host(inputs[0]), host(inputs[1]), host(inputs[3]), dn=c.dn)
    kept, s0, s1, pin = CH.end_state(c, as_state(state), as_state(final), lock)
    print(f"[post_chain] {which}, the kernels' chain: pinned joints {pin:.3e} m from their anchors (bound {FR.PIN_BOUND:g}); raw -> final\n" + CH.report(s0, s1))
    assert all(kept.values()), kept
    # the kernels' own metric launches on the final joints, under their modules' rules
    J, C = final[2], final[3]
    Jn, Cn, bn = host(J), host(C), host(beats)
    want = GRP.group_metrics(Jn, details=True)
    ok, why = GRP.judge(want, 1e-6)
    assert ok, why
    TGR._compare(group_metrics(J, return_frames=True), want, f"[post_chain] {which} final group_metrics")
    want = GR.ground(AR.pos_of(Jn), Jn, Cn, details=True)
    ok, why = CH.ground_metrics_clear(want)
    assert ok, why
    assert TG._metrics_match(G.ground_metrics(J, C), want["before"], f"{which} final ground_metrics") <= GR.FLOAT_BOUND
    TS.check_scores(S.smoothness(J), Jn, f"{which} final")
    zeros = np.zeros(Jn.shape[:3] + (4,), np.float32) if Cn is None else Cn
    assert MR.decisions_clear(Jn, zeros, bn)
    TM._compare(motion_metrics(J, C, beats), MR.metrics(Jn, Cn, bn), f"[post_chain] {which} final motion_metrics")


# ---- d. poison --------------------------------------------------------------------------------------------------------------------------------------
REPORTS = {"beat_sync": ("status", "copied", "moved", "anchors"), "smooth": ("copied",), "keep_apart": ("pushed", "capped", "contact_before", "contact_after"),
           "ground": ("capped",), "foot_lock": ("planted", "clamped")}


def poisoned_state(c, d):
    state, beats, parents, offsets = exported(c, d)
    q, pos = CH.poisoned(host(state[0]), host(state[1]), c.dn)
    tq, tpos = dev(q), dev(pos)
    poses = foot_lock(tq, tpos, torch.zeros_like(state[3]), dn=c.dn, parents=parents, offsets=offsets).joints      # every contact off: the FK of the poses as they are
    assert torch.equal(bits(poses)[torch.isfinite(poses)], bits(state[2])[torch.isfinite(poses)])                  # the export's words where they are finite
    return state, (tq, tpos, poses, state[3]), beats, parents, offsets


def non_finite(a):
    return ~np.isfinite(np.asarray(a))


def test_a_poisoned_frame_goes_through_every_stage_as_the_restatements_say(diffusion):
    c = CH.case("N")
    clean, state, beats, parents, offsets = poisoned_state(c, diffusion)
    stages, final = kernels(state, beats, c.dn, CH.STAGES, parents, offsets, shift=True)
    bn = host(beats)
    for name in CH.STAGES:
        inputs, r = stages[name]
        before = as_state(inputs)
        joints_out = host(r.joints) if name in ("beat_sync", "smooth", "foot_lock") else None
        jin = host(TB.input_joints(inputs[0], inputs[1], beats, c.dn, inputs[3], r, True)) if name == "beat_sync" else None
        ref, after = CH.stage(name, before, bn, c.dn, joints_in=jin, joints_out=joints_out)
        got = dict(q=host(getattr(r, "q", inputs[0])), pos=host(getattr(r, "pos", inputs[1])), joints=host(r.joints))
        for k in ("q", "pos", "joints"):
            want = after[k] if k != "joints" or joints_out is None else CH.joints_of(after["q"], after["pos"], c.dn)
            assert np.array_equal(non_finite(got[k]), non_finite(want)), (name, k, int(non_finite(got[k]).sum()), int(non_finite(want).sum()))
        for k in REPORTS[name]:
            assert np.array_equal(host(getattr(r, k)), ref[k]), (name, k, host(getattr(r, k)), ref[k])
        if name == "ground":
            for side in ("before", "after"):
                for k in GR.COUNTS:
                    assert np.array_equal(host(getattr(r, side)[k]), ref[side][k]), (name, side, k)
        print(f"[post_chain] P {name}: non-finite floats q {int(non_finite(got['q']).sum())}, pos {int(non_finite(got['pos']).sum())}, joints "
              f"{int(non_finite(got['joints']).sum())}; " + ", ".join(f"{k} {host(getattr(r, k)).ravel().tolist()}" for k in REPORTS[name]))
    # the poison stays where it was put: the NaN in q and nothing else there; in pos the frame's component of the clip's dancers and
    # nothing else (keep_apart's direction from an infinite root is Inf / Inf by include/tcdiff_apart.h, and 0 times it reaches that
    # component of the dancer and of its partners in that frame: held above, stage by stage)
    q, pos = host(final[0]), host(final[1])
    cq, t, dd, j, k = CH.POISON_Q
    assert int(non_finite(q).sum()) == 1 and np.isnan(q[cq, t * c.dn + dd, j, k])
    cp, t, dd, k = CH.POISON_POS
    bad = np.argwhere(non_finite(pos))
    assert non_finite(pos[cp, t * c.dn + dd, k]) and set(map(tuple, bad)) <= {(cp, t * c.dn + e, k) for e in range(c.dn)}


@pytest.mark.parametrize("poison", [False, True], ids=["N", "P"])
def test_a_clip_alone_gives_the_bits_it_has_in_the_batch(poison, diffusion):
    c = CH.case("N")
    clean, state, beats, parents, offsets = poisoned_state(c, diffusion)
    state = state if poison else clean
    _, whole = kernels(state, beats, c.dn, CH.STAGES, parents, offsets)
    for clip in range(c.clips):
        one = tuple(t[clip:clip + 1].contiguous() for t in state)
        _, alone = kernels(one, beats[clip:clip + 1], c.dn, CH.STAGES, parents, offsets)
        for x, y in zip(alone, whole):
            assert torch.equal(bits(x), bits(y[clip:clip + 1]))


def test_a_dancer_no_poison_reaches_keeps_the_bits_of_the_clean_run(diffusion):
    """By the headers a dancer's state reaches another's through keep_apart's pairs (include/tcdiff_apart.h), through a shared
    beat_sync warp (include/tcdiff_beatsync.h: with `share` the dancers of a clip share one warp, and render_sample shares) and through
    ground's floor, estimated from all the dancers of a clip (include/tcdiff_ground.h); smooth and foot_lock work dancer by dancer.
    So: through smooth and foot_lock alone every other dancer keeps every bit of the clean run.  Through the whole chain the poisoned
    dancers' clip-mates are excepted, and both clips of P hold poison: nothing is left to compare there, and the stage-locked test above
    is what holds that run."""
    c = CH.case("N")
    clean, state, beats, parents, offsets = poisoned_state(c, diffusion)
    on = ("smooth", "foot_lock")
    _, want = kernels(clean, beats, c.dn, on, parents, offsets)
    _, got = kernels(state, beats, c.dn, on, parents, offsets)
    keep = np.ones((c.clips, c.dn), bool)
    keep[CH.POISON_Q[0], CH.POISON_Q[2]] = keep[CH.POISON_POS[0], CH.POISON_POS[2]] = False
    assert keep.sum() == 4
    for g, w in zip(got[:2], want[:2]):
        g, w = SR.frames_of(host(g), c.dn), SR.frames_of(host(w), c.dn)
        assert np.array_equal(g.view(np.int32)[keep], w.view(np.int32)[keep]) and not np.array_equal(g.view(np.int32)[~keep], w.view(np.int32)[~keep])
    assert np.array_equal(host(got[2]).view(np.int32)[keep], host(want[2]).view(np.int32)[keep])


# ---- e. repeatability -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CASES)
def test_a_second_run_gives_the_same_bits(which, diffusion):
    c = CH.case(which)
    runs = []
    for _ in range(2):
        state, beats, parents, offsets = exported(c, diffusion)
        stages, final = kernels(state, beats, c.dn, CH.STAGES, parents, offsets, shift=True)
        runs.append([t for t in state + final if t is not None] + [v for name in CH.STAGES for v in stages[name][1] if isinstance(v, torch.Tensor)])
    assert len(runs[0]) == len(runs[1]) > 40
    for x, y in zip(*runs):
        assert torch.equal(bits(x), bits(y))
