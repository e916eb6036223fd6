"""GPU checks of the beat synchroniser (tcdiff_amd/beat_sync.py, csrc/beatsync.hip) against the numpy restatement tests/beatsync_ref.py
of include/tcdiff_beatsync.h: equal bits on every decision and every float64 output, on pos and on the contacts; the rotations within a
bound measured against the restatement (the device's acos, sin and atan2 are not numpy's), the joints within a bound measured against a
float64 FK of the returned poses; motion_beats against motion_metrics; the seeded late dancers under the existing motion_metrics
kernel; the identity cases; a NaN dancer; two runs and a clip alone; render_sample; the refusals.  Run with -s for the figures kept in
profiles/beatsync.txt."""
import importlib
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import beatsync_ref as R
import smooth_ref as SR
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS
from tcdiff_amd.metrics import motion_metrics

B = importlib.import_module("tcdiff_amd.beat_sync")                # the package's attribute of this name is the function
pytestmark = pytest.mark.gpu
DEV = "cuda"
ROT_BOUND, FK_BOUND = R.ROT_BOUND, R.FK_BOUND          # in tests/beatsync_ref.py: tests/test_post_chain_gpu.py holds the chain to the same two
SHAPES = [(1, 1, 2), (1, 1, 4), (2, 3, 65), (1, 2, 257), (1, 3, 300)]
PER_WARP = ("warp", "speed", "kin", "status", "kin_count", "music_count", "matched", "dropped", "anchors", "shift_max", "rate_min", "rate_max",
            "rate_min_frame", "rate_max_frame")


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r, axis=-1)[..., None, None]
    Kx = np.zeros(r.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -r[..., 2], r[..., 1], r[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -r[..., 0], -r[..., 1], r[..., 0]
    small = th < 1e-6
    s = np.where(small, 1.0 - th ** 2 / 6, np.sin(th) / np.where(small, 1.0, th))
    c = np.where(small, 0.5 - th ** 2 / 24, (1 - np.cos(th)) / np.where(small, 1.0, th) ** 2)
    return np.eye(3) + s * Kx + c * (Kx @ Kx)


def fk64(q, pos):
    """a forward kinematics of its own: Rodrigues matrices, whole arrays at once"""
    local = rodrigues(q)
    off = np.asarray(SMPL_OFFSETS, np.float32).astype(np.float64)
    P, W = [None] * 24, [None] * 24
    for j in range(24):
        p = SMPL_PARENTS[j]
        if p < 0:
            P[j], W[j] = np.asarray(pos, np.float64), local[..., j, :, :]
        else:
            P[j] = P[p] + W[p] @ off[j]
            W[j] = W[p] @ local[..., j, :, :]
    return np.stack(P, -2)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared cases are read-only


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def npbits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def fields(s):
    """every tensor of a BeatSync, the two metric dicts flattened"""
    flat = [v for v in s[:20] if v is not None]
    return flat + [v for side in (s.before, s.after) if side is not None for v in side.values()]


def same_bits(a, b):
    fa, fb = fields(a), fields(b)
    return len(fa) == len(fb) and all(torch.equal(bits(x), bits(y)) for x, y in zip(fa, fb))


def input_joints(q, pos, beats, dn, contacts, out, share, **kw):
    """the launcher's `joints_in` of the call that gave `out` (BeatSync does not carry them), with every other output held to `out`'s bits"""
    b, T = q.shape[0], q.shape[1] // dn
    W = 1 if share else dn
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=DEV)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=DEV)
    w = B._table_on(float(kw.get("sigma_smooth", 5.0)), q.device)
    ws = torch.empty(K.beat_sync_workspace(b, dn, T), dtype=torch.uint8, device=DEV)
    o = dict(q=torch.empty_like(q), pos=torch.empty_like(pos), contacts=None if contacts is None else torch.empty_like(contacts),
             joints=torch.empty(b, dn, T, 24, 3, device=DEV), joints_in=torch.empty(b, dn, T, 24, 3, device=DEV), warp=f64(b, W, T),
             speed=f64(b, W, T - 1), kin=torch.empty(b, W, T, dtype=torch.uint8, device=DEV), status=i32(b, W), kin_count=i32(b, W),
             music_count=i32(b, W), matched=i32(b, W), dropped=i32(b, W), anchors=i32(b, W), shift_max=f64(b, W), rate_min=f64(b, W),
             rate_max=f64(b, W), rate_min_frame=i32(b, W), rate_max_frame=i32(b, W), moved=i32(b, dn), copied=i32(b, dn))
    K.beat_sync(q, pos, contacts, beats, b, dn, T, share, kw.get("max_shift", 7), kw.get("max_rate", 1.5), kw.get("strength", 1.0), (w.numel() - 1) // 2,
                w, SMPL_PARENTS, SMPL_OFFSETS, ws, *o.values())
    for k, v in o.items():
        if k != "joints_in" and v is not None:
            assert torch.equal(bits(v), bits(getattr(out, k))), k
    return o["joints_in"]


def check_against(out, q, pos, beats, dn, contacts, share, what, **kw):
    """every output of one call against the restatement of the same inputs (numpy), the speed taken from the device's own float32 joints
    of the input.  Returns the largest rotation and joint differences."""
    tq, tpos, tb, tc = (dev(a) for a in (q, pos, beats, contacts))
    Jin = input_joints(tq, tpos, tb, dn, tc, out, share, **kw).cpu().numpy()
    with np.errstate(invalid="ignore"):
        assert np.nanmax(np.abs(Jin - fk64(SR.frames_of(q, dn), SR.frames_of(pos, dn))), initial=0.0) <= FK_BOUND
    ref = R.beat_sync(q, pos, beats, dn, contacts=contacts, share=share, joints_in=Jin, **kw)
    b, T = q.shape[0], q.shape[1] // dn
    W = 1 if share else dn
    for k in PER_WARP + ("moved", "copied"):                                                  # equal bits: every decision, every float64
        got = getattr(out, k).cpu().numpy()
        assert got.shape == ref[k].shape and got.dtype == ref[k].dtype, (k, got.shape, got.dtype, ref[k].shape, ref[k].dtype)
        assert np.array_equal(npbits(got), npbits(ref[k])), (what, k)
    assert out.warp.shape == (b, W, T) and out.moved.shape == (b, dn)
    got_q, got_pos = out.q.cpu().numpy(), out.pos.cpu().numpy()
    assert got_q.shape == q.shape and got_pos.shape == pos.shape and got_q.dtype == got_pos.dtype == np.float32
    assert np.array_equal(npbits(got_pos), npbits(ref["pos"]))
    if contacts is None:
        assert out.contacts is None
    else:
        assert np.array_equal(npbits(out.contacts.cpu().numpy()), npbits(ref["contacts"]))
    warp = np.repeat(ref["warp"], dn, 1) if share else ref["warp"]                           # (b, dn, T)
    slerped = SR.rows_of(np.broadcast_to((warp != np.floor(warp))[..., None], (b, dn, T, 24))) & np.isfinite(ref["q64"]).all(-1)
    assert np.array_equal(npbits(got_q)[~slerped], npbits(ref["q"])[~slerped])                # copies: the input's words
    with np.errstate(invalid="ignore"):
        ang = SR.angles(got_q.astype(np.float64), ref["q64"])
    rot = float(ang[slerped].max()) if slerped.any() else 0.0
    joints = out.joints.cpu().numpy()
    assert joints.shape == (b, dn, T, 24, 3) and joints.dtype == np.float32
    with np.errstate(invalid="ignore"):
        fk = float(np.nanmax(np.abs(joints - fk64(SR.frames_of(got_q, dn), SR.frames_of(got_pos, dn))), initial=0.0))
    print(f"[beatsync] {what}: rotations {rot:.2e} rad from the restatement (bound {ROT_BOUND:.1e}), joints {fk:.2e} m from a float64 FK (bound "
          f"{FK_BOUND:.1e}); anchors {ref['anchors'].ravel().tolist()} of {ref['matched'].ravel().tolist()} matched, "
          f"{ref['music_count'].ravel().tolist()} music and {ref['kin_count'].ravel().tolist()} kinematic beats, moved {ref['moved'].ravel().tolist()}")
    assert rot <= ROT_BOUND and fk <= FK_BOUND
    if out.before is not None:
        sg = float(kw.get("sigma_smooth", 5.0))
        again = motion_metrics(dev(Jin), beats=tb, sigma_smooth=sg)
        assert all(torch.equal(bits(out.before[k]), bits(again[k])) for k in again)
        again = motion_metrics(out.joints, beats=tb, sigma_smooth=sg)
        assert all(torch.equal(bits(out.after[k]), bits(again[k])) for k in again)
    return rot, fk


# ---- against the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_contacts", [True, False])
@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_beat_sync_against_the_restatement(shape, share, with_contacts):
    b, dn, T = shape
    q, pos, contacts, beats = R.case(b, dn, T)
    contacts = contacts if with_contacts else None
    tq, tpos, tb, tc = (dev(a) for a in (q, pos, beats, contacts))
    q0, p0 = tq.clone(), tpos.clone()
    out = B.beat_sync(tq, tpos, tb, dn=dn, contacts=tc, share=share)
    assert isinstance(out, B.BeatSync) and torch.equal(bits(tq), bits(q0)) and torch.equal(bits(tpos), bits(p0))      # the inputs are not written
    assert out.q.data_ptr() != tq.data_ptr()
    check_against(out, q, pos, beats, dn, contacts, share, f"{shape} share={share} contacts={with_contacts}")
    if T >= 65:
        assert int(out.anchors.sum()) > 0 and int(out.moved.sum()) > 0
    assert same_bits(out, B.beat_sync(tq, tpos, tb, dn=dn, contacts=tc, share=share))                                # two calls, equal bits
    bare = B.beat_sync(tq, tpos, tb, dn=dn, contacts=tc, share=share, measure=False)
    assert bare.before is None and bare.after is None and same_bits(bare, out._replace(before=None, after=None))


def test_other_parameters_and_a_clip_alone():
    b, dn, T = 2, 3, 65
    q, pos, contacts, beats = R.case(b, dn, T)
    kw = dict(max_shift=3, max_rate=1.2, strength=0.5, sigma_smooth=3.0)
    tq, tpos, tb, tc = (dev(a) for a in (q, pos, beats, contacts))
    for share in (True, False):
        out = B.beat_sync(tq, tpos, tb, dn=dn, contacts=tc, share=share, **kw)
        check_against(out, q, pos, beats, dn, contacts, share, f"other parameters share={share}", **kw)
        for c in range(b):                                                                        # a clip alone: the same bits as in the batch
            alone = B.beat_sync(tq[c:c + 1], tpos[c:c + 1], tb[c:c + 1], dn=dn, contacts=tc[c:c + 1], share=share, **kw)
            for x, y in zip(fields(alone), fields(out)):
                assert torch.equal(bits(x), bits(y[c:c + 1]))


# ---- motion_beats ----------------------------------------------------------------------------------------------------------------------------------
def test_motion_beats_is_motion_metrics_count_and_reads_a_view_in_place():
    for name, (q, pos, beats, dn) in (("seeded dance", R.case(2, 3, 150)[:2] + (R.case(2, 3, 150)[3], 3)), ("late dancers", R.late_dancers()[:3] + (3,))):
        b, T = q.shape[0], q.shape[1] // dn
        J = fk64(q.reshape(b, T, dn, 24, 3), pos.reshape(b, T, dn, 3)).astype(np.float32)          # frame-major, as the export's launch writes it
        view = dev(J).permute(0, 2, 1, 3, 4)
        assert not view.is_contiguous()
        got, same = B.motion_beats(view), B.motion_beats(view.contiguous())
        assert all(torch.equal(bits(got[k]), bits(same[k])) for k in got) and list(got) == ["speed", "kin", "kin_count"]
        mm = motion_metrics(view, beats=dev(beats))
        assert got["kin_count"].dtype == torch.int32 and torch.equal(got["kin_count"].long(), mm["motion_beats"]) and int(got["kin_count"].min()) > 0
        for share in (False, True):
            out, ref = B.motion_beats(view, share=share), R.motion_beats(np.moveaxis(J, 1, 2), share=share)
            for k in ("speed", "kin", "kin_count"):
                assert np.array_equal(npbits(out[k].cpu().numpy()), npbits(ref[k])), (name, share, k)
            assert torch.equal(out["kin"].sum(-1).int(), out["kin_count"])
        print(f"[beatsync] motion_beats, {name}: kin_count {got['kin_count'].cpu().tolist()} = motion_metrics' motion_beats; speed, kin equal the restatement's")


# ---- what it is for ------------------------------------------------------------------------------------------------------------------------------
def test_the_late_dancers_come_onto_the_beat_on_the_device():
    q, pos, beats, lags = R.late_dancers()
    dn = len(lags)
    for share in (False, True):
        out = B.beat_sync(dev(q), dev(pos), dev(beats), dn=dn, share=share)
        before, after = out.before["beat_align"].cpu().numpy(), out.after["beat_align"].cpu().numpy()
        print(f"[beatsync] late dancers (lags {lags.tolist()}, share={share}): beat_align {before.round(3).tolist()} -> {after.round(3).tolist()}, "
              f"matched {out.matched.cpu().tolist()}, anchors {out.anchors.cpu().tolist()}, shift_max {out.shift_max.cpu().round(decimals=2).tolist()}")
        assert (after > before).all() and int(out.matched.min()) > 0
        check_against(out, q, pos, beats, dn, None, share, f"late dancers share={share}")


# ---- the identity cases -----------------------------------------------------------------------------------------------------------------------------
def test_strength_0_and_silent_beats_return_the_input_bit_for_bit():
    q, pos, contacts, beats = R.case(2, 3, 65)
    tq, tpos, tc = dev(q), dev(pos), dev(contacts)
    for share in (True, False):
        for what, tb, kw in (("strength=0", dev(beats), dict(strength=0.0)), ("silent", dev(np.zeros_like(beats)), {})):
            out = B.beat_sync(tq, tpos, tb, dn=3, contacts=tc, share=share, **kw)
            assert torch.equal(bits(out.q), bits(tq)) and torch.equal(bits(out.pos), bits(tpos)) and torch.equal(bits(out.contacts), bits(tc)), what
            assert not out.moved.any() and not out.copied.any() and not out.shift_max.any()
            assert torch.equal(out.warp, torch.arange(65, dtype=torch.float64, device=DEV).expand_as(out.warp))
            assert (int(out.anchors.sum()) > 0) == (what == "strength=0") and (int(out.music_count.sum()) == 0) == (what == "silent")
            assert all(torch.equal(bits(out.before[k]), bits(out.after[k])) for k in out.before)


def test_a_nan_dancer_is_copied_through_and_no_other_dancers_bits_change():
    b, dn, T = 2, 3, 65
    q, pos, contacts, beats = R.case(b, dn, T)
    qn = np.array(q)
    qn[1, 30 * dn + 1, 0, 2] = np.nan                          # clip 1, dancer 1, frame 30, the root's rotation: every joint of the frame
    clean = B.beat_sync(dev(q), dev(pos), dev(beats), dn=dn, contacts=dev(contacts), share=False, measure=False)
    out = B.beat_sync(dev(qn), dev(pos), dev(beats), dn=dn, contacts=dev(contacts), share=False, measure=False)
    assert out.status.cpu().tolist() == [[0, 0, 0], [0, 1, 0]] and int(out.kin_count[1, 1]) == 0 and int(out.moved[1, 1]) == 0
    assert bool(torch.isnan(out.speed[1, 1]).all()) and int(out.copied[1, 1]) == 0
    fo, fi = SR.frames_of(out.q.cpu().numpy(), dn), SR.frames_of(qn, dn)
    assert np.array_equal(npbits(fo[1, 1]), npbits(fi[1, 1]))                                  # the copy-through, the NaN's word included
    assert np.array_equal(npbits(SR.frames_of(out.pos.cpu().numpy(), dn)[1, 1]), npbits(SR.frames_of(pos, dn)[1, 1]))
    assert torch.equal(bits(out.contacts[1, 1]), bits(dev(contacts)[1, 1]))
    keep = np.ones((b, dn), bool)
    keep[1, 1] = False
    for k in ("warp", "speed", "kin", "status", "kin_count", "matched", "anchors", "rate_min", "rate_max", "shift_max", "moved", "copied", "joints", "contacts"):
        assert torch.equal(bits(getattr(out, k))[torch.from_numpy(keep).to(DEV)], bits(getattr(clean, k))[torch.from_numpy(keep).to(DEV)]), k
    fc = SR.frames_of(clean.q.cpu().numpy(), dn)
    assert np.array_equal(npbits(fo[keep]), npbits(fc[keep]))
    check_against(out, qn, pos, beats, dn, contacts, False, "a NaN dancer")
    pooled = B.beat_sync(dev(qn), dev(pos), dev(beats), dn=dn, share=True, measure=False)        # pooled: the whole clip is copied through
    assert pooled.status.cpu().tolist() == [[0], [1]] and torch.equal(bits(pooled.q[1]), bits(dev(qn)[1])) and int(pooled.moved[0].min()) > 0
    # a non-finite float that the speed does not see (a leaf's rotation moves no joint): the outputs that need it are copied through
    ql = np.array(q)
    ql[0, 20 * dn + 2, 22, 1] = np.inf
    out = B.beat_sync(dev(ql), dev(pos), dev(beats), dn=dn, share=False, measure=False)
    assert out.status.cpu().tolist() == [[0, 0, 0]] * 2 and int(out.copied.sum()) == int(out.copied[0, 2])
    check_against(out, ql, pos, beats, dn, None, False, "a non-finite leaf rotation")


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def _normalizer(scale, min_):
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_, n.scaler.min_ = scale.float(), min_.float()
    return n


DN = 2
NORM = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
NAMES = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]


@pytest.fixture(scope="module")
def diffusion():
    """the small model tests/test_footlock_gpu.py builds, built again here"""
    from oracle import tcdiff_oracle as O
    from tcdiff_amd import DanceDecoder, GaussianDiffusion
    seq = 60
    sd = O.synth_state_dict(dn=DN, seq_len=seq)
    model = DanceDecoder(nfeats=151, seq_len=seq, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=TF.gelu, required_dancer_num=DN)
    model.load_state_dict(sd)
    return GaussianDiffusion(model, seq, 151, None, schedule="cosine", n_timestep=100, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=seq).to(DEV).eval()


def _files(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


def _pickles(folder):
    out = []
    for name in E.fk_out_names("normal", 7, NAMES):
        with open(os.path.join(folder, name), "rb") as f:
            out.append(pickle.load(f))
    return out


def test_render_sample_retimes_before_every_corrector_and_writer(diffusion, tmp_path):
    T = 60
    g = torch.Generator().manual_seed(5)
    t = torch.arange(T)[None, :, None, None]
    # every channel moves as A cos(pi (t - 2) / 12): whatever the map from channels to joints, every joint rests at t = 2 + 12 n
    x = ((1.2 * torch.rand(2, 1, DN, 151, generator=g) - 0.6) * torch.cos(np.pi * (t - 2) / 12.0)).reshape(2, T * DN, 151)
    x[:, ::3, :4] = 1.0                                                    # some rows declare every foot planted
    cond = torch.zeros(2, 2 * T, 438)
    cond[:, 24::24, 53] = 1.0                                              # a music beat every 12 motion frames, 2 before the dancers rest
    kw = dict(name=NAMES, required_dancer_num=DN)
    cls = type(diffusion)
    assert diffusion.beat_sync is False and cls.beat_sync is False

    def absent(self):
        raise AttributeError("beat_sync")
    Without = type("Without", (cls,), {"beat_sync": property(absent)})    # the class as it was before the attribute existed
    try:
        diffusion.__class__ = Without
        assert not hasattr(diffusion, "beat_sync")
        diffusion.render_sample(x, cond, NORM, 7, None, fk_out=str(tmp_path / "fk_absent"), glb_out=str(tmp_path / "glb_absent"), **kw)
    finally:
        diffusion.__class__ = cls
    diffusion.render_sample(x, cond, NORM, 7, None, fk_out=str(tmp_path / "fk0"), glb_out=str(tmp_path / "glb0"), **kw)
    assert _files(tmp_path / "fk0") == _files(tmp_path / "fk_absent") and _files(tmp_path / "glb0") == _files(tmp_path / "glb_absent")
    parents, offsets = diffusion._skeleton(torch.device(DEV))
    q, pos, poses, contacts = E.export_poses(x.to(DEV), NORM, "normal", DN, parents=parents, offsets=offsets)
    from tcdiff_amd.metrics import beats_from_cond
    beats = beats_from_cond(cond.to(DEV), T)
    assert beats.cpu().nonzero()[:, 1].tolist() == [12, 24, 36, 48] * 2
    want = B.beat_sync(q, pos, beats, dn=DN, contacts=contacts, parents=parents, offsets=offsets)
    assert int(want.anchors.sum()) > 0 and not torch.equal(want.q, q) and not torch.equal(want.pos, pos)
    try:
        diffusion.beat_sync = True
        diffusion.render_sample(x, cond, NORM, 7, None, fk_out=str(tmp_path / "fk1"), glb_out=str(tmp_path / "glb1"), **kw)
        with pytest.raises(L.TcdiffError, match="beat_sync reads the music's beats from cond"):
            diffusion.render_sample(x, None, NORM, 7, None, fk_out=str(tmp_path / "fk_none"), **kw)
    finally:
        del diffusion.beat_sync                                            # back to the class attribute
    for c, d in enumerate(_pickles(tmp_path / "fk1")):
        assert np.array_equal(d["smpl_poses"], want.q[c].cpu().numpy().reshape(-1, 72)) and np.array_equal(d["smpl_trans"], want.pos[c].cpu().numpy())
        assert np.array_equal(d["full_pose"], want.joints[c].cpu().numpy())
    from tcdiff_amd.gltf import write_glb_out
    glb = write_glb_out(str(tmp_path / "glbw"), "normal", 7, NAMES, want.q, want.pos, DN, parents=parents, offsets=offsets)
    assert _files(tmp_path / "glb1") == _files(os.path.dirname(glb[0])) != _files(tmp_path / "glb0")
    # with the filter and the foot lock as well: both act on the retimed poses and contacts
    from tcdiff_amd.footlock import foot_lock
    from tcdiff_amd.smooth import smooth
    smoothed = smooth(want.q, want.pos, dn=DN, parents=parents, offsets=offsets, measure=False)
    locked = foot_lock(smoothed.q, smoothed.pos, want.contacts, dn=DN, parents=parents, offsets=offsets)
    try:
        diffusion.beat_sync = diffusion.smooth = diffusion.foot_lock = True
        diffusion.render_sample(x, cond, NORM, 7, None, fk_out=str(tmp_path / "fk_all"), **kw)
    finally:
        del diffusion.beat_sync, diffusion.smooth, diffusion.foot_lock
    for c, d in enumerate(_pickles(tmp_path / "fk_all")):
        assert np.array_equal(d["smpl_poses"], locked.q[c].cpu().numpy().reshape(-1, 72)) and np.array_equal(d["smpl_trans"], smoothed.pos[c].cpu().numpy())
        assert np.array_equal(d["full_pose"], locked.joints[c].cpu().numpy())
    assert diffusion.beat_sync is False
    diffusion.render_sample(x, cond, NORM, 7, None, fk_out=str(tmp_path / "fk2"), **kw)
    assert _files(tmp_path / "fk2") == _files(tmp_path / "fk0")


def test_refusals_on_the_device():
    q, pos, contacts, beats = R.case(1, 2, 4)
    with pytest.raises(L.TcdiffError, match="one device"):
        B.beat_sync(dev(q), dev(pos).cpu(), dev(beats), dn=2)
    with pytest.raises(L.TcdiffError, match="one device"):
        B.beat_sync(dev(q), dev(pos), dev(beats).cpu(), dn=2)
    with pytest.raises(L.TcdiffError, match="one device"):
        B.beat_sync(dev(q), dev(pos), dev(beats), dn=2, contacts=dev(contacts).cpu())
    with pytest.raises(L.TcdiffError, match=r"beats must be \(1, 4\) uint8"):
        B.beat_sync(dev(q), dev(pos), dev(beats)[:, :3], dn=2)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        B.motion_beats(torch.zeros(1, 1, 6, 24, 3))
    with pytest.raises(L.TcdiffError, match="TC_BEATSYNC_MAX_FRAMES"):
        B.motion_beats(torch.zeros(1, 1, 4097, 24, 3, device=DEV))
