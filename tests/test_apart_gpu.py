"""tcp_keep_apart (csrc/apart.hip) and tcdiff_amd/apart.py on an MI355X against the numpy float64 restatement tests/apart_ref.py.

Equality on every integer output.  On the float64 outputs -- shift, max_shift, max_step, gap_min_* -- the bound FLOAT_BOUND below: a
hundred times the largest difference measured (profiles/apart.txt), and never looser than 1e-9 m, a nanometre: 1/60 of float32's
resolution at one metre, above which the next check could not hold.  The difference measured is 0 in every case, so the bound is
equality: kernel and restatement do the same correctly rounded float64 operations (+, -, *, /, sqrt) in the same order, contraction
off, and the only reductions are minima and maxima, which round nothing.  The float32 outputs within one float32 ulp of the restatement's,
and frames whose shift is 0 bit-equal to the input.  No case is excluded: the restatement alone first shows (here again, and for
every input in tests/test_apart_cpu.py) that no discontinuous decision is a near-tie.

The cross-checks against group_metrics tie the two features together without trusting the new kernels: what keep_apart reports as
"after" is what group_metrics measures on the joints it returns, to the bit."""
import os
import pickle

import numpy as np
import pytest
import torch

import apart_ref as A
import footlock_ref as FR
import group_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import apart as P
from tcdiff_amd import export as E
from tcdiff_amd import footlock as F
from tcdiff_amd import kernels as K
from tcdiff_amd.group_metrics import group_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED, FLOAT_BOUND = A.MEASURED, A.FLOAT_BOUND          # in tests/apart_ref.py: tests/test_post_chain_gpu.py holds the chain to the same bound
INTS = ("contact_before", "contact_after", "pushed", "capped")
FLOATS = ("shift", "max_shift", "max_step", "gap_min_before", "gap_min_after")
_want = {}
_worst = {"f64": 0.0, "ulp": 0}


def _reference(pos, J, key, **kw):
    if key not in _want:
        ref = A.keep_apart(pos, J, details=True, **kw)
        ok, why = A.judge(ref)
        assert ok, f"a decision of the reference is a near-tie on these inputs: {why}"
        _want[key] = ref
    return _want[key]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # a copy: the shared inputs are read-only


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(a: P.Apart, b: P.Apart):
    for name, x, y in zip(P.Apart._fields, a, b):
        assert (x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))), name


def _ordered(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _compare(got: P.Apart, want, pos, J, what):
    b, dn, T = J.shape[:3]
    npairs = dn * (dn - 1) // 2
    assert isinstance(got, P.Apart) and got.pos.dtype == got.joints.dtype == torch.float32 and got.joints.is_contiguous()
    assert tuple(got.pos.shape) == (b, T * dn, 3) and tuple(got.joints.shape) == (b, dn, T, 24, 3) and tuple(got.shift.shape) == (b, dn, T, 2)
    for k in INTS:
        g = getattr(got, k)
        assert g.dtype == torch.int64 and tuple(g.shape) == (b, npairs) and np.array_equal(g.cpu().numpy(), want[k]), (what, k, g, want[k])
    worst = 0.0
    for k in FLOATS:
        g, w = getattr(got, k), want[k]
        assert g.dtype == torch.float64 and tuple(g.shape) == w.shape, (what, k)
        g = g.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k, g, w)
        err = np.abs(g - w)[~np.isnan(w)]
        worst = max(worst, float(err.max()) if err.size else 0.0)
    ulp = 0
    for g, w in ((got.pos.cpu().numpy(), want["pos"]), (got.joints.cpu().numpy(), want["joints"])):
        assert np.array_equal(np.isnan(g), np.isnan(w)), what
        ok = ~np.isnan(w)
        ulp = max(ulp, int(np.abs(_ordered(g) - _ordered(w))[ok].max()))
    _worst["f64"], _worst["ulp"] = max(_worst["f64"], worst), max(_worst["ulp"], ulp)
    print(f"[apart] {what}: float64 outputs within {worst:.3e} m of the restatement (bound {FLOAT_BOUND:.3e}), float32 within {ulp} ulp; "
          f"contact frames {int(want['contact_before'].sum())} -> {int(want['contact_after'].sum())}; so far {_worst['f64']:.3e} m, {_worst['ulp']} ulp")
    assert worst <= FLOAT_BOUND and ulp <= 1, (what, worst, ulp)
    still = (got.shift.cpu().numpy() == 0).all(-1)                                        # (b, dn, T): the copy rule
    assert np.array_equal(got.joints.cpu().numpy()[still].view(np.uint32), np.asarray(J)[still].view(np.uint32)), what
    rows = np.moveaxis(still, 1, 2).reshape(b, T * dn)
    assert np.array_equal(got.pos.cpu().numpy()[rows].view(np.uint32), np.asarray(pos)[rows].view(np.uint32)), what
    up = want.get("up", 2)
    assert np.array_equal(got.joints.cpu().numpy()[..., up].view(np.uint32), np.asarray(J)[..., up].view(np.uint32)), what


@pytest.mark.parametrize("by", [A.SPREAD, 0.0], ids=["spread", "unspread"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_float64_restatement(shape, by):
    """T = 1, 2: below blend + 1; 7: above it; 5 dancers x 70 frames: ten pairs; 2 clips x 150: several workgroups of four frames; 1125:
    a song, past the 256 threads of the reductions.  Spread: dancers that meet now and then (two dancers alone never do: the copy
    path); unspread: dancers that walk through each other, every path of the iteration, capped frames among them"""
    pos, J = A.spread(*shape, by=by)
    want = _reference(pos, J, (shape, by))
    got = P.keep_apart(_dev(pos), _dev(J), dn=shape[1], return_shift=True)
    _compare(got, want, pos, J, f"{shape} {'spread' if by else 'unspread'}")
    if by == 0.0 and shape[2] > 1:
        assert want["pushed"].sum() > 0 and (got.shift != 0).any()


def test_other_parameters():
    """up = 1 on permuted data, rounds 0 and 1, iterations 1, blend 0 and blend > T, a mobility with zeros, radii and a tree of the caller's"""
    for name, (pos, J), kw in A.parameter_cases():
        want = dict(_reference(pos, J, ("parameters", name), **kw), up=kw.get("up", 2))
        got = P.keep_apart(_dev(pos), _dev(J), dn=J.shape[1], return_shift=True, **kw)
        _compare(got, want, pos, J, name)
        if name == "mobility":
            assert not got.shift[:, [1, 3]].any() and got.shift[:, [0, 2, 4]].any()
        if name == "rounds=0":
            assert not got.shift.any() and torch.equal(got.contact_before, got.contact_after) and int(got.contact_before.sum()) > 0


def test_strided_views_are_read_in_place_and_runs_repeat():
    shape = (2, 3, 150)
    pos, J = (_dev(a) for a in A.spread(*shape, by=0.0))
    jv = J.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)          # (b, T, dn, 24, 3) storage: what tcdiff_pose_export writes
    assert not jv.is_contiguous() and torch.equal(jv, J)
    first = P.keep_apart(pos, J, dn=3, return_shift=True)
    _same_bits(P.keep_apart(pos, jv, dn=3, return_shift=True), first)
    _same_bits(P.keep_apart(pos, J, dn=3, return_shift=True), first)
    wide = torch.zeros(2, 3, 150, 30, 3, device=DEV)                            # a slice with larger outer strides
    wide[:, :, :, 3:27] = J
    _same_bits(P.keep_apart(pos, wide[:, :, :, 3:27], dn=3, return_shift=True), first)
    plain = P.keep_apart(pos, J, dn=3)                                          # the shift plane in the workspace
    assert plain.shift is None
    _same_bits(plain._replace(shift=first.shift), first)
    with pytest.raises(L.TcdiffError, match="contiguous"):
        P.keep_apart(pos, J.transpose(-1, -2).contiguous().transpose(-1, -2), dn=3)
    with pytest.raises(L.TcdiffError, match="one device"):
        P.keep_apart(pos.cpu(), J, dn=3)


def test_the_outputs_land_where_they_are_told_and_nothing_else_is_written():
    shape = (2, 3, 5)
    b, dn, T = shape
    npairs, pad = 3, 37
    pos, J = (_dev(a) for a in A.spread(*shape, by=0.0))
    public = P.keep_apart(pos, J, dn=dn, return_shift=True)
    buf, view = {}, {}
    for name, t in zip(P.Apart._fields, public):
        n = t.numel()
        buf[name] = torch.full((n + 2 * pad,), -77, dtype=t.dtype, device=DEV)
        view[name] = buf[name][pad:pad + n].view(t.shape)
    nbytes = K.keep_apart_workspace(b, dn, T)
    assert nbytes == (41 * b * npairs * T + 16 * b * dn * T + 7) // 8 * 8
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    for shift in (view["shift"], None):
        K.keep_apart(pos, J, 2, [0] + R.SMPL_PARENTS[1:], R.capsule_radii().tolist(), [1.0] * dn, 0.02, 8, 3, 5, 0.6, ws[:nbytes], view["pos"],
                     view["joints"], shift, view["contact_before"], view["contact_after"], view["gap_min_before"], view["gap_min_after"],
                     view["pushed"], view["capped"], view["max_shift"], view["max_step"])
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all())
        for k in buf:
            assert bool((buf[k][:pad] == -77).all()) and bool((buf[k][-pad:] == -77).all()), k
        _same_bits(P.Apart(**view), public)
    zero = torch.full((b, dn, T, 2), -77.0, dtype=torch.float64, device=DEV)   # no round: the shift plane handed in is cleared
    K.keep_apart(pos, J, 2, [0] + R.SMPL_PARENTS[1:], R.capsule_radii().tolist(), [1.0] * dn, 0.02, 8, 0, 5, 0.6, ws[:nbytes], view["pos"],
                 view["joints"], zero, view["contact_before"], view["contact_after"], view["gap_min_before"], view["gap_min_after"],
                 view["pushed"], view["capped"], view["max_shift"], view["max_step"])
    assert not zero.any() and torch.equal(_bits(view["joints"]), _bits(J)) and torch.equal(_bits(view["pos"]), _bits(pos))


def test_a_nan_joint_changes_its_own_frame_and_nothing_else():
    shape = (2, 3, 5)
    pos, clean = A.spread(*shape, by=0.0)
    J = clean.copy()
    J.view(np.uint32)[1, 0, 2, 20, 1] = 0x7FC12345                      # clip 1, dancer 0, frame 2, the left wrist: a NaN with a payload
    want = _reference(pos, J, "nan joint", blend=0)
    got = P.keep_apart(_dev(pos), _dev(J), dn=3, blend=0, return_shift=True)
    _compare(got, want, pos, J, "a NaN joint")
    base = P.keep_apart(_dev(pos), _dev(clean), dn=3, blend=0, return_shift=True)
    # with blend = 0 the frames are independent: clip 0 and the other frames of clip 1 keep their bits
    for x, y in ((got.joints, base.joints), (got.shift, base.shift)):
        keep = torch.ones(2, 3, 5, dtype=torch.bool, device=DEV)
        keep[1, :, 2] = False
        assert torch.equal(_bits(x)[keep], _bits(y)[keep])
    assert not got.shift[1, 0, 2].any() and int(got.joints.view(torch.int32)[1, 0, 2, 20, 1]) == 0x7FC12345          # neither pushed nor changed
    for k in INTS + ("gap_min_before", "gap_min_after"):                # the other clip: the same bits
        assert torch.equal(_bits(getattr(got, k))[0], _bits(getattr(base, k))[0]), k
    assert torch.equal(got.contact_before[1, 2], base.contact_before[1, 2])          # the pair without the dancer, before anything moves
    softer = P.keep_apart(_dev(pos), _dev(J), dn=3, return_shift=True)               # the default blend: the other clip is untouched still
    soft0 = P.keep_apart(_dev(pos), _dev(clean), dn=3, return_shift=True)
    assert torch.equal(_bits(softer.joints)[0], _bits(soft0.joints)[0]) and torch.equal(_bits(softer.shift)[0], _bits(soft0.shift)[0])
    assert int(torch.isnan(softer.joints).sum()) == 1


def test_group_metrics_measures_what_keep_apart_reports():
    for shape, by in (((1, 5, 70), A.SPREAD), ((2, 3, 150), 0.0)):
        pos, J = (_dev(a) for a in A.spread(*shape, by=by))
        T = shape[2]
        got = P.keep_apart(pos, J, dn=shape[1])
        after, before = group_metrics(got.joints), group_metrics(J)
        rate = lambda n: n.cpu().numpy().astype(np.float64) / float(T)          # the quotient on the host: one correctly rounded division
        assert np.array_equal(after["body_contact_rate"].cpu().numpy(), rate(got.contact_after))
        assert torch.equal(_bits(after["body_gap_min"]), _bits(got.gap_min_after))
        assert np.array_equal(before["body_contact_rate"].cpu().numpy(), rate(got.contact_before))
        assert torch.equal(_bits(before["body_gap_min"]), _bits(got.gap_min_before))
        assert int(got.contact_after.sum()) < int(got.contact_before.sum())
        assert torch.equal(got.pos.view(shape[0], T, shape[1], 3).permute(0, 2, 1, 3), got.joints[:, :, :, 0])          # pos follows its root


def test_one_dancer_is_returned_as_it_is():
    pos, J = (_dev(a) for a in A.spread(2, 3, 5))
    J1, pos1 = J[:, :1], pos.view(2, 5, 3, 3)[:, :, 0].contiguous()
    got = P.keep_apart(pos1, J1, dn=1, return_shift=True)
    assert got.pos is pos1 and got.joints is J1 and tuple(got.shift.shape) == (2, 1, 5, 2) and not got.shift.any()
    for k in INTS + ("gap_min_before", "gap_min_after"):
        assert tuple(getattr(got, k).shape) == (2, 0) and getattr(got, k).is_cuda
    assert got.max_shift.tolist() == [[0.0], [0.0]] == got.max_step.tolist()


# ---- with the foot lock, and through render_sample ---------------------------------------------------------------------------------------------
def test_keep_apart_then_foot_lock_pins_the_feet_of_the_shifted_motion():
    """the order render_sample takes: a shifted root slides a planted foot, and the foot lock run afterwards re-pins it"""
    import test_footlock_gpu as TF
    q, pos, contacts, blend, _ = FR.case("ends")
    T = q.shape[1] // FR.DN
    near = pos.copy().reshape(1, T, FR.DN, 3)
    near[:, :, 1] = near[:, :, 0] + np.float32([0.3, 0.0, 0.05])       # the second dancer walks beside the first, bodies overlapping
    near = near.reshape(1, T * FR.DN, 3)
    tq, tpos, tc = _dev(q), _dev(near), _dev(contacts)
    raw = F.foot_lock(tq, tpos, torch.zeros_like(tc), dn=FR.DN).joints          # every contact off: the FK of the poses as they are
    apart = P.keep_apart(tpos, raw, dn=FR.DN, up=1)
    assert int(apart.pushed.sum()) > 0 and int(apart.contact_after.sum()) < int(apart.contact_before.sum())
    assert torch.equal(apart.pos.view(1, T, FR.DN, 3).permute(0, 2, 1, 3), apart.joints[:, :, :, 0])
    locked = F.foot_lock(tq, apart.pos, tc, dn=FR.DN, blend=blend)
    moved = apart.pos.cpu().numpy()
    ref = FR.foot_lock(q, moved, contacts, dn=FR.DN, blend=blend)
    TF.check_against(locked, ref, "after keep_apart")
    P1 = TF.fk64(TF.frames_of(locked.q.cpu().numpy()), TF.frames_of(moved))
    worst = 0.0
    for leg, (h, k, a, e) in enumerate(FR.LEGS):                          # every planted, unclamped frame stands on the restatement's anchor
        g, st = ref["g"][:, :, leg], ref["status"][:, :, leg]
        pin = np.where((g == 2)[..., None], P1[..., e, :], P1[..., a, :])
        free = (g != 0) & (st != 2)
        assert free.any()
        worst = max(worst, float(np.linalg.norm(pin - ref["anchor"][:, :, leg], axis=-1)[free].max()))
    print(f"[apart] keep_apart then foot_lock: planted joints within {worst:.3e} m of their anchors (bound {TF.PIN_BOUND:g})")
    assert worst <= TF.PIN_BOUND
    assert np.abs(locked.joints.cpu().numpy()[:, :, :, 0] - apart.joints.cpu().numpy()[:, :, :, 0]).max() == 0          # the shifted roots stand


def test_render_sample_hands_the_shifted_motion_to_the_foot_lock_and_every_writer(tmp_path):
    import test_footlock_gpu as TF
    from tcdiff_amd import GaussianDiffusion
    from tcdiff_amd.gltf import write_glb_out
    DN = 2
    d = GaussianDiffusion.__new__(GaussianDiffusion)                      # render_sample of given samples asks nothing of the model
    torch.nn.Module.__init__(d)
    d.smpl = None
    x = torch.rand(2, 8 * DN, 151, generator=torch.Generator().manual_seed(5)) * 2 - 1
    x[:, ::3, :4] = 1.0                                                    # some rows declare every foot planted
    x[:, :, 4:7] *= 0.05                                                   # the roots within 0.2 m of each other: the bodies overlap
    x = x.to(DEV)
    assert d.keep_apart is False and d.foot_lock is False
    kw = dict(name=TF.NAMES, required_dancer_num=DN)
    d.render_sample(x, None, TF.NORM, 7, None, fk_out=str(tmp_path / "fk0"), glb_out=str(tmp_path / "glb0"), **kw)
    parents, offsets = d._skeleton(torch.device(DEV))
    q, pos, poses, contacts = E.export_poses(x, TF.NORM, "normal", DN, parents=parents, offsets=offsets)
    # both attributes off: the files of the export alone, byte for byte
    assert TF._files(tmp_path / "fk0") == TF._files(os.path.dirname(E.write_fk_out(str(tmp_path / "fkw"), "normal", 7, TF.NAMES, q, pos, poses)[0]))
    assert TF._files(tmp_path / "glb0") == TF._files(os.path.dirname(write_glb_out(str(tmp_path / "glbw"), "normal", 7, TF.NAMES, q, pos, DN,
                                                                                   parents=parents, offsets=offsets)[0]))
    apart = P.keep_apart(pos, poses, dn=DN, parents=parents)
    assert int(apart.pushed.sum()) > 0 and not torch.equal(apart.pos, pos)
    locked = F.foot_lock(q, apart.pos, contacts, dn=DN, parents=parents, offsets=offsets)
    for attrs, want_q, want_joints in ((dict(keep_apart=True), q, apart.joints), (dict(keep_apart=True, foot_lock=True), locked.q, locked.joints)):
        out = "_".join(attrs)
        try:
            for k in attrs:
                setattr(d, k, True)
            d.render_sample(x, None, TF.NORM, 7, None, fk_out=str(tmp_path / ("fk_" + out)), glb_out=str(tmp_path / ("glb_" + out)), **kw)
        finally:
            for k in attrs:
                delattr(d, k)                                              # back to the class attributes
        for c, name in enumerate(E.fk_out_names("normal", 7, TF.NAMES)):
            with open(tmp_path / ("fk_" + out) / name, "rb") as f:
                got = pickle.load(f)
            assert np.array_equal(got["smpl_poses"], want_q[c].cpu().numpy().reshape(-1, 72)), out
            assert np.array_equal(got["smpl_trans"], apart.pos[c].cpu().numpy()) and np.array_equal(got["full_pose"], want_joints[c].cpu().numpy()), out
        want = write_glb_out(str(tmp_path / ("glbw_" + out)), "normal", 7, TF.NAMES, want_q, apart.pos, DN, parents=parents, offsets=offsets)
        assert TF._files(tmp_path / ("glb_" + out)) == TF._files(os.path.dirname(want[0])) != TF._files(tmp_path / "glb0")
    assert d.keep_apart is False and d.foot_lock is False
    d.render_sample(x, None, TF.NORM, 7, None, fk_out=str(tmp_path / "fk2"), glb_out=str(tmp_path / "glb2"), **kw)
    assert TF._files(tmp_path / "fk2") == TF._files(tmp_path / "fk0") and TF._files(tmp_path / "glb2") == TF._files(tmp_path / "glb0")
