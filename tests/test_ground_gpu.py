"""tcf_ground / tcf_ground_metrics (csrc/ground.hip) and tcdiff_amd/ground.py on an MI355X against the numpy float64 restatement
tests/ground_ref.py.

Equality on every integer output.  On the float64 outputs -- floor, shift, max_shift, max_step and the three values of "before" and
"after" -- the bound FLOAT_BOUND below: a hundred times the largest difference measured (profiles/ground.txt), and never looser than
1e-9 m.  The difference measured is 0 in every case, so the bound is equality: kernel and restatement do the same correctly rounded
float64 operations (+, -, *, /, sqrt) in the same order, contraction off; the minima, maxima and the median round nothing, and the
sums run in ascending frame order in both.  The float32 outputs within one float32 ulp of the restatement's, frames whose shift is 0
and the components that are not `up` bit-equal to the input.  No case is excluded: the restatement alone first shows (here again,
and for every input in tests/test_ground_cpu.py) that no discontinuous decision is a near-tie.

ground_metrics on the joints ground returns reproduces ground's "after" to the bit: the two entry points share the kernels that
measure, and "after" is measured on the float32 words that are returned."""
import importlib
import os
import pickle

import numpy as np
import pytest
import torch

import footlock_ref as FR
import ground_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import footlock as F
from tcdiff_amd import kernels as K

P = importlib.import_module("tcdiff_amd.ground")          # the module: the package's attribute `ground` is the function
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED, FLOAT_BOUND = R.MEASURED, R.FLOAT_BOUND          # in tests/ground_ref.py: tests/test_post_chain_gpu.py holds the chain to the same bound
_want = {}
_worst = {"f64": 0.0, "ulp": 0}


def _reference(key, pos, J, Cn, **kw):
    if key not in _want:
        ref = R.ground(pos, J, Cn, details=True, **kw)
        ok, why = R.judge(ref)
        assert ok, f"a decision of the reference is a near-tie on these inputs: {why}"
        _want[key] = ref
    return _want[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)          # a copy: the shared inputs are read-only


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(x, y, what):
    assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y)), what


def _same_bits(a, b):
    for name, x, y in zip(P.Ground._fields, a, b):
        if isinstance(x, dict):
            for k in P.METRICS:
                _same(x[k], y[k], (name, k))
        elif x is None or y is None:
            assert x is None and y is None, name
        else:
            _same(x, y, name)


def _ordered(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _close(g, w, what):
    """a float64 output against the restatement's: NaN where it has NaN, elsewhere within FLOAT_BOUND; -> the largest difference"""
    g = g.cpu().numpy()
    assert g.dtype == np.float64 and g.shape == w.shape, what
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, g, w)
    err = np.abs(g - w)[~np.isnan(w)]
    return float(err.max()) if err.size else 0.0


def _metrics_match(got, want, what):
    worst = 0.0
    for k in R.COUNTS:
        g = got[k]
        assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), want[k]), (what, k, g, want[k])
    for k in R.VALUES + ("floor",):
        worst = max(worst, _close(got[k], want[k], (what, k)))
    return worst


def _compare(got: P.Ground, want, pos, J, what, up=2):
    b, dn, T = J.shape[:3]
    assert isinstance(got, P.Ground) and got.pos.dtype == got.joints.dtype == torch.float32 and got.joints.is_contiguous()
    assert tuple(got.pos.shape) == (b, T * dn, 3) and tuple(got.joints.shape) == (b, dn, T, 24, 3) and tuple(got.shift.shape) == (b, dn, T)
    assert set(got.before) == set(got.after) == set(P.METRICS)
    assert got.capped.dtype == torch.int64 and np.array_equal(got.capped.cpu().numpy(), want["capped"]), (what, "capped")
    worst = max(_metrics_match(got.before, want["before"], what + " before"), _metrics_match(got.after, want["after"], what + " after"))
    for k in ("floor", "shift", "max_shift", "max_step"):
        worst = max(worst, _close(getattr(got, k), want[k], (what, k)))
    ulp = 0
    for g, w in ((got.pos.cpu().numpy(), want["pos"]), (got.joints.cpu().numpy(), want["joints"])):
        assert np.array_equal(np.isnan(g), np.isnan(w)), what
        ok = ~np.isnan(w)
        ulp = max(ulp, int(np.abs(_ordered(g) - _ordered(w))[ok].max()))
    _worst["f64"], _worst["ulp"] = max(_worst["f64"], worst), max(_worst["ulp"], ulp)
    print(f"[ground] {what}: float64 outputs within {worst:.3e} of the restatement (bound {FLOAT_BOUND:.3e}), float32 within {ulp} ulp; "
          f"penetration frames {int(want['before']['penetration_frames'].sum())} -> {int(want['after']['penetration_frames'].sum())}, "
          f"capped {int(want['capped'].sum())}; so far {_worst['f64']:.3e}, {_worst['ulp']} ulp")
    assert worst <= FLOAT_BOUND and ulp <= 1, (what, worst, ulp)
    still = got.shift.cpu().numpy() == 0                                                 # (b, dn, T): the copy rule
    assert np.array_equal(got.joints.cpu().numpy()[still].view(np.uint32), np.asarray(J)[still].view(np.uint32)), what
    rows = np.moveaxis(still, 1, 2).reshape(b, T * dn)
    assert np.array_equal(got.pos.cpu().numpy()[rows].view(np.uint32), np.asarray(pos)[rows].view(np.uint32)), what
    flat = [k for k in range(3) if k != up]
    assert np.array_equal(got.joints.cpu().numpy()[..., flat].view(np.uint32), np.asarray(J)[..., flat].view(np.uint32)), what
    assert np.array_equal(got.pos.cpu().numpy()[..., flat].view(np.uint32), np.asarray(pos)[..., flat].view(np.uint32)), what


@pytest.mark.parametrize("variant", R.variants(), ids=lambda v: v[0].replace(" ", "").replace(",", "-"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_float64_restatement(shape, variant):
    """T = 1, 2: below blend + 1; 7: above it; 2 clips x 3 dancers: the last clip without a planted frame (the median of the body
    lows); 5 dancers x 70 frames; 2 clips x 150: the workload's clip length; 1125: past 256 threads in the median (4500 candidates, the
    keys past TC_GROUND_MEDIAN_KEYS read again from the workspace) and past one wave of frames in the walks.  The floor estimated and
    given, the contacts given and the still rule."""
    pos, J, Cn = R.seeded(*shape)
    name, with_contacts, floor = variant
    c = Cn if with_contacts else None
    want = _reference((shape, name), pos, J, c, floor=floor)
    got = P.ground(_dev(pos), _dev(J), _dev(c), dn=shape[1], floor=floor, return_shift=True)
    _compare(got, want, pos, J, f"{shape} {name}")
    alone = P.ground_metrics(_dev(J), _dev(c), floor=floor)                 # launches 1, 2 and 5 alone: "before"
    assert set(alone) == set(P.METRICS) and _metrics_match(alone, want["before"], f"{shape} {name} ground_metrics") <= FLOAT_BOUND
    if shape[2] >= 7:
        assert int(got.capped.sum()) > 0 and int(got.before["penetration_frames"].sum()) > int(got.after["penetration_frames"].sum())


def test_other_parameters():
    """blend 0 and blend > T, up = 1 on permuted data, another max_lift and tolerance; each with the contacts and with the still rule"""
    for name, (pos, J, Cn), kw in R.parameter_cases():
        for c in (Cn, None):
            what = f"{name}, {'contacts' if c is not None else 'still rule'}"
            want = _reference(("parameters", what), pos, J, c, **kw)
            got = P.ground(_dev(pos), _dev(J), _dev(c), dn=J.shape[1], return_shift=True, **kw)
            _compare(got, want, pos, J, what, up=kw.get("up", 2))


def test_strided_views_are_read_in_place_and_runs_repeat():
    shape = (2, 3, 150)
    pos, J, Cn = (_dev(a) for a in R.seeded(*shape))
    jv = J.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)          # (b, T, dn, 24, 3) storage: what tcdiff_pose_export writes
    cv = Cn.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not jv.is_contiguous() and torch.equal(_bits(jv), _bits(J)) and not cv.is_contiguous()          # the words: J holds a NaN
    first = P.ground(pos, J, Cn, dn=3, return_shift=True)
    _same_bits(P.ground(pos, jv, cv, dn=3, return_shift=True), first)
    _same_bits(P.ground(pos, J, Cn, dn=3, return_shift=True), first)
    wide = torch.zeros(2, 3, 150, 30, 3, device=DEV)                            # a slice with larger outer strides
    wide[:, :, :, 3:27] = J
    _same_bits(P.ground(pos, wide[:, :, :, 3:27], Cn, dn=3, return_shift=True), first)
    plain = P.ground(pos, J, Cn, dn=3)                                          # the shift plane in the workspace
    assert plain.shift is None
    _same_bits(plain._replace(shift=first.shift), first)
    given = P.ground(pos, J, Cn, dn=3, floor=first.floor.clone(), return_shift=True)          # the floor as a tensor: the median skipped
    _same_bits(given, first)
    number = P.ground(pos, J, Cn, dn=3, floor=0.01, return_shift=True)
    _same_bits(P.ground(pos, J, Cn, dn=3, floor=torch.full((2,), 0.01, dtype=torch.float64, device=DEV), return_shift=True), number)
    for k in P.METRICS:
        _same(P.ground_metrics(jv, cv)[k], first.before[k], k)
    with pytest.raises(L.TcdiffError, match="contiguous"):
        P.ground(pos, J.transpose(-1, -2).contiguous().transpose(-1, -2), dn=3)
    with pytest.raises(L.TcdiffError, match="one device"):
        P.ground(pos.cpu(), J, dn=3)


def test_the_outputs_land_where_they_are_told_and_nothing_else_is_written():
    shape = (2, 3, 5)
    b, dn, T = shape
    pad = 37
    pos, J, Cn = (_dev(a) for a in R.seeded(*shape))
    public = P.ground(pos, J, Cn, dn=dn, return_shift=True)
    names = ("pos", "joints", "shift", "floor", "cb", "vb", "ca", "va", "capped", "max_shift", "max_step")
    like = dict(pos=public.pos, joints=public.joints, shift=public.shift, floor=public.floor, capped=public.capped, max_shift=public.max_shift,
                max_step=public.max_step, cb=torch.empty(3, b, dn, dtype=torch.int64), ca=torch.empty(3, b, dn, dtype=torch.int64),
                vb=torch.empty(3, b, dn, dtype=torch.float64), va=torch.empty(3, b, dn, dtype=torch.float64))
    buf, view = {}, {}
    for name in names:
        t = like[name]
        buf[name] = torch.full((t.numel() + 2 * pad,), -77, dtype=t.dtype, device=DEV)
        view[name] = buf[name][pad:pad + t.numel()].view(t.shape)
    nbytes = K.ground_workspace(b, dn, T)
    assert nbytes == (73 * b * dn * T + 7) // 8 * 8
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    parents = [0] + list(R.G.SMPL_PARENTS[1:])
    for shift in (view["shift"], None):
        K.ground(pos, J, Cn, 2, parents, R.G.capsule_radii().tolist(), None, 0.95, 0.01, 0.005, 5, 0.5, ws[:nbytes], view["pos"], view["joints"],
                 shift, view["floor"], view["cb"], view["vb"], view["ca"], view["va"], view["capped"], view["max_shift"], view["max_step"])
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all())
        for k in names:
            if k == "shift" and shift is None:
                continue
            assert bool((buf[k][:pad] == -77).all()) and bool((buf[k][-pad:] == -77).all()), k
        got = P.Ground(view["pos"], view["joints"], view["floor"], P._metrics(view["floor"], view["cb"], view["vb"]),
                       P._metrics(view["floor"], view["ca"], view["va"]), view["capped"], view["max_shift"], view["max_step"],
                       public.shift if shift is None else view["shift"])
        _same_bits(got, public)
    for k in ("floor", "cb", "vb"):                                              # ground_metrics into the same sentinels
        buf[k].fill_(-77)
    K.ground_metrics(J, Cn, 2, parents, R.G.capsule_radii().tolist(), None, 0.95, 0.01, 0.005, ws[:nbytes], view["floor"], view["cb"], view["vb"])
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all())
    for k in ("floor", "cb", "vb"):
        assert bool((buf[k][:pad] == -77).all()) and bool((buf[k][-pad:] == -77).all()), k
    for k, v in P._metrics(view["floor"], view["cb"], view["vb"]).items():
        _same(v, public.before[k], k)


def test_a_nan_frame_changes_its_own_frame_and_nothing_else():
    """with blend = 0, the floor given and the frame unplanted, the frames of a dancer are independent: the NaN frame keeps its words
    and its shift is 0, every other frame keeps the bits of the run without it"""
    shape = (2, 3, 150)
    pos, Jc, Cn = R.seeded(*shape)
    clean = np.array(Jc)
    bad_t = R.windows(150)[4]
    clean[:, 2, bad_t, 15, 0] = clean[:, 2, bad_t - 1, 15, 0]                 # the seeded NaN replaced: a clean input
    t0 = 150 // 2                                                             # inside the long unplanted stretch
    assert not Cn[1, 0, t0].any()
    J = clean.copy()
    J.view(np.uint32)[1, 0, t0, 20, 1] = 0x7FC12345                          # clip 1, dancer 0, the left wrist: a NaN with a payload
    want = _reference("nan frame", pos, J, Cn, blend=0, floor=0.01)
    got = P.ground(_dev(pos), _dev(J), _dev(Cn), dn=3, blend=0, floor=0.01, return_shift=True)
    _compare(got, want, pos, J, "a NaN frame")
    base = P.ground(_dev(pos), _dev(clean), _dev(Cn), dn=3, blend=0, floor=0.01, return_shift=True)
    keep = torch.ones(2, 3, 150, dtype=torch.bool, device=DEV)
    keep[1, 0, t0] = False
    for x, y in ((got.joints, base.joints), (got.shift, base.shift)):
        assert torch.equal(_bits(x)[keep], _bits(y)[keep])
    assert float(got.shift[1, 0, t0]) == 0.0 and int(got.joints.view(torch.int32)[1, 0, t0, 20, 1]) == 0x7FC12345
    assert float(base.shift[1, 0, t0]) != 0.0                                 # it would have moved
    for k in R.COUNTS + R.VALUES:                                              # the other clip and the other dancers: the same bits
        assert torch.equal(_bits(got.after[k])[0], _bits(base.after[k])[0]) and torch.equal(_bits(got.after[k])[1, 1:], _bits(base.after[k])[1, 1:]), k
    assert int(torch.isnan(got.joints).sum()) == 1


def test_ground_metrics_measures_what_ground_reports():
    for shape in ((1, 5, 70), (2, 3, 150), (1, 2, 1125)):
        pos, J, Cn = (_dev(a) for a in R.seeded(*shape))
        got = P.ground(pos, J, Cn, dn=shape[1])
        after = P.ground_metrics(got.joints, Cn, floor=got.floor)
        for k in P.METRICS:
            _same(after[k], got.after[k], (shape, k))
        assert int(got.after["penetration_frames"].sum()) < int(got.before["penetration_frames"].sum())
        T, dn = shape[2], shape[1]
        assert torch.equal(got.pos.view(shape[0], T, dn, 3).permute(0, 2, 1, 3), got.joints[:, :, :, 0])          # pos follows its root


# ---- with the foot lock, and through render_sample ---------------------------------------------------------------------------------------------
def test_ground_then_foot_lock_pins_the_feet_on_the_floor():
    """the order render_sample takes.  footlock_ref's motion (y up), every capsule 5 cm, each dancer's pos moved so that its lowest foot
    joint stands at 0.1 m in two runs of planted frames and the body is well above the floor between them; ground to the floor 0,
    then foot_lock: each pinned joint stands on the floor plus the foot's radius, within 1e-6 m"""
    T, DN, r = 40, FR.DN, 0.05
    q, pos = FR.motion(T, seed=31)
    tq, tpos = _dev(q), _dev(pos)
    off = torch.zeros(1, DN, T, 4, device=DEV)
    raw = F.foot_lock(tq, tpos, off, dn=DN).joints.cpu().numpy().astype(np.float64)          # every contact off: the FK of the poses
    runs = np.zeros(T, bool)
    runs[4:16] = runs[24:36] = True
    contacts = np.zeros((1, DN, T, 4), np.float32)
    lift = pos.reshape(1, T, DN, 3).astype(np.float64)
    pins = []
    for d in range(DN):
        y = raw[0, d, :, :, 1]
        feet = [7, 8, 10, 11]
        j = feet[int(np.argmin(y[runs][:, feet].mean(0)))]                     # the lowest foot joint of the runs: it is pinned
        assert (y[runs].argmin(1) == j).all(), "the pinned joint must be the lowest joint of the body in its runs"
        contacts[0, d, runs, {7: 0, 8: 1, 10: 2, 11: 3}[j]] = 1.0
        lift[0, :, d, 1] += np.where(runs, 0.1 - y[:, j], 0.45 - y.min(1))
        pins.append(j)
    moved = lift.astype(np.float32).reshape(1, T * DN, 3)
    tm, tc = _dev(moved), _dev(contacts)
    joints = F.foot_lock(tq, tm, off, dn=DN).joints
    g = P.ground(tm, joints, tc, dn=DN, up=1, floor=0.0, radii=np.full(24, r), return_shift=True)
    assert int(g.capped.sum()) == 0 and float(g.shift[:, :, 4:16].min()) < -0.049
    locked = F.foot_lock(tq, g.pos, tc, dn=DN)
    out = locked.joints.cpu().numpy()
    worst = 0.0
    for d, j in enumerate(pins):
        worst = max(worst, float(np.abs(out[0, d, runs, j, 1] - r).max()))
    print(f"[ground] ground then foot_lock: pinned joints {pins} within {worst:.3e} m of the floor plus the foot's radius (bound 1e-6)")
    assert worst <= 1e-6


def test_render_sample_grounds_the_motion_and_changes_only_the_vertical(tmp_path):
    import test_footlock_gpu as TF
    from tcdiff_amd import GaussianDiffusion
    DN = 2
    d = GaussianDiffusion.__new__(GaussianDiffusion)                      # render_sample of given samples asks nothing of the model
    torch.nn.Module.__init__(d)
    d.smpl = None
    x = torch.rand(2, 8 * DN, 151, generator=torch.Generator().manual_seed(5)) * 2 - 1
    x[:, ::3, :4] = 1.0                                                    # some rows declare every foot planted
    x = x.to(DEV)
    assert d.ground is False
    kw = dict(name=TF.NAMES, required_dancer_num=DN)
    d.render_sample(x, None, TF.NORM, 7, None, fk_out=str(tmp_path / "fk0"), **kw)
    parents, offsets = d._skeleton(torch.device(DEV))
    q, pos, poses, contacts = E.export_poses(x, TF.NORM, "normal", DN, parents=parents, offsets=offsets)
    g = P.ground(pos, poses, contacts, dn=DN, parents=parents)
    assert float(g.max_shift.max()) > 0
    try:
        d.ground = True
        d.render_sample(x, None, TF.NORM, 7, None, fk_out=str(tmp_path / "fk1"), **kw)
    finally:
        del d.ground                                                       # back to the class attribute
    moved = False
    for c, name in enumerate(E.fk_out_names("normal", 7, TF.NAMES)):
        with open(tmp_path / "fk0" / name, "rb") as f:
            off = pickle.load(f)
        with open(tmp_path / "fk1" / name, "rb") as f:
            on = pickle.load(f)
        assert np.array_equal(on["smpl_poses"], off["smpl_poses"])
        assert np.array_equal(on["smpl_trans"][..., :2].view(np.uint32), off["smpl_trans"][..., :2].view(np.uint32))          # x, y: their bits
        moved |= not np.array_equal(on["smpl_trans"][..., 2], off["smpl_trans"][..., 2])
        assert np.array_equal(on["smpl_trans"], g.pos[c].cpu().numpy()) and np.array_equal(on["full_pose"], g.joints[c].cpu().numpy())
    assert moved
    assert d.ground is False
    d.render_sample(x, None, TF.NORM, 7, None, fk_out=str(tmp_path / "fk2"), **kw)
    assert TF._files(tmp_path / "fk2") == TF._files(tmp_path / "fk0")
    assert os.listdir(tmp_path / "fk0")
