"""tcg_group_metrics (csrc/group.hip) and tcdiff_amd/group_metrics.py on an MI355X against the numpy float64 restatement
tests/group_ref.py.

The bound is rtol 1e-10 plus atol 1e-12 on every floating-point output with NaN at the same places, and equality on every integer
output and on the per-frame `closest` plane -- the bound tests/test_metrics_gpu.py holds its float64 kernels to.  It is derived, not
measured: kernel and restatement do the same float64 operations on the same float32 inputs up to the order of the sums (each of at
most ~1e3 terms of size O(1), an order error of at most N 2^-53 ~ 1e-13) and sqrt / division good to an ulp.  No case is excluded: the
restatement alone first shows (here again, and for every input in tests/test_group_cpu.py) that no decision is a near-tie."""
import importlib

import numpy as np
import pytest
import torch

import group_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd import metrics as M

G = importlib.import_module("tcdiff_amd.group_metrics")          # the package's attribute of this name is the function
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-10, 1e-12
FLOATS = ("body_contact_rate", "body_gap_min", "path_crossing_rate", "sync", "sync_zero", "gap")
INTS = ("body_contact_episodes", "body_closest", "path_crossings", "sync_lag", "closest")
ORDER = ["body_contact_rate", "body_gap_min", "body_contact_episodes", "body_closest", "path_crossings", "path_crossing_rate", "sync",
         "sync_lag", "sync_zero"]
_want = {}


def _reference(J, key, **kw):
    if key not in _want:
        ref = R.group_metrics(J, details=True, **kw)
        ok, why = R.judge(ref, kw.get("sigma_floor", 1e-6))
        assert ok, f"a decision of the reference is a near-tie on these inputs: {why}"
        _want[key] = ref
    return _want[key]


def _compare(got, want, what):
    assert list(got) == ORDER + ["gap", "closest"], (what, list(got))
    for k in FLOATS + INTS:
        g, w = got[k], want[k]
        assert g.is_cuda and tuple(g.shape) == w.shape, (what, k, tuple(g.shape), w.shape)
        g = g.cpu().numpy()
        if k in INTS:
            assert g.dtype == (np.int32 if k == "closest" else np.int64) and np.array_equal(g, w), (what, k, g, w)
            continue
        assert g.dtype == np.float64
        nan = np.isnan(w)
        err = np.abs(g - w)[~nan]
        print(f"{what} {k}: NaN {int(nan.sum())} of {w.size}, worst error {float(err.max()) if err.size else 0.0:.3e}")
        assert np.array_equal(np.isnan(g), nan), (what, k, g, w)
        assert bool((err <= ATOL + RTOL * np.abs(w[~nan])).all()), (what, k, g, w)


def _same_bits(a, b):
    assert list(a) == list(b)
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), k


def _bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x


def _dev(J):
    return torch.from_numpy(np.array(J, np.float32, order="C")).to(DEV)          # a copy: synth's arrays are read-only


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_float64_restatement(shape):
    """T = 1: no step; T = 2: one step, no lag; T = 3: the first correlation; 5 dancers x 70 frames: ten pairs, past one wave of
    frames; 150: several workgroups of four frames; 1125: past the pairs kernel's 256 threads, every window and every lag"""
    J = R.synth(*shape)
    _compare(G.group_metrics(_dev(J), return_frames=True), _reference(J, shape), shape)


def test_other_parameters():
    """up = 1, window = 0 and max_lag = 0; a window longer than the clip, all 129 lags and fps = 60; radii, a tree and a sigma_floor of
    the caller's with the window fps gives"""
    for n, (shape, kw) in enumerate(R.parameter_cases()):
        J = R.synth(*shape)
        _compare(G.group_metrics(_dev(J), return_frames=True, **kw), _reference(J, ("parameters", n), **kw), sorted(kw))


def test_exact_ties_take_the_stated_side():
    """inputs whose arithmetic is exact, so that the ties are ties on the device too: every bone pair of two upright sticks at a
    common height (the smallest code), equal frames (the first), the lags -1 and +1 (the negative one), all even lags (lag 0)"""
    xs = [1.0, 0.25, 0.25, 1.0, 0.25, 1.0, 0.25, 1.0]
    J = R.clip(R.stick_dancer(0.0, T=8), np.concatenate([R.stick_dancer(x) for x in xs]))
    for radii, code in ((np.full(24, 0.125), 25), (None, 75)):
        want = R.group_metrics(J, radii=radii)
        got = G.group_metrics(_dev(J), radii=radii, return_frames=True)
        assert (want["closest"] == code).all() and want["body_closest"][0, 0].tolist() == [1, code // 24, code % 24]
        for k in FLOATS + INTS:
            assert np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True), k
    beat = np.tile([1 / 64, 3 / 64], 20)
    for other, lag, zero in ((beat, 0, 1.0), (beat[::-1], -1, -1.0)):
        got = G.group_metrics(_dev(R.clip(R.stepper(beat), R.stepper(other) + np.float32(2.0))))
        assert got["sync"].item() == 1.0 and got["sync_lag"].item() == lag and got["sync_zero"].item() == zero


def test_the_frame_planes_land_where_they_are_told_and_nothing_else_is_written():
    shape = (2, 3, 5)
    b, dn, T = shape
    P, pad = 3, 37
    J = _dev(R.synth(*shape))
    public = G.group_metrics(J, return_frames=True)
    sizes = {"gap": (b, P, T), "closest": (b, P, T), "body_closest": (b, P, 3)}
    buf, view = {}, {}
    for k in ORDER + ["gap", "closest"]:
        shp = sizes.get(k, (b, P))
        n = int(np.prod(shp))
        dt = public[k].dtype
        buf[k] = torch.full((n + 2 * pad,), -77, dtype=dt, device=DEV)
        view[k] = buf[k][pad:pad + n].view(shp)
    nbytes = K.group_workspace(b, dn, T, 15)
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    K.group_metrics(J, 2, 30.0, [-1] + R.SMPL_PARENTS[1:], R.capsule_radii().tolist(), 30, 15, 1e-6, ws[:nbytes], view["gap"], view["closest"],
                    view["body_contact_rate"], view["body_gap_min"], view["body_contact_episodes"], view["body_closest"],
                    view["path_crossings"], view["path_crossing_rate"], view["sync"], view["sync_lag"], view["sync_zero"])
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all())
    for k in buf:
        assert bool((buf[k][:pad] == -77).all()) and bool((buf[k][-pad:] == -77).all()), k
    _same_bits({k: view[k] for k in public}, public)
    _same_bits({k: v for k, v in public.items() if k not in ("gap", "closest")}, G.group_metrics(J))          # the planes in the workspace


def test_strided_views_are_read_in_place_and_runs_repeat():
    """the frame-major layout tcdiff_pose_export writes, permuted as export_poses permutes it, without the copy"""
    shape = (2, 3, 150)
    J = _dev(R.synth(*shape))
    jv = J.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)          # (b, T, dn, 24, 3) storage
    assert not jv.is_contiguous() and torch.equal(jv, J)
    first = G.group_metrics(J, return_frames=True)
    _same_bits(G.group_metrics(jv, return_frames=True), first)
    _same_bits(G.group_metrics(J, return_frames=True), first)
    wide = torch.zeros(2, 3, 150, 30, 3, device=DEV)                            # a slice with larger outer strides
    wide[:, :, :, 3:27] = J
    _same_bits(G.group_metrics(wide[:, :, :, 3:27], return_frames=True), first)
    with pytest.raises(L.TcdiffError, match="contiguous"):
        G.group_metrics(J.transpose(-1, -2).contiguous().transpose(-1, -2))
    with pytest.raises(L.TcdiffError, match="max_lag"):
        G.group_metrics(J, max_lag=65)


def test_one_dancer_gives_empty_tensors():
    J = _dev(R.synth(2, 3, 5))[:, :1]
    got = G.group_metrics(J, return_frames=True)
    assert list(got) == ORDER + ["gap", "closest"]
    for k, v in got.items():
        want = (2, 0, 3) if k == "body_closest" else (2, 0, 5) if k in ("gap", "closest") else (2, 0)
        assert v.is_cuda and tuple(v.shape) == want, k
        assert v.dtype == (torch.int32 if k == "closest" else torch.int64 if k in INTS else torch.float64), k
    assert all(np.isnan(v) for v in M.summarize(got).values())


def test_a_nan_joint_poisons_its_own_pair_and_frame():
    shape = (2, 3, 5)
    clean = R.synth(*shape)
    J = clean.copy()
    J[1, 0, 2, 20] = np.nan                                             # clip 1, dancer 0, frame 2, the left wrist
    want = _reference(J, "nan joint")
    got = G.group_metrics(_dev(J), return_frames=True)
    _compare(got, want, "a NaN joint")
    base = G.group_metrics(_dev(clean), return_frames=True)
    gap, gap0 = got["gap"].cpu().numpy(), base["gap"].cpu().numpy()
    hit = np.zeros(gap.shape, bool)
    hit[1, :2, 2] = True                                                # the pairs (0, 1) and (0, 2) of clip 1, frame 2
    assert np.isnan(gap[hit]).all() and np.array_equal(gap[~hit], gap0[~hit])
    assert (got["closest"].cpu().numpy()[hit] == 24 * 20 + 1).all()     # the first bone pair that holds the joint
    for k in ORDER:                                                     # the other clip and the pair without the dancer: the same bits
        assert torch.equal(_bits(got[k])[0], _bits(base[k])[0]) and torch.equal(_bits(got[k])[1, 2], _bits(base[k])[1, 2]), k
    assert torch.equal(got["path_crossings"], base["path_crossings"]) and bool(torch.isfinite(got["body_gap_min"]).all())


def test_evaluate_group_is_export_then_group_metrics():
    g = torch.Generator().manual_seed(11)
    dn, S = 3, 20
    norm = tio.Normalizer(torch.randn(400, 151, generator=g))
    x = (torch.rand(2, S * dn, 151, generator=g) * 2 - 1).to(DEV)
    got = G.evaluate_group(x, norm, dn)
    _, _, poses, _ = E.export_poses(x, norm, "normal", dn)
    assert tuple(poses.shape) == (2, dn, S, 24, 3) and list(got) == ORDER and tuple(got["sync"].shape) == (2, 3)
    _same_bits(got, G.group_metrics(poses))
    pv = poses.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)
    _same_bits(G.group_metrics(pv), got)
    summary = M.summarize(got)
    assert list(summary) == ORDER and all(type(v) is float for v in summary.values())
    # long mode: 3 half-overlapping windows of 20 frames are one song of 40
    x3 = (torch.rand(3, S * dn, 151, generator=g) * 2 - 1).to(DEV)
    got = G.evaluate_group(x3, norm, dn, mode="long", window=5, max_lag=7)
    _, _, full, _ = E.export_poses(x3, norm, "long", dn)
    assert tuple(full.shape) == (1, dn, 40, 24, 3) and tuple(got["body_closest"].shape) == (1, 3, 3)
    _same_bits(got, G.group_metrics(full, window=5, max_lag=7))
    assert int(got["sync_lag"].abs().max()) <= 7
