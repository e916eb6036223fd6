"""csrc/set_metrics.hip and tcdiff_amd/set_metrics.py on an MI355X against the numpy float64 restatement tests/set_metrics_ref.py.

Bounds.  Kinetic features, statistics and ``div``: rtol 1e-10 per element with NaN at the same places -- kernel and restatement
do the same float64 operations on the same inputs up to the order of sums of at most ~1e4 terms (an order error of at most
N 2^-53 relative to the sum of the terms' magnitudes) and sqrt good to an ulp.  One statistic is a sum that cancels: ``mu_z`` of
``fit_reference`` is the mean of rows just normalised to mean zero, so its value IS the order error; there the same argument
bounds the difference by 1e-10 times the mean magnitude of the column's terms, and that is what is asserted for it.
``fid``: |got - want| <= 1e-10 (|mu - mu_ref|^2 + tr S1 + tr S2), against eigenvalues from numpy.linalg.eigh / eigvalsh; before
any comparison the restatement alone shows that no eigenvalue of either decomposition is within a factor 3 of the clamp's
threshold.  No case is left out.  The worst observed figure of every case is printed."""
import numpy as np
import pytest
import torch

import set_metrics_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import metrics as M
from tcdiff_amd import set_metrics as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-10
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _close(got, want, what, scale=None):
    """per element |got - want| <= RTOL |want| (or RTOL scale where one is given), NaN in the same places"""
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    g = got.cpu().numpy()
    nan = np.isnan(want)
    ref = np.abs(want) if scale is None else np.broadcast_to(scale, want.shape)
    err, ref = np.abs(g - want)[~nan], ref[~nan]
    nz = ref != 0
    rel = float((err[nz] / ref[nz]).max()) if nz.any() else 0.0
    print(f"{what}: NaN {int(nan.sum())} of {want.size}, worst relative error {rel:.3e}")
    assert np.array_equal(np.isnan(g), nan), (what, g, want)
    assert bool((err <= RTOL * ref).all()), (what, rel)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- kinetic features --------------------------------------------------------------------------------------------------------
def _features_want(shape, **kw):
    return _once(("kin", shape, tuple(sorted(kw.items()))), lambda: R.kinetic_features(R.synth_joints(*shape), **kw))


@pytest.mark.parametrize("shape", R.FEATURE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kinetic_features_against_the_restatement(shape):
    """T = 1, 2: NaN; T = 3 .. 5: both window ends clip in every frame; T = 6: the first full window; T = 600: a thread adds three
    frames before the tree"""
    got = S.kinetic_features(_dev(R.synth_joints(*shape)))
    want = _features_want(shape)
    assert np.isnan(want).all() == (shape[2] < 3) and np.isnan(want).any() == (shape[2] < 3)
    _close(got, want, f"kinetic features {shape}")


@pytest.mark.parametrize("kw", [dict(up=1), dict(window=1), dict(fps=60, up=0, window=3), dict(window=1000)], ids=str)
def test_kinetic_features_other_parameters(kw):
    """window = 1000: every window is the whole clip (the restatement's loops make that one slow on long clips: short ones only)"""
    for shape in ((2, 3, 4), (1, 2, 6), (2, 3, 150))[:2 if kw.get("window", 0) > 100 else 3]:
        _close(S.kinetic_features(_dev(R.synth_joints(*shape)), **kw), _features_want(shape, **kw), f"kinetic features {shape} {kw}")


def test_kinetic_features_read_strided_views_in_place_and_repeat():
    """the frame-major layout tcdiff_pose_export writes, through the permuted view, without a copy"""
    shape = (2, 3, 150)
    joints = _dev(R.synth_joints(*shape))
    first = S.kinetic_features(joints)
    _close(first, _features_want(shape), "contiguous")
    jv = joints.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)              # (b, T, dn, 24, 3) storage
    assert not jv.is_contiguous() and torch.equal(jv, joints)
    _same_bits(S.kinetic_features(jv), first)
    _same_bits(S.kinetic_features(joints), first)
    wide = torch.zeros(2, 3, 150, 30, 3, device=DEV)                                     # a slice with larger outer strides
    wide[:, :, :, 3:27] = joints
    _same_bits(S.kinetic_features(wide[:, :, :, 3:27]), first)
    with pytest.raises(L.TcdiffError, match="contiguous"):
        S.kinetic_features(joints.transpose(-1, -2).contiguous().transpose(-1, -2))
    for bad in (dict(up=3), dict(window=0), dict(window=1.5), dict(fps=0)):
        with pytest.raises(L.TcdiffError):
            S.kinetic_features(joints, **bad)


# ---- statistics --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.STATS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fit_reference_against_the_restatement(shape):
    """N = 2 and D = 1: the smallest set; N = 3 < D = 5; N = 257: a thread adds two rows before the tree, D = 72: nine column tiles
    of the covariance; D = 12: a tile that ends inside the matrix.  One column of every D > 1 is constant: std 0 exactly, a zero
    row and column of the covariance."""
    X = R.stats_case(shape)
    want = _once(("fit", shape), lambda: R.fit_reference(X))
    got = S.fit_reference(_dev(X))
    assert got.n == shape[0] and got.dim == shape[1]
    _close(got.mean, want["mean"], f"{shape} mean")
    _close(got.std, want["std"], f"{shape} std")
    z = R.normalise(X, want["mean"], want["std"])
    _close(got.mu_z, want["mu_z"], f"{shape} mu_z (relative to the mean magnitude of its terms)", scale=np.abs(z).mean(0))
    _close(got.cov_z, want["cov_z"], f"{shape} cov_z")
    assert torch.equal(got.cov_z, got.cov_z.T)
    if shape[1] > 1:
        c = shape[1] // 2
        assert float(got.std[c]) == 0.0 and not bool(got.cov_z[c].any()) and not bool(got.cov_z[:, c].any())
    again = S.fit_reference(_dev(X))
    for k in ("mean", "std", "mu_z", "cov_z"):
        _same_bits(getattr(got, k), getattr(again, k))


# ---- scores --------------------------------------------------------------------------------------------------------------------
def _score_case(shape):
    def make():
        ref_x, gen_x = R.score_case(shape)
        ref = R.fit_reference(ref_x)
        want = {"scored": R.set_scores(gen_x, ref), "itself": R.set_scores(ref_x, ref)}
        for what, w in want.items():
            ok, closest = R.clamp_clear(w["eigs"])
            assert ok, f"{shape} {what}: an eigenvalue of the restatement is a factor {closest:.3g} from the clamp's threshold"
        return ref_x, gen_x, ref, want
    return _once(("score", shape), make)


def _check_scores(got, want, what):
    assert list(got) == ["fid", "div"]
    for v in got.values():
        assert v.is_cuda and v.dtype == torch.float64 and v.dim() == 0
    _close(got["div"], np.asarray(want["div"]), f"{what} div")
    fid = float(got["fid"])
    err = abs(fid - want["fid"])
    print(f"{what} fid: {fid:.12g}, restatement {want['fid']:.12g}, |difference| / (|dmu|^2 + tr S1 + tr S2) = {err / want['scale']:.3e}")
    assert err <= RTOL * want["scale"], (what, fid, want["fid"])


@pytest.mark.parametrize("shape", R.SCORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_set_scores_against_the_restatement(shape):
    """D = 72 full rank; N_ref, M < D: rank-deficient on both sides, where the clamp decides; D = 5 odd and D = 1: the round-robin's
    padding player and no pair at all; each also as a set against itself, where fid is 0 within the bound"""
    ref_x, gen_x, ref_want, want = _score_case(shape)
    ref = S.fit_reference(_dev(ref_x))
    got = S.set_scores(_dev(gen_x), ref, check=True)
    _check_scores(got, want["scored"], f"{shape}")
    itself = S.set_scores(_dev(ref_x), ref, check=True)
    _check_scores(itself, want["itself"], f"{shape} against itself")
    assert abs(float(itself["fid"])) <= RTOL * want["itself"]["scale"]
    again = S.set_scores(_dev(gen_x), ref)
    for k in got:
        _same_bits(got[k], again[k])


def test_a_loaded_reference_scores_the_same(tmp_path):
    ref_x, gen_x, _, want = _score_case((12, 40, 9))
    ref = S.fit_reference(_dev(ref_x))
    ref.save(tmp_path / "ref.npz")
    back = S.SetStats.load(tmp_path / "ref.npz", DEV)
    a, b = S.set_scores(_dev(gen_x), ref), S.set_scores(_dev(gen_x), back)
    for k in a:
        _same_bits(a[k], b[k])
    with pytest.raises(L.TcdiffError, match="columns"):
        S.set_scores(_dev(gen_x)[:, :11], ref)
    with pytest.raises(L.TcdiffError, match="at least 2 rows"):
        S.set_scores(_dev(gen_x)[:1], ref)


def test_the_sweep_cap_is_never_silent():
    """one sweep cannot finish a 12 x 12 decomposition: fid is NaN, and with check=True the call raises"""
    ref_x, gen_x, _, _ = _score_case((12, 40, 9))
    ref = S.fit_reference(_dev(ref_x))
    got = S.set_scores(_dev(gen_x), ref, _max_sweeps=1)
    assert bool(torch.isnan(got["fid"])) and not bool(torch.isnan(got["div"]))
    with pytest.raises(L.TcdiffError, match="did not converge"):
        S.set_scores(_dev(gen_x), ref, check=True, _max_sweeps=1)


def test_evaluate_set_is_export_features_scores():
    g = torch.Generator().manual_seed(11)
    dn, T = 3, 20
    norm = tio.Normalizer(torch.randn(400, 151, generator=g))
    real = _dev(R.synth_joints(4, dn, T))
    ref = S.reference_from_joints(real, window=1)
    feats = S.kinetic_features(real, window=1)
    assert tuple(feats.shape) == (4, dn, 72)
    by_hand = S.fit_reference(feats.reshape(4 * dn, 72))
    assert ref.n == 12
    for k in ("mean", "std", "mu_z", "cov_z"):
        _same_bits(getattr(ref, k), getattr(by_hand, k))
    x = (torch.rand(2, T * dn, 151, generator=g) * 2 - 1).to(DEV)
    got = S.evaluate_set(x, norm, dn, ref, window=1, check=True)
    _, _, poses, _ = E.export_poses(x, norm, "normal", dn)
    want = S.set_scores(S.kinetic_features(poses, window=1).reshape(2 * dn, 72), ref)
    assert list(got) == ["fid", "div"]
    for k in got:
        _same_bits(got[k], want[k])
    s = M.summarize(got)
    assert all(type(v) is float and np.isfinite(v) for v in s.values()) and s["fid"] == float(got["fid"]) and s["div"] > 0
    # long mode: 3 half-overlapping windows of 20 frames are one song of 40 frames, a set of dn rows
    x3 = (torch.rand(3, T * dn, 151, generator=g) * 2 - 1).to(DEV)
    got = S.evaluate_set(x3, norm, dn, ref, mode="long", window=1)
    _, _, full, _ = E.export_poses(x3, norm, "long", dn)
    assert tuple(full.shape) == (1, dn, 40, 24, 3)
    want = S.set_scores(S.kinetic_features(full, window=1).reshape(dn, 72), ref)
    for k in got:
        _same_bits(got[k], want[k])
