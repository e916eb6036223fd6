"""CPU checks of the set-level metrics (no GPU): the numpy float64 restatement tests/set_metrics_ref.py against hand-checkable
motions, scipy's matrix square root and pdist; the seeded score inputs against the clamp's near-tie condition; SetStats' file
round trip; and the host side of tcdiff_amd.set_metrics (validation, no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.linalg import sqrtm
from scipy.spatial.distance import pdist

import set_metrics_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import set_metrics as S

FPS = 32                      # 1 / fps = 2^-5: the motions below are exact in float32 and their features exact in float64


def _joint_motion(T, fn):
    """every joint of one dancer at fn(t) plus its own rest position: (T, 24, 3) float32, exactly representable"""
    rest = (np.arange(72).reshape(24, 3) % 7 - 3) * 0.25
    J = np.stack([rest + np.asarray(fn(t), np.float64)[None, :] for t in range(T)])
    assert np.array_equal(J.astype(np.float32).astype(np.float64), J)
    return J.astype(np.float32)


@pytest.mark.parametrize("T", [3, 4, 5, 6, 40])
@pytest.mark.parametrize("window", [1, 2, 3])
def test_constant_velocity(T, window):
    v = np.array([0.5, -0.25, 1.0])                                    # metres per second
    f = R.kinetic_one(_joint_motion(T, lambda t: v * t / FPS), fps=FPS, up=2, window=window).reshape(24, 3)
    assert np.array_equal(f[:, 0], np.full(24, 0.5 ** 2 + 0.25 ** 2)) and np.array_equal(f[:, 1], np.full(24, 1.0))
    assert np.array_equal(f[:, 2], np.zeros(24))
    f = R.kinetic_one(_joint_motion(T, lambda t: v * t / FPS), fps=FPS, up=1, window=window).reshape(24, 3)
    assert np.array_equal(f[:, 0], np.full(24, 0.5 ** 2 + 1.0)) and np.array_equal(f[:, 1], np.full(24, 0.25 ** 2))


@pytest.mark.parametrize("T", [3, 4, 5, 6, 40])
@pytest.mark.parametrize("window", [1, 2])
def test_constant_acceleration(T, window):
    a = np.array([2.0, -4.0, 4.0])                                     # |a| = 6
    f = R.kinetic_one(_joint_motion(T, lambda t: 0.5 * a * (t / FPS) ** 2), fps=FPS, window=window).reshape(24, 3)
    assert np.array_equal(f[:, 2], np.full(24, 6.0))
    assert (f[:, :2] > 0).all()


def test_a_still_body_and_short_clips():
    assert np.array_equal(R.kinetic_one(_joint_motion(9, lambda t: np.zeros(3))), np.zeros(72))
    for T in (1, 2):
        assert np.isnan(R.kinetic_one(_joint_motion(T, lambda t: np.ones(3) * t))).all()
    assert not np.isnan(R.kinetic_one(_joint_motion(3, lambda t: np.ones(3) * t))).any()


def test_windows_clip_at_both_ends():
    """T = 4, w = 2, one joint moving along x by steps 1, 2, 4 (d[1..3]) at fps 1: v_1 = v_2 = v_3 = 7 / 3 (every window is the
    whole clip); accelerations d[s+1] - d[s] = 1, 2 for s = 1, 2, every a_i their mean 1.5"""
    x = [0.0, 1.0, 3.0, 7.0]
    f = R.kinetic_one(_joint_motion(4, lambda t: [x[t], 0.0, 0.0]), fps=1, window=2).reshape(24, 3)
    assert f[0, 0] == pytest.approx((7 / 3) ** 2, rel=1e-15) and f[0, 1] == 0.0 and f[0, 2] == 1.5
    # w = 1: v_1 = (1 + 2) / 2, v_2 = 7 / 3, v_3 = (2 + 4) / 2; a_1 = (1 + 2) / 2 (s = 1, 2), a_2 = 1.5, a_3 = 2 (s = 2 only)
    f = R.kinetic_one(_joint_motion(4, lambda t: [x[t], 0.0, 0.0]), fps=1, window=1).reshape(24, 3)
    assert f[0, 0] == pytest.approx((1.5 ** 2 + (7 / 3) ** 2 + 3.0 ** 2) / 3, rel=1e-15) and f[0, 2] == pytest.approx(5.0 / 3, rel=1e-15)


def test_fid_is_scipys_on_a_full_rank_pair():
    ref_x, gen_x = R.score_case((72, 200, 150))
    ref = R.fit_reference(ref_x)
    got = R.set_scores(gen_x, ref)
    S1, S2 = ref["cov_z"], got["cov"]
    root = sqrtm(S1 @ S2)
    want = float(((got["mu"] - ref["mu_z"]) ** 2).sum() + np.trace(S1) + np.trace(S2) - 2.0 * np.trace(root).real)
    print(f"fid {got['fid']:.12f}, with scipy.linalg.sqrtm {want:.12f}: relative difference {abs(got['fid'] - want) / want:.2e}")
    assert got["fid"] > 1.0 and abs(got["fid"] - want) <= 1e-9 * want


@pytest.mark.parametrize("shape", R.SCORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_set_against_itself_is_at_distance_zero(shape):
    ref_x, _ = R.score_case(shape)
    ref = R.fit_reference(ref_x)
    got = R.set_scores(ref_x, ref)
    assert np.array_equal(got["mu"], ref["mu_z"]) and np.array_equal(got["cov"], ref["cov_z"])
    print(f"{shape}: fid(x, x) = {got['fid']:.3e} of scale {got['scale']:.3e}")
    assert abs(got["fid"]) <= 1e-10 * got["scale"]


@pytest.mark.parametrize("shape", R.SCORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seeded_score_inputs_keep_clear_of_the_clamp(shape):
    ref_x, gen_x = R.score_case(shape)
    ref = R.fit_reference(ref_x)
    for what, x in (("scored", gen_x), ("itself", ref_x)):
        got = R.set_scores(x, ref)
        ok, closest = R.clamp_clear(got["eigs"])
        print(f"{shape} {what}: the closest eigenvalue is a factor {closest:.3g} from its threshold")
        assert ok, (shape, what, closest)
    D, n_ref, m = shape
    w, lam = R.set_scores(gen_x, ref)["eigs"]
    assert int((R.clamped_roots(w) > 0).sum()) == min(D, n_ref - 1)                     # the ranks the clamp is there to find
    assert int((R.clamped_roots(lam) > 0).sum()) == min(D, n_ref - 1, m - 1)


def test_the_clamp_condition_sees_a_near_tie():
    eig = np.array([1.0, 2.0 * 3 * 2.0 ** -52, 0.0])                                     # threshold 3 * 2^-52
    assert R.clamp_clear([eig]) == (False, 2.0)
    assert R.clamp_clear([np.array([1.0, 0.4 * 3 * 2.0 ** -52, -1e-18])])[0] is False
    assert R.clamp_clear([np.array([1.0, 1e-3, 1e-18, -1e-17])])[0]
    assert R.clamp_clear([np.zeros(4)]) == (True, np.inf)


@pytest.mark.parametrize("shape", [(9, 12), (30, 72), (3, 1)])
def test_div_is_scipys_mean_pairwise_distance(shape):
    Z = R.synth_feats(shape[0], shape[1], 3)
    assert R.diversity(Z) == pytest.approx(pdist(Z).mean(), rel=1e-13)


@pytest.mark.parametrize("shape", R.STATS_SHAPES)
def test_statistics_are_numpys(shape):
    X = R.stats_case(shape)
    st = R.fit_reference(X)
    n, D = shape
    assert st["n"] == n
    np.testing.assert_allclose(st["mean"], X.mean(0), rtol=1e-13)
    np.testing.assert_allclose(st["std"], X.std(0), rtol=1e-12, atol=0)
    Z = (X - X.mean(0)) / (X.std(0) + 1e-10)
    np.testing.assert_allclose(st["cov_z"], np.cov(Z, rowvar=False).reshape(D, D), rtol=1e-9, atol=1e-14)
    assert np.array_equal(st["cov_z"], st["cov_z"].T)
    if D > 1:                                                                              # the constant column
        c = D // 2
        assert st["std"][c] == 0.0 and st["mu_z"][c] == 0.0 and not st["cov_z"][c].any() and not st["cov_z"][:, c].any()


def test_set_stats_round_trip(tmp_path):
    st = R.fit_reference(R.stats_case((40, 12)))
    s = S.SetStats(st["n"], *(torch.from_numpy(st[k]) for k in ("mean", "std", "mu_z", "cov_z")))
    assert s.dim == 12
    path = tmp_path / "ref.npz"
    s.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ["cov_z", "mean", "mu_z", "n", "std"] and int(f["n"]) == 40
    back = S.SetStats.load(path, "cpu")
    assert back.n == 40
    for k in ("mean", "std", "mu_z", "cov_z"):
        a, b = getattr(s, k), getattr(back, k)
        assert b.dtype == torch.float64 and a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64)), k
    with pytest.raises(L.TcdiffError):
        S.SetStats(3, torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64),
                   torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(L.TcdiffError):
        S.SetStats(3, *(torch.zeros(4),) * 3, torch.zeros(4, 4))                          # float32


def test_no_cpu_fallback_and_input_checks():
    with pytest.raises(L.TcdiffError, match="MI355X"):
        S.kinetic_features(torch.zeros(1, 2, 5, 24, 3))
    with pytest.raises(L.TcdiffError, match="joints must be"):
        S.kinetic_features(torch.zeros(1, 2, 5, 72))
    with pytest.raises(L.TcdiffError, match="float32"):
        S.kinetic_features(torch.zeros(1, 2, 5, 24, 3, dtype=torch.float64))
    with pytest.raises(L.TcdiffError, match="contiguous"):
        S.kinetic_features(torch.zeros(1, 2, 5, 3, 24).transpose(-1, -2))
    with pytest.raises(L.TcdiffError, match="MI355X"):
        S.reference_from_joints(torch.zeros(2, 2, 5, 24, 3))
    x = torch.zeros(4, 6, dtype=torch.float64)
    with pytest.raises(L.TcdiffError, match="MI355X"):
        S.fit_reference(x)
    with pytest.raises(L.TcdiffError, match="at least 2 rows"):
        S.fit_reference(x[:1])
    with pytest.raises(L.TcdiffError, match="float64"):
        S.fit_reference(x.float())
    with pytest.raises(L.TcdiffError, match="columns"):
        S.fit_reference(torch.zeros(4, L.SET_MAX_D + 1, dtype=torch.float64))
    with pytest.raises(L.TcdiffError, match=r"\(N, D\)"):
        S.fit_reference(torch.zeros(4, dtype=torch.float64))
    ref = S.SetStats(4, *(torch.zeros(6, dtype=torch.float64),) * 3, torch.zeros(6, 6, dtype=torch.float64))
    with pytest.raises(L.TcdiffError, match="MI355X"):
        S.set_scores(x, ref)
    with pytest.raises(L.TcdiffError, match="columns"):
        S.set_scores(x[:, :5], ref)
    with pytest.raises(L.TcdiffError, match="SetStats"):
        S.set_scores(x, {"mean": 0})
    with pytest.raises(L.TcdiffError):
        S.evaluate_set(torch.zeros(1, 6, 151), None, 2, ref)


def test_launchers_validate_their_arguments_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    lib = L.load()
    for sym in ("tcdiff_kinetic_features", "tcdiff_set_stats", "tcdiff_set_scores", "tcdiff_set_check"):
        assert sym in L.EXPORTS
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    s3 = (C.c_long * 3)(0, 0, 0)

    def kin(joints=p, js=s3, b=1, dn=1, T=3, up=2, w=2, fps=30.0, out=p):
        return lib.tcdiff_kinetic_features(joints, js, b, dn, T, up, w, fps, out, None)
    assert kin(joints=None) == -1 and kin(js=None) == -1 and kin(out=None) == -1
    assert kin(b=0) == -1 and kin(dn=0) == -1 and kin(T=0) == -1 and kin(up=3) == -1 and kin(up=-1) == -1
    assert kin(w=0) == -1 and kin(fps=0.0) == -1 and kin(fps=float("nan")) == -1

    def stats(feats=p, N=2, D=1, mean=p, z=p, cov=p, rows=None):
        return lib.tcdiff_set_stats(feats, N, D, 1, mean, p, z, p, p, cov, rows, None)
    assert stats(feats=None) == -1 and stats(mean=None) == -1 and stats(z=None) == -1 and stats(cov=None) == -1
    assert stats(N=1) == -1 and stats(D=0) == -1 and stats(D=L.SET_MAX_D + 1) == -4

    def scores(mu=p, M=2, D=1, sweeps=30, fid=p, status=p):
        return lib.tcdiff_set_scores(mu, p, p, p, p, M, D, sweeps, fid, p, status, None)
    assert scores(mu=None) == -1 and scores(fid=None) == -1 and scores(status=None) == -1
    assert scores(M=1) == -1 and scores(D=0) == -1 and scores(sweeps=0) == -1 and scores(sweeps=L.SET_MAX_SWEEPS + 1) == -1
    assert scores(D=L.SET_MAX_D + 1) == -4
    assert lib.tcdiff_set_check(None, None) == -1
    assert (L.SET_MAX_D, L.SET_MAX_SWEEPS) == (72, 30)
    with pytest.raises(L.TcdiffError, match="did not converge"):
        L.check(-5, "tcdiff_set_check")


def test_the_package_exports_the_set_metrics():
    import tcdiff_amd
    for name in ("SetStats", "kinetic_features", "fit_reference", "set_scores", "evaluate_set", "reference_from_joints"):
        assert getattr(tcdiff_amd, name) is getattr(S, name) and name in tcdiff_amd.__all__
