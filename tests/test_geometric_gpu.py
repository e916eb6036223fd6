"""csrc/geometric.hip and tcdiff_amd/set_metrics.py's geometric features on an MI355X against the numpy float64 restatement
tests/geometric_ref.py.

The bar is equal bits, no tolerance.  A feature is an integer count divided by T - 1, so kernel and restatement differ only where
they decide a predicate differently, and they evaluate the same float64 expressions (acos excepted, good to an ulp or two) -- a
decision can differ only at a near-tie.  Before every comparison the restatement alone shows that no decision of that input is
within a relative 1e-9 of its threshold (tests/test_geometric_cpu.py shows it for the seeded cases; the inputs made here assert
it themselves), seven orders of magnitude above what rounding can move."""
import numpy as np
import pytest
import torch

import geometric_ref as G
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd import set_metrics as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GPU_CASES = [c for c in G.CASES if c != ("A", (1, 2, 257))]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a writable copy: the shared cases are read-only)


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _equal(got, want, what):
    """got on the device == want of the restatement, NaN in the same places"""
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    g = got.cpu().numpy()
    print(f"{what}: {int((g != want).sum() - np.isnan(want).sum())} of {want.size} differ")
    assert np.array_equal(g, want, equal_nan=True), (what, np.argwhere(~((g == want) | (np.isnan(g) & np.isnan(want)))))


def _want(J, up, tau, table=None, rng=None):
    feats, _, margin = G.geometric_features(J, up, tau, table, rng)
    assert margin >= G.MIN_MARGIN, margin
    return feats


@pytest.mark.parametrize("case", GPU_CASES, ids=G.case_id)
def test_geometric_features_against_the_restatement(case):
    """T = 1: NaN; T = 2 .. 5: a chunk of a few lanes; T = 64, 65, 66: one chunk less a frame, exactly one, one and a frame; T = 129:
    two chunks and a frame; T = 600: ten; family B: rows 8 and the FAST rows take both values"""
    J, tau, (want, _, margin) = G.case(*case)
    assert margin >= G.MIN_MARGIN
    got = S.geometric_features(_dev(J), time_per_frame=tau)
    assert np.isnan(want).all() == (case[1][2] < 2) and np.isnan(want).any() == (case[1][2] < 2)
    _equal(got, want, G.case_id(case))
    if case[0] == "A":                                                   # 1 / 120 is the default
        _same_bits(S.geometric_features(_dev(J)), got)


def test_strided_views_are_read_in_place_and_runs_repeat():
    """the frame-major layout tcdiff_pose_export writes, through the permuted view, without a copy"""
    J, tau, (want, _, _) = G.case("A", (2, 3, 150))
    joints = _dev(J)
    first = S.geometric_features(joints)
    _equal(first, want, "contiguous")
    jv = joints.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)              # (b, T, dn, 24, 3) storage
    assert not jv.is_contiguous() and torch.equal(jv, joints)
    _same_bits(S.geometric_features(jv), first)
    _same_bits(S.geometric_features(joints), first)
    wide = torch.zeros(2, 3, 150, 30, 3, device=DEV)                                     # a slice with larger outer strides
    wide[:, :, :, 3:27] = joints
    _same_bits(S.geometric_features(wide[:, :, :, 3:27]), first)
    with pytest.raises(L.TcdiffError, match="contiguous"):
        S.geometric_features(joints.transpose(-1, -2).contiguous().transpose(-1, -2))
    t, r = S.geometric_table()
    t[4, 0] = 7
    with pytest.raises(L.TcdiffError, match="kind"):
        S.geometric_features(joints, table=(t, r))


def test_the_up_axis_moved_to_one_gives_the_same_bits():
    """the same motion turned so that its up axis is y (a rotation: the components moved cyclically), with up=1"""
    for case in (("A", (2, 3, 150)), ("B", (1, 2, 65))):
        J, tau, (want, _, _) = G.case(*case)
        turned = np.ascontiguousarray(J[..., [1, 2, 0]])
        assert np.array_equal(_want(turned, 1, tau), want)               # the restatement itself: no decision changes
        _equal(S.geometric_features(_dev(turned), up=1, time_per_frame=tau), want, f"{G.case_id(case)} with up = 1")
        turned = np.ascontiguousarray(J[..., [2, 0, 1]])
        assert np.array_equal(_want(turned, 0, tau), want)
        _equal(S.geometric_features(_dev(turned), up=0, time_per_frame=tau), want, f"{G.case_id(case)} with up = 0")


def test_custom_tables():
    """R = 1 of each kind; R = 72: the default table repeated and cut; a row's own thresholds"""
    J, tau, (want, _, _) = G.case("B", (2, 3, 40))
    joints = _dev(J)
    table, rng = G.default_table()
    for kind in range(6):
        r = int(np.argmax(table[:, 0] == kind))
        got = S.geometric_features(joints, time_per_frame=tau, table=(table[r:r + 1], rng[r:r + 1]))
        _equal(got, want[:, :, r:r + 1], f"R = 1, {G.KINDS[kind]} (row {r})")
    t72, r72 = np.concatenate([table] * 3)[:72], np.concatenate([rng] * 3)[:72]
    got = S.geometric_features(joints, time_per_frame=tau, table=(_dev(t72), _dev(r72)))          # device tensors are taken too
    _equal(got, np.concatenate([want] * 3, axis=2)[:, :, :72], "R = 72")
    r2 = rng.copy()
    r2[:, 0] *= 0.5                                                      # other thresholds (angles: lo halves, hi stays)
    _equal(S.geometric_features(joints, time_per_frame=tau, table=(table, r2)), _want(J, 2, tau, table, r2), "halved thresholds")
    _equal(S.geometric_features(joints, time_per_frame=tau, lengths={"hl": 0.5 * G.HL, "sw": 0.5 * G.SW, "hw": 0.5 * G.HW}),
           _want(J, 2, tau, table, np.where(table[:, :1] == G.ANGLE, rng, 0.5 * rng)), "halved lengths")
    _equal(S.geometric_features(joints, time_per_frame=tau), want, "the default table again")


def test_a_table_corrupted_on_the_device_counts_nothing_in_its_rows():
    """what the Python wrapper refuses, the kernel must still survive: kind 9, point 40 and point -1 written into the device copy"""
    J, tau, (want, _, _) = G.case("A", (2, 3, 150))
    joints = _dev(J)
    table, rng = G.default_table()
    t_dev, r_dev = _dev(table), _dev(rng)
    t_dev[3, 0], t_dev[7, 2], t_dev[12, 1] = 9, 40, -1                   # (row 12 is FAST, which does not read a: refused all the same)
    feats = torch.empty(2, 3, 32, dtype=torch.float64, device=DEV)
    K.geometric_features(joints, 2, t_dev, r_dev, tau, feats)
    expect = want.copy()
    expect[:, :, [3, 7, 12]] = 0.0
    assert (want[:, :, [3, 7, 12]] > 0).any((0, 1)).all()                # the three rows did count before
    _equal(feats, expect, "corrupted rows 3, 7 and 12")
    bad = table.copy()
    bad[3, 0], bad[7, 2], bad[12, 1] = 9, 40, -1
    assert np.array_equal(G.geometric_features(J, 2, tau, bad, rng)[0], expect)


def test_a_nan_joint_touches_only_the_rows_and_frames_that_read_it():
    J, tau, (want, counts, _) = G.case("A", (1, 2, 65))
    Jn = J.copy()
    Jn[0, 1, 30, G.LWRIST, 0] = np.nan                                   # a horizontal component: the floor does not see it
    feats, cn, margin = G.geometric_features(Jn, 2, tau)
    assert margin >= G.MIN_MARGIN
    table, _ = G.default_table()
    reads = np.array([G.LWRIST in ((a, b, p) if k == G.MOVE else (p,) if k == G.FAST else (a, b, c, p)) for k, a, b, c, p in table.tolist()])
    lost = counts - cn                                                   # per row 0, 1 or 2 frames: frame 30 and, for the velocities, 31
    assert not lost[0, 0].any() and not lost[0, 1][~reads].any() and lost[0, 1][reads].any()
    assert lost.min() >= 0 and lost.max() <= 2 and set(np.nonzero(lost[0, 1] == 2)[0]) <= {1, 9, 10, 11, 13}
    _equal(S.geometric_features(_dev(Jn)), feats, "a NaN in lwrist x at frame 30")
    Jn = J.copy()
    Jn[0, 0, 64, G.HEAD, 2] = np.nan                                     # the last frame's `up` component: its floor is NaN
    feats, cn, margin = G.geometric_features(Jn, 2, tau)
    lost = counts - cn                                                   # the rows that read the floor, one frame each
    assert margin >= G.MIN_MARGIN and not lost[0, 1].any() and lost[0, 0].any() and lost.min() >= 0 and lost.max() <= 1
    assert set(np.nonzero(lost[0, 0])[0]) <= {16, 17, 29, 30}
    _equal(S.geometric_features(_dev(Jn)), feats, "a NaN in head z at the last frame")


def test_nothing_outside_feats_is_written():
    J, tau, (want, _, _) = G.case("A", (2, 3, 150))
    joints = _dev(J)
    table, rng = G.default_table()
    for R in (32, 5):
        buf = torch.full((64 + 6 * R + 64,), -7.25, dtype=torch.float64, device=DEV)
        feats = buf[64:64 + 6 * R].view(2, 3, R)
        K.geometric_features(joints, 2, _dev(table[:R]), _dev(rng[:R]), tau, feats)
        _equal(feats, want[:, :, :R], f"R = {R} inside sentinels")
        assert bool((buf[:64] == -7.25).all()) and bool((buf[64 + 6 * R:] == -7.25).all())
    J1 = G.case("A", (1, 1, 1))[0]                                       # T = 1: R NaNs and nothing else
    buf = torch.full((64 + 32 + 64,), -7.25, dtype=torch.float64, device=DEV)
    K.geometric_features(_dev(J1), 2, _dev(table), _dev(rng), tau, buf[64:96].view(1, 1, 32))
    assert bool(torch.isnan(buf[64:96]).all()) and bool((buf[:64] == -7.25).all()) and bool((buf[96:] == -7.25).all())


# ---- the set-level chain -------------------------------------------------------------------------------------------------------
FID_ITSELF_RTOL = 1e-10          # test_set_metrics_gpu.py's bound for fid_k of a set against itself: RTOL (|dmu|^2 + tr S1 + tr S2)


def test_reference_from_joints_and_set_scores_are_the_hand_made_chain():
    J = G.case_joints("B", (8, 3, 40))
    real = _dev(J)
    tau = G.TAU["B"]
    ref = S.reference_from_joints(real, features="geometric", time_per_frame=tau)
    feats = S.geometric_features(real, time_per_frame=tau)
    assert tuple(feats.shape) == (8, 3, 32) and ref.n == 24 and ref.dim == 32
    by_hand = S.fit_reference(feats.reshape(24, 32))
    for k in ("mean", "std", "mu_z", "cov_z"):
        _same_bits(getattr(ref, k), getattr(by_hand, k))
    gen = _dev(G.case_joints("B", (2, 3, 40)))
    rows = S.geometric_features(gen, time_per_frame=tau).reshape(6, 32)
    a, b = S.set_scores(rows, ref, check=True), S.set_scores(rows, by_hand)
    for k in a:
        _same_bits(a[k], b[k])
    assert float(a["fid"]) > 0 and float(a["div"]) > 0
    # fid_g of a set against its own reference: zero within the bound test_set_metrics_gpu.py holds fid_k of a set against itself to
    itself = S.set_scores(feats.reshape(24, 32), ref, check=True)
    scale = float(torch.trace(ref.cov_z)) * 2
    print(f"fid_g of the set against itself: {float(itself['fid']):.3e}, scale {scale:.3e}")
    assert abs(float(itself["fid"])) <= FID_ITSELF_RTOL * scale


def test_evaluate_set_all_is_the_two_single_calls():
    g = torch.Generator().manual_seed(11)
    dn, T = 3, 20
    norm = tio.Normalizer(torch.randn(400, 151, generator=g))
    real = _dev(G.case_joints("A", (4, dn, T)))
    refs = {"kinetic": S.reference_from_joints(real, window=1), "geometric": S.reference_from_joints(real, "geometric")}
    assert refs["kinetic"].dim == 72 and refs["geometric"].dim == 32
    x = (torch.rand(2, T * dn, 151, generator=g) * 2 - 1).to(DEV)
    got = S.evaluate_set_all(x, norm, dn, refs, check=True, kinetic=dict(window=1))
    assert list(got) == ["fid_k", "div_k", "fid_g", "div_g"]
    k = S.evaluate_set(x, norm, dn, refs["kinetic"], window=1)
    gm = S.evaluate_set(x, norm, dn, refs["geometric"], features="geometric")
    for name, want in (("fid_k", k["fid"]), ("div_k", k["div"]), ("fid_g", gm["fid"]), ("div_g", gm["div"])):
        assert got[name].is_cuda and got[name].dtype == torch.float64 and got[name].dim() == 0
        _same_bits(got[name], want)
    _, _, poses, _ = E.export_poses(x, norm, "normal", dn)
    by_hand = S.set_scores(S.geometric_features(poses).reshape(2 * dn, 32), refs["geometric"])
    _same_bits(gm["fid"], by_hand["fid"])
    _same_bits(gm["div"], by_hand["div"])
    only = S.evaluate_set_all(x, norm, dn, {"geometric": refs["geometric"]}, geometric=dict(time_per_frame=1 / 120))
    assert list(only) == ["fid_g", "div_g"]
    _same_bits(only["fid_g"], got["fid_g"])
    _same_bits(only["div_g"], got["div_g"])
    assert list(S.evaluate_set_all(x, norm, dn, {"kinetic": refs["kinetic"]}, kinetic=dict(window=1))) == ["fid_k", "div_k"]
    x3 = (torch.rand(3, T * dn, 151, generator=g) * 2 - 1).to(DEV)      # long mode: one song, a set of dn rows
    long = S.evaluate_set_all(x3, norm, dn, refs, mode="long", kinetic=dict(window=1))
    _, _, full, _ = E.export_poses(x3, norm, "long", dn)
    want = S.set_scores(S.geometric_features(full).reshape(dn, 32), refs["geometric"])
    _same_bits(long["fid_g"], want["fid"])
    _same_bits(long["div_g"], want["div"])
