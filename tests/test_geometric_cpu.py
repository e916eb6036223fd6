"""CPU checks of the geometric features (no GPU): the numpy float64 restatement tests/geometric_ref.py on hand-checkable poses; the
conditions on the seeded inputs under which the GPU test may ask for equal bits (no decision a near-tie, every column takes both
values); the product's table against the restatement's copy; csrc/geo_math.h built for the host against the restatement; the host
side of tcdiff_amd.set_metrics.geometric_features (validation, no CPU fallback); and the second header, include/tcdiff_hip_ext.h."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import geometric_ref as G
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd import set_metrics as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _body(T=2):
    """a standing body, z up, facing +y, the left side at +x: (T, 24, 3) float32 with every joint at its own place"""
    J = np.zeros((24, 3))
    for k, (x, y, z) in {G.ROOT: (0, 0, 1.0), G.LHIP: (0.1, 0, 0.95), G.RHIP: (-0.1, 0, 0.95), G.BELLY: (0, 0, 1.1),
                         G.LKNEE: (0.1, 0, 0.5), G.RKNEE: (-0.1, 0, 0.5), G.SPINE: (0, 0, 1.2), G.LANKLE: (0.1, 0, 0.1),
                         G.RANKLE: (-0.1, 0, 0.1), G.CHEST: (0, 0, 1.3), G.LTOES: (0.1, 0.1, 0.0), G.RTOES: (-0.1, 0.1, 0.0),
                         G.NECK: (0, 0, 1.5), G.LINSHOULDER: (0.1, 0, 1.45), G.RINSHOULDER: (-0.1, 0, 1.45), G.HEAD: (0, 0, 1.7),
                         G.LSHOULDER: (0.2, 0, 1.45), G.RSHOULDER: (-0.2, 0, 1.45), G.LELBOW: (0.2, 0, 1.2),
                         G.RELBOW: (-0.2, 0, 1.2), G.LWRIST: (0.2, 0, 0.95), G.RWRIST: (-0.2, 0, 0.95), G.LHAND: (0.2, 0, 0.9),
                         G.RHAND: (-0.2, 0, 0.9)}.items():
        J[k] = (x, y, z)
    return np.repeat(J[None], T, axis=0).astype(np.float32)


def _one(J, table, rng, tau=1 / 120, up=2):
    counts, _ = G.one_dancer(J, up, tau, np.asarray(table, np.int32), np.asarray(rng, np.float64))
    return list(counts)


# ---- the restatement on poses that can be checked by hand ---------------------------------------------------------------------
def test_a_wrist_a_known_distance_in_front_of_the_shoulder_plane():
    """NPLANE with normal lshoulder -> rshoulder through lwrist (row 8's form): the right wrist, 0.4 to the right of the left one,
    is 0.4 along the normal; PLANE through root, lshoulder and neck, the plane y = 0: the wrist 0.25 in front of it"""
    J = _body()
    row = [G.NPLANE, G.LSHOULDER, G.RSHOULDER, G.LWRIST, G.RWRIST]
    assert _one(J, [row, row], [[0.39, 0], [0.41, 0]]) == [1, 0]
    J[:, G.RWRIST, 1] = 0.25                                              # 0.25 in front of the plane y = 0
    # n = (c - a) x (b - a) with a = root, b = lshoulder (+x, up), c = neck (straight up): (0, 0, .5) x (.2, 0, .45) = (0, .1, 0)
    row = [G.PLANE, G.ROOT, G.LSHOULDER, G.NECK, G.RWRIST]
    assert _one(J, [row, row], [[0.2499, 0], [0.2501, 0]]) == [1, 0]
    row = [G.PLANE, G.ROOT, G.NECK, G.LSHOULDER, G.RWRIST]                # b and c exchanged: the other side
    assert _one(J, [row, row], [[-0.2501, 0], [-0.2499, 0]]) == [1, 0]


def test_an_elbow_at_exactly_ninety_degrees():
    J = _body()
    J[:, G.LWRIST] = J[:, G.LELBOW] + np.float32([0, 0.25, 0])            # the forearm forward, the upper arm up
    row = [G.ANGLE, G.LELBOW, G.LSHOULDER, G.LELBOW, G.LWRIST]
    assert _one(J, [row] * 4, [[0, 110], [89.999, 90.001], [90.001, 180], [0, 89.999]]) == [1, 1, 0, 0]
    assert _one(J, [row, row], [[90.0, 180.0], [0.0, 90.0]]) == [0, 0]   # both bounds are strict (acos(0) 180 / pi is 90 exactly)
    J = _body()                                                          # the arm straight down: the forearm opposes the upper arm
    assert _one(J, [row, row], [[0, 110], [110, 180.1]]) == [0, 1]


def test_a_joint_moving_at_a_known_speed_along_and_across_a_direction():
    tau = 0.125
    J = _body(3)
    J[1, G.RWRIST] += np.float32([0.125, 0, 0])                           # frame 1: 1 m/s along +x, towards the left wrist
    J[2, G.RWRIST] = J[1, G.RWRIST] + np.float32([0, 0.5, 0])             # frame 2: 4 m/s along +y, across it
    fast = [G.FAST, G.RWRIST, G.RWRIST, G.RWRIST, G.RWRIST]
    assert _one(J, [fast] * 3, [[0.999, 0], [1.001, 0], [4.001, 0]], tau) == [2, 1, 0]
    move = [G.MOVE, G.ROOT, G.LWRIST, G.HEAD, G.RWRIST]                   # relative to the root, along root -> lwrist = (.2, 0, -.05)
    along = 1.0 * 0.2 / np.sqrt(0.2 ** 2 + 0.05 ** 2)
    assert _one(J, [move] * 3, [[along - 1e-3, 0], [along + 1e-3, 0], [1e-9, 0]], tau) == [1, 0, 1]     # frame 2 moves across: v = 0
    away = [G.MOVE, G.ROOT, G.RWRIST, G.HEAD, G.RWRIST]                   # along root -> rwrist: frame 1 approaches the root
    assert _one(J, [away], [[0.0, 0]], tau) == [1]                        # (negative), frame 2 leaves it
    nmove = [G.NMOVE, G.ROOT, G.LSHOULDER, G.NECK, G.RWRIST]              # the normal of that plane is +y (see above)
    assert _one(J, [nmove] * 2, [[3.999, 0], [4.001, 0]], tau) == [1, 0]
    both = _body(2)                                                       # a and p move together: no relative motion
    both[1] += np.float32([0.3, 0.3, 0.0])
    assert _one(both, [move, nmove, fast], [[1e-9, 0], [1e-9, 0], [3.39, 0]], tau) == [0, 0, 1]       # |(.3, .3)| / .125 = 3.394


def test_a_body_lying_flat_and_the_floor_from_the_lowest_joint():
    """row 28: the angle of root -> neck against `up` is 0 standing and 90 lying; rows 16 / 17: the ankle above the floor"""
    table, rng = G.default_table()
    stand = _body()
    lying = stand[:, :, [0, 2, 1]].copy()                                 # the body's axis along y
    lying[:, :, 2] += 0.2
    assert G.one_dancer(stand, 2, 1 / 120, table, rng)[0][28] == 0 and G.one_dancer(lying, 2, 1 / 120, table, rng)[0][28] == 1
    assert G.one_dancer(lying, 1, 1 / 120, table, rng)[0][28] == 0       # with y up it stands again
    # the floor is the lowest joint (the toes at z = 0): the ankle is 0.1 above it, 1.2 hl = 0.308 is not reached ...
    assert G.points(stand, 2)[0, G.FLOOR].tolist() == [0.0, 0.0, 0.0]
    assert list(G.one_dancer(stand, 2, 1 / 120, table, rng)[0][16:18]) == [0, 0]
    jump = stand.copy()
    jump[:, G.RANKLE, 2] = 0.4                                            # ... one raised ankle is
    assert list(G.one_dancer(jump, 2, 1 / 120, table, rng)[0][16:18]) == [1, 0]
    jump[:, G.LHAND, 2] = -0.25                                           # a hand 0.25 below the toes lowers the floor under both
    assert G.points(jump, 2)[1, G.FLOOR].tolist() == [0.0, 0.0, -0.25]
    assert list(G.one_dancer(jump, 2, 1 / 120, table, rng)[0][16:18]) == [1, 1]
    # rows 29 / 30, normal -up through the floor, threshold -1.2 hl: the wrist (0.95) is BELOW 1.2 hl above the floor?  no
    assert list(G.one_dancer(stand, 2, 1 / 120, table, rng)[0][29:31]) == [0, 0]
    low = stand.copy()
    low[:, G.LWRIST, 2] = 0.3
    assert list(G.one_dancer(low, 2, 1 / 120, table, rng)[0][29:31]) == [0, 1]


def test_zero_length_normal_nan_joint_and_a_single_frame():
    J = _body(3)
    angle = [G.ANGLE, G.LELBOW, G.LELBOW, G.LELBOW, G.LWRIST]             # b - a = 0: 0 / 0
    nplane = [G.NPLANE, G.NECK, G.NECK, G.ROOT, G.HEAD]
    plane = [G.PLANE, G.ROOT, G.NECK, G.HEAD, G.LWRIST]                   # three points on a line: the cross product is zero
    assert _one(J, [angle, nplane, plane], [[-1, 181], [-1e300, 0], [-1e300, 0]]) == [0, 0, 0]
    J[1, G.LWRIST, 0] = np.nan
    fast_l = [G.FAST, G.LWRIST, G.LWRIST, G.LWRIST, G.LWRIST]
    fast_r = [G.FAST, G.RWRIST, G.RWRIST, G.RWRIST, G.RWRIST]
    assert _one(J, [fast_l, fast_r], [[-1.0, 0], [-1.0, 0]]) == [0, 2]   # frames 1 and 2 both read the NaN; the other wrist does not
    J = _body(4)
    J[1, G.LWRIST, 2] = np.nan                                            # in the `up` component the floor of frame 1 is NaN too
    above = [G.NPLANE, G.ZERO, G.UP, G.FLOOR, G.RANKLE]
    assert _one(J, [above, fast_l], [[-1.0, 0], [-1.0, 0]]) == [2, 1]
    feats, counts, margin = G.geometric_features(_body(1)[None, None])
    assert feats.shape == (1, 1, 32) and np.isnan(feats).all() and margin == np.inf


# ---- conditions on the seeded inputs -------------------------------------------------------------------------------------------
def test_no_seeded_decision_is_a_near_tie_and_every_column_takes_both_values():
    """shown on the restatement alone, before any other implementation is asked for equal bits"""
    margin, fires, rests, fires_a = np.inf, np.zeros(32, bool), np.zeros(32, bool), np.zeros(32, bool)
    for fam, shape in G.CASES:
        _, _, (feats, counts, m) = G.case(fam, shape)
        print(f"{fam} {shape}: smallest margin {m:.3e}")
        margin = min(margin, m)
        if shape[2] >= 2:
            fires |= (feats > 0).any((0, 1))
            rests |= (feats < 1).any((0, 1))
            if fam == "A":
                fires_a |= (feats > 0).any((0, 1)) & (feats < 1).any((0, 1))
            assert np.array_equal(feats, counts / np.float64(shape[2] - 1)) and counts.max() <= shape[2] - 1
    print(f"smallest margin {margin:.3e}; columns with both values in family A alone: {int(fires_a.sum())}")
    assert margin >= G.MIN_MARGIN
    assert fires.all() and rests.all()


# ---- the product's table ----------------------------------------------------------------------------------------------------------
def test_the_products_table_is_the_restatements():
    table, rng = S.geometric_table()
    want_t, want_r = G.default_table()
    assert table.dtype == np.int32 and rng.dtype == np.float64 and np.array_equal(table, want_t) and np.array_equal(rng, want_r)
    assert len(S.GEOMETRIC_TABLE) == S.N_GEOMETRIC == 32
    for row, (kind, a, b, c, p, lo, hi) in zip(S.GEOMETRIC_TABLE, G.ROWS):
        assert (S.GEO_KINDS.index(row[0]),) + tuple(S.GEO_POINTS.index(n) for n in row[1:5]) == (kind, a, b, c, p)
        if kind == G.ANGLE:
            assert row[5:] == (lo, hi)
        else:
            assert row[6] in ("hl", "sw", "hw") and row[5] * S.geometric_lengths()[row[6]] == lo
    ln = S.geometric_lengths()
    assert abs(ln["hl"] - 0.25683810921) < 1e-11 and abs(ln["sw"] - 0.39084835854) < 1e-11 and abs(ln["hw"] - 0.11924706586) < 1e-11
    assert abs(ln["hl"] - G.HL) < 1e-12 and abs(ln["sw"] - G.SW) < 1e-12 and abs(ln["hw"] - G.HW) < 1e-12
    assert [L.GEO_PLANE, L.GEO_NPLANE, L.GEO_MOVE, L.GEO_NMOVE, L.GEO_ANGLE, L.GEO_FAST] == list(range(6)) == \
        [S.GEO_KINDS.index(k) for k in G.KINDS] and L.GEO_POINTS == len(S.GEO_POINTS) == 28
    t2, r2 = S.geometric_table({"hl": 1.0})
    assert np.array_equal(t2, table) and r2[0, 0] == 1.8 and r2[8, 0] == rng[8, 0] and r2[6].tolist() == [0.0, 110.0]
    with pytest.raises(L.TcdiffError, match="lengths"):
        S.geometric_table({"arm": 1.0})


# ---- csrc/geo_math.h on the host ------------------------------------------------------------------------------------------------
def test_geo_math_on_the_host_counts_what_the_restatement_counts(tmp_path):
    """the SAME source the HIP kernel compiles, built with g++ without contraction: equal counts on both families, on the
    hand-made degenerate rows and on a table with entries out of range"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    so = str(tmp_path / "geometric_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "host", "geometric_host.cpp")])
    lib = C.CDLL(so)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def host(J, up, tau, table, rng):
        J, table, rng = np.ascontiguousarray(J, np.float32), np.ascontiguousarray(table, np.int32), np.ascontiguousarray(rng, np.float64)
        out = np.zeros(len(table), np.int64)
        lib.host_geometric_counts(vp(J), C.c_int(J.shape[0]), C.c_int(up), vp(table), vp(rng), C.c_int(len(table)), C.c_double(tau),
                                  vp(out))
        return out
    table, rng = G.default_table()
    frames = 0
    for fam, shape in G.CASES:
        J, tau, (_, counts, _) = G.case(fam, shape)
        for c in range(shape[0]):
            for d in range(shape[1]):
                assert np.array_equal(host(J[c, d], 2, tau, table, rng), counts[c, d]), (fam, shape, c, d)
                frames += shape[2] - 1
    print(f"{frames} frames x 32 rows")
    J, tau, _ = G.case("B", (1, 2, 65))
    turned = np.ascontiguousarray(J[0, 1][:, :, [1, 2, 0]])               # the same motion with the up axis moved to 1
    want, m = G.one_dancer(turned, 1, tau, table, rng)
    assert m >= G.MIN_MARGIN and np.array_equal(host(turned, 1, tau, table, rng), want)
    assert np.array_equal(want, G.case("B", (1, 2, 65))[2][1][0, 1])
    bad = table.copy()
    bad[3, 0], bad[7, 2], bad[9, 4] = 9, 40, -1
    Jn = J[0, 0].copy()
    Jn[7, G.LWRIST, 2] = np.nan
    want, m = G.one_dancer(Jn, 2, tau, bad, rng)
    assert m >= G.MIN_MARGIN and want[3] == want[7] == want[9] == 0 and np.array_equal(host(Jn, 2, tau, bad, rng), want)
    deg = [[G.ANGLE, G.LELBOW, G.LELBOW, G.LELBOW, G.LWRIST], [G.NPLANE, G.NECK, G.NECK, G.ROOT, G.HEAD],
           [G.PLANE, G.ROOT, G.ROOT, G.HEAD, G.LWRIST], [G.FAST, 0, 0, 0, G.LWRIST]]
    assert host(J[0, 0], 2, tau, deg, [[-1, 181], [-1e300, 0], [-1e300, 0], [-1.0, 0]]).tolist() == [0, 0, 0, 64]
    assert host(J[0, 0][:1], 2, tau, table, rng).tolist() == [0] * 32


# ---- the host side ----------------------------------------------------------------------------------------------------------------
def test_no_cpu_fallback_and_input_checks():
    ok = torch.zeros(1, 2, 5, 24, 3)
    with pytest.raises(L.TcdiffError, match="MI355X"):
        S.geometric_features(ok)
    with pytest.raises(L.TcdiffError, match="joints must be"):
        S.geometric_features(torch.zeros(1, 2, 5, 72))
    with pytest.raises(L.TcdiffError, match="float32"):
        S.geometric_features(ok.double())
    with pytest.raises(L.TcdiffError, match="contiguous"):
        S.geometric_features(torch.zeros(1, 2, 5, 3, 24).transpose(-1, -2))
    with pytest.raises(L.TcdiffError, match="empty"):
        S.geometric_features(torch.zeros(1, 0, 5, 24, 3))
    for bad in (dict(up=3), dict(up=-1), dict(up=1.5)):
        with pytest.raises(L.TcdiffError, match="up must be"):
            S.geometric_features(ok, **bad)
    for tau in (0, -1 / 120, float("inf"), float("nan")):
        with pytest.raises(L.TcdiffError, match="time_per_frame"):
            S.geometric_features(ok, time_per_frame=tau)
    with pytest.raises(L.TcdiffError, match="lengths"):
        S.geometric_features(ok, lengths={"hl": float("nan")})
    table, rng = S.geometric_table()
    with pytest.raises(L.TcdiffError, match="MI355X"):                     # a good table of the caller's passes the host's checks
        S.geometric_features(ok, table=(table, rng))
    with pytest.raises(L.TcdiffError, match="MI355X"):
        S.geometric_features(ok, table=(table[:1].tolist(), rng[:1].tolist()))
    with pytest.raises(L.TcdiffError, match="carries its own"):
        S.geometric_features(ok, table=(table, rng), lengths={"hl": 1.0})

    def refused(t, r, match):
        with pytest.raises(L.TcdiffError, match=match):
            S.geometric_features(ok, table=(t, r))
    t = table.copy()
    t[5, 0] = 6
    refused(t, rng, "kind")
    t[5, 0] = -1
    refused(t, rng, "kind")
    t = table.copy()
    t[31, 4] = 28
    refused(t, rng, "point")
    t[31, 4], t[0, 1] = 0, -1
    refused(t, rng, "point")
    refused(np.concatenate([table] * 3)[:73], np.concatenate([rng] * 3)[:73], "1 to 72 table rows")
    refused(table[:0], rng[:0], "1 to 72 table rows")
    r = rng.copy()
    r[2, 1] = np.inf
    refused(table, r, "finite")
    r[2, 1] = np.nan
    refused(table, r, "finite")
    refused(table, rng[:31], "pair")
    refused(table[:, :4], rng, "pair")
    refused(table.astype(np.float64), rng, "pair")
    refused(table, None, "pair")
    with pytest.raises(L.TcdiffError, match="pair"):
        S.geometric_features(ok, table=table)
    with pytest.raises(L.TcdiffError, match="MI355X"):
        S.reference_from_joints(torch.zeros(2, 2, 5, 24, 3), features="geometric")
    with pytest.raises(L.TcdiffError, match="features must be"):
        S.reference_from_joints(torch.zeros(2, 2, 5, 24, 3), features="kinematic")
    with pytest.raises(L.TcdiffError, match="features must be"):
        S.evaluate_set(None, None, 3, None, features="g")
    with pytest.raises(L.TcdiffError, match="refs maps"):
        S.evaluate_set_all(None, None, 3, {})
    with pytest.raises(L.TcdiffError, match="refs maps"):
        S.evaluate_set_all(None, None, 3, {"fid_g": None})


def test_the_launcher_validates_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    lib = L.load()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    s3 = (C.c_long * 3)(0, 0, 0)

    def geo(joints=p, js=s3, b=1, dn=1, T=3, up=2, table=p, rng=p, R=32, tau=1 / 120, out=p):
        return lib.tcdiff_geometric_features(joints, js, b, dn, T, up, table, rng, R, tau, out, None)
    assert geo(joints=None) == -1 and geo(js=None) == -1 and geo(table=None) == -1 and geo(rng=None) == -1 and geo(out=None) == -1
    assert geo(b=0) == -1 and geo(dn=0) == -1 and geo(T=0) == -1 and geo(R=0) == -1 and geo(up=3) == -1 and geo(up=-1) == -1
    assert geo(tau=0.0) == -1 and geo(tau=-1.0) == -1 and geo(tau=float("nan")) == -1 and geo(tau=float("inf")) == -1
    assert geo(R=73) == -4 and geo(R=1 << 20) == -4
    assert geo(b=1 << 20, dn=1 << 20) == -4


# ---- the second header ---------------------------------------------------------------------------------------------------------
def _dynamic_symbols(path):
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split()}
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", path], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    return {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}


def test_the_second_header_parses_and_the_first_is_unchanged():
    ext = _abi.load_ext()
    assert ext.structs == {} and list(ext.functions) == ["tcdiff_geometric_features"]
    assert ext.constants == {"TC_GEO_PLANE": 0, "TC_GEO_NPLANE": 1, "TC_GEO_MOVE": 2, "TC_GEO_NMOVE": 3, "TC_GEO_ANGLE": 4,
                             "TC_GEO_FAST": 5, "TC_GEO_POINTS": 28}
    I, VP = C.c_int, C.c_void_p
    assert ext.functions["tcdiff_geometric_features"] == (
        I, [VP, VP, I, I, I, I, VP, VP, I, C.c_double, VP, VP],
        ["const float*", "const long*", "int", "int", "int", "int", "const int*", "const double*", "int", "double", "double*",
         "hipStream_t"])
    for abi in (_abi.load(), L.ABI):
        assert len(abi.structs) == 17 and len(abi.functions) == 79 and "tcdiff_geometric_features" not in abi.functions
        assert not any(k.startswith("TC_GEO_") for k in abi.constants)
    assert L.EXT.functions.keys() == ext.functions.keys() and L.EXT.constants == ext.constants
    assert L.EXPORTS == sorted(list(L.ABI.functions) + list(L.EXT.functions)) and len(L.EXPORTS) == 80
    from tcdiff_amd import build
    build.build(verbose=False)
    assert "tcdiff_geometric_features" in _dynamic_symbols(L.LIB_PATH)
    assert L.load().tcdiff_geometric_features.argtypes == ext.functions["tcdiff_geometric_features"][1]
    with open(_abi.HEADER_EXT) as f:
        text = f.read()
    assert text.count('#include "tcdiff_hip.h"') == 1 and "NOT pinned" in text


def test_the_second_header_read_by_the_c_compiler(tmp_path):
    """what test_ctypes_structures_match_the_header does for the first header: the macro values, and a translation unit that calls
    the launcher with every argument cast to its parsed C type and assigns it to a function pointer of the parsed signature"""
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    ext = L.EXT
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    src = ['#include <stdio.h>', '#include "tcdiff_hip_ext.h"', "int main(void) {"]
    src += [f'  printf("%ld\\n", (long)({macro}));' for macro in ext.constants]
    src += ['  printf("%ld\\n", (long)(TC_SET_MAX_D));', "  return 0;", "}"]
    cfile, exe = tmp_path / "ext.c", tmp_path / "ext"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + [str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == list(ext.constants.values()) + [L.SET_MAX_D]
    calls = ['#include "tcdiff_hip_ext.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in ext.functions.items():
        assert restype is C.c_int and argtypes == [C.c_void_p if c.endswith("*") else _abi.SCALARS[c] for c in ctexts], fname
        calls.append(f"  {{ int (*f)({', '.join(ctexts)}) = {fname}; (void)f; }}")
        zeros = [f"({c})0" if c.endswith("*") or c == "hipStream_t" else f"({c})z" for c in ctexts]
        calls.append(f"  (void){fname}({', '.join(zeros)});")
    calls.append("}")
    tu = tmp_path / "calls.c"
    tu.write_text("\n".join(calls))
    r = subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-c", str(tu), "-o", str(tmp_path / "calls.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_package_exports_the_geometric_features():
    import tcdiff_amd
    for name in ("GEOMETRIC_TABLE", "geometric_features", "geometric_table", "evaluate_set_all"):
        assert getattr(tcdiff_amd, name) is getattr(S, name) and name in tcdiff_amd.__all__
