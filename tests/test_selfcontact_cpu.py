"""CPU checks of the self-contact metric (no GPU): the numpy restatement tests/selfcontact_ref.py of include/tcdiff_selfcontact.h on
bodies that can be checked by hand, the default list of bone pairs against its loop restatement, the twelfth header and its binding,
the launchers' refusals, csrc/selfcontact_math.h with csrc/group_math.h built for the host as a stand-alone program with the address
and undefined-behaviour sanitizers against the restatement, and the conditions the GPU comparison rests on: on the seeded scenes no
decision of the metric is a near-tie, and the scenes are not trivial."""
import ctypes as C
import importlib
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import group_ref
import selfcontact_ref as R
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS

S = importlib.import_module("tcdiff_amd.self_contact")          # the package's attribute of this name is the function
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tci_self_contact_workspace", "tci_self_contact"]
QUARTER = np.full(24, 0.25)
ONE = dict(parents=R.CHAIN, radii=QUARTER, mask=R.pair_mask([(1, 3)]), tolerance=0.125)


def clip(J):
    return np.asarray(J, np.float32)[None, None]


# ---- 1. bodies that can be checked by hand --------------------------------------------------------------------------------------------------
def test_a_fold_brings_two_bones_to_a_known_distance():
    ref = R.self_contact(clip(R.bars([1.0])), **ONE)
    assert ref["gap"][0, 0, 0] == (1.0 - 0.25) - 0.25 == 0.5 and ref["closest"][0, 0, 0] == 24 * 1 + 3
    assert ref["self_contact_rate"][0, 0] == 0.0 and ref["self_contact_episodes"][0, 0] == 0 and np.isnan(ref["self_depth_mean"][0, 0])
    assert ref["self_gap_min"][0, 0] == 0.5 and ref["self_closest"][0, 0].tolist() == [0, 1, 3] and not ref["self_pair_frames"].any()
    ref = R.self_contact(clip(R.bars([0.125])), **ONE)
    assert ref["gap"][0, 0, 0] == -0.375 and ref["self_contact_rate"][0, 0] == 1.0 and ref["self_depth_mean"][0, 0] == 0.375
    assert ref["self_pair_frames"][0, 0, R.PAIRS.index((1, 3))] == 1 and ref["self_pair_frames"].sum() == 1


def test_contact_is_strictly_deeper_than_the_tolerance():
    at, deeper = R.bars([0.375]), R.bars([0.25])                        # gaps of -0.125 (the tolerance itself) and -0.25
    assert R.self_contact(clip(at), **ONE)["gap"][0, 0, 0] == -0.125
    assert R.self_contact(clip(at), **ONE)["self_contact_rate"][0, 0] == 0.0 and not R.self_contact(clip(at), **ONE)["self_pair_frames"].any()
    assert R.self_contact(clip(deeper), **ONE)["self_contact_rate"][0, 0] == 1.0
    zero = dict(ONE, tolerance=0.0)
    assert R.self_contact(clip(R.bars([0.5])), **zero)["gap"][0, 0, 0] == 0.0                    # touching is no contact
    assert R.self_contact(clip(R.bars([0.5])), **zero)["self_contact_rate"][0, 0] == 0.0
    assert R.self_contact(clip(at), **zero)["self_contact_rate"][0, 0] == 1.0


def test_episodes_the_minimum_the_depth_and_a_nan_joint():
    a = [1.0, 0.25, 0.25, 1.0, 0.125, 1.0, 0.25, 1.0]                   # contact on frames 1-2, 4, 6: three episodes
    J = R.bars(a)
    ref = R.self_contact(clip(J), **ONE)
    assert ref["gap"][0, 0].tolist() == [0.5, -0.25, -0.25, 0.5, -0.375, 0.5, -0.25, 0.5]
    assert ref["self_contact_episodes"][0, 0] == 3 and ref["self_contact_rate"][0, 0] == 0.5
    assert ref["self_gap_min"][0, 0] == -0.375 and ref["self_closest"][0, 0].tolist() == [4, 1, 3]
    assert ref["self_depth_mean"][0, 0] == (0.25 + 0.25 + 0.375 + 0.25) / 4 and ref["self_pair_frames"][0, 0, R.PAIRS.index((1, 3))] == 4
    J2 = J.copy()
    J2[4] = J2[2]                                                       # frames 1, 2, 4 and 6 now tie: the first frame wins
    assert R.self_contact(clip(J2), **ONE)["self_closest"][0, 0].tolist() == [1, 1, 3]
    J[4, 3, 1] = np.nan                                                 # the deepest frame loses a joint: it is skipped, not a contact
    ref = R.self_contact(clip(J), **ONE)
    assert np.isnan(ref["gap"][0, 0, 4]) and ref["closest"][0, 0, 4] == 27 and np.isfinite(np.delete(ref["gap"][0, 0], 4)).all()
    assert ref["self_contact_episodes"][0, 0] == 2 and ref["self_contact_rate"][0, 0] == 3 / 8
    assert ref["self_closest"][0, 0].tolist() == [1, 1, 3] and ref["self_gap_min"][0, 0] == -0.25 and ref["self_depth_mean"][0, 0] == 0.25
    assert ref["self_pair_frames"][0, 0, R.PAIRS.index((1, 3))] == 3
    J[:, 3, 1] = np.nan
    ref = R.self_contact(clip(J), **ONE)
    assert np.isnan(ref["self_gap_min"][0, 0]) and ref["self_closest"][0, 0].tolist() == [-1, -1, -1] and np.isnan(ref["self_depth_mean"][0, 0])
    assert ref["self_contact_rate"][0, 0] == 0.0 and ref["self_contact_episodes"][0, 0] == 0 and not ref["self_pair_frames"].any()
    # a NaN on a bone that is not listed changes nothing; among several NaN pairs the smallest code is reported
    K = R.bars(a)
    K[:, 9, 0] = np.nan
    assert np.array_equal(R.self_contact(clip(K), **ONE)["gap"], R.self_contact(clip(R.bars(a)), **ONE)["gap"])
    two = dict(ONE, mask=R.pair_mask([(1, 3), (1, 5), (3, 5)]))
    K = R.bars(a)
    K[:, 5, 2] = np.nan                                                 # bone 5: the pairs (1, 5) and (3, 5)
    ref = R.self_contact(clip(K), **two)
    assert np.isnan(ref["gap"]).all() and (ref["closest"] == 24 * 1 + 5).all() and ref["self_pair_frames"][0, 0, R.PAIRS.index((1, 3))] == 4


def test_pair_frames_tell_which_limbs():
    a, b = [0.25, 1.0, 0.25, 1.0], [1.0, 0.25, 0.25, 0.25]
    kw = dict(ONE, mask=R.pair_mask([(1, 3), (1, 5)]))
    ref = R.self_contact(clip(R.bars(a, b)), **kw)
    k13, k15, k35 = (R.PAIRS.index(p) for p in ((1, 3), (1, 5), (3, 5)))
    assert ref["self_pair_frames"][0, 0, k13] == 2 and ref["self_pair_frames"][0, 0, k15] == 3 and ref["self_pair_frames"].sum() == 5
    assert ref["gap"][0, 0].tolist() == [-0.25, -0.25, -0.25, -0.25] and ref["closest"][0, 0].tolist() == [27, 29, 27, 29]
    assert ref["self_closest"][0, 0].tolist() == [0, 1, 3] and ref["self_contact_episodes"][0, 0] == 1
    ref = R.self_contact(clip(R.bars(a, b)), **dict(kw, mask=R.pair_mask([(1, 3), (1, 5), (3, 5)])))
    assert ref["self_pair_frames"][0, 0, k35] == 1                      # bones 3 and 5 are sqrt(1/8) apart in frame 2 alone
    assert ref["closest"][0, 0].tolist() == [27, 29, 27, 29]            # its gap there, sqrt(1/8) - 1/2, is not the frame's smallest


def test_the_exact_tie_takes_the_smallest_code_and_the_first_frame():
    J = R.tie_body(T=2)
    kw = dict(parents=R.CHAIN, radii=QUARTER, mask=R.pair_mask([(1, 5), (2, 5)]), tolerance=0.0)
    ref = R.self_contact(clip(J), details=True, **kw)
    g = R.pair_gaps(J[0], QUARTER, R.CHAIN)
    assert g[R.PAIRS.index((1, 5))] == g[R.PAIRS.index((2, 5))] == (np.sqrt(3.0) - 0.25) - 0.25
    assert (ref["closest"] == 24 * 1 + 5).all() and ref["self_closest"][0, 0].tolist() == [0, 1, 5]
    assert (ref["details"]["frame_lead"] == 0.0).all() and ref["details"]["dancer_lead"] == 0.0 and not R.judge(ref)[0]
    assert R.self_contact(clip(J), **dict(kw, mask=R.pair_mask([(2, 5)])))["closest"][0, 0, 0] == 24 * 2 + 5


def test_the_depth_sum_follows_the_lane_order():
    g = np.random.default_rng(3)
    gap = -g.uniform(0.01, 0.2, 200)
    con = g.uniform(size=200) < 0.6
    lanes = [sum((-gap[t] for t in range(l, 200, 64) if con[t]), 0.0) for l in range(64)]
    for o in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
    assert R.depth_sum(gap, con) == lanes[0] and abs(lanes[0] - float((-gap[con]).sum())) < 1e-12
    assert R.depth_sum(gap[:3], [False] * 3) == 0.0


# ---- 2. the list of bone pairs -----------------------------------------------------------------------------------------------------------------
def test_pair_index_pair_of_and_pair_mask_round_trip():
    idx = S.pair_index()
    assert idx == R.PAIRS and len(idx) == 253 == S.PAIRS and idx[0] == (1, 2) and idx[1] == (1, 3) and idx[22] == (2, 3) and idx[-1] == (22, 23)
    assert idx == sorted(idx) and all(1 <= i < j <= 23 for i, j in idx)
    assert all(S.pair_of(k) == idx[k] for k in range(253))
    idx.clear()
    assert len(S.pair_index()) == 253                                   # a fresh list every call
    m = S.pair_mask([(1, 3), (20, 3), (22, 23)])
    assert m.dtype == np.bool_ and m.shape == (253,) and [S.pair_of(int(k)) for k in np.flatnonzero(m)] == [(1, 3), (3, 20), (22, 23)]
    assert np.array_equal(m, R.pair_mask([(1, 3), (20, 3), (22, 23)]))
    assert np.array_equal(S.pair_mask([S.pair_of(int(k)) for k in np.flatnonzero(R.self_pairs())]), R.self_pairs())
    assert not S.pair_mask([]).any()
    for bad in (-1, 253, 1.0, True, "3"):
        with pytest.raises(L.TcdiffError, match="pair_of"):
            S.pair_of(bad)
    for bad in ([(0, 3)], [(3, 3)], [(3, 24)], [(1, 2, 3)], [5], 7):
        with pytest.raises(L.TcdiffError, match="pair_mask"):
            S.pair_mask(bad)


def test_self_pairs_equals_its_loop_restatement():
    assert R.OFFSETS.tolist() == SMPL_OFFSETS and R.SMPL_PARENTS == list(SMPL_PARENTS)
    assert np.array_equal(S.rest_pose(), R.rest_pose())
    got = S.self_pairs()
    assert got.dtype == np.bool_ and got.shape == (253,) and np.array_equal(got, R.self_pairs())
    assert int(got.sum()) == int(R.self_pairs().sum()) == 183           # the count the restatement gives with the defaults
    listed = {S.pair_of(int(k)) for k in np.flatnonzero(got)}
    assert (20, 3) not in listed and (3, 20) in listed and (21, 15) not in listed and (15, 21) in listed          # a forearm and the trunk, the head
    assert (1, 2) not in listed and (4, 5) not in listed and (3, 6) not in listed          # the hips, the thighs (3 cm into each other at rest), the spine
    for hops in range(4):
        assert np.array_equal(S.self_pairs(hops=hops), R.self_pairs(hops=hops)), hops
        assert np.array_equal(S.self_pairs(hops=hops, rest_margin=-1.0), R.self_pairs(hops=hops, rest_margin=-1.0)), hops
    none_out = S.self_pairs(hops=0, rest_margin=-10.0)
    assert none_out.all()                                               # no two different bones are 0 hops apart
    only_hops = [int(S.self_pairs(hops=h, rest_margin=-10.0).sum()) for h in range(5)]
    assert only_hops == sorted(only_hops, reverse=True) and only_hops[1] < 253
    parents, radii = group_ref.custom_skeleton()
    assert np.array_equal(S.self_pairs(parents=parents, radii=radii), R.self_pairs(parents=parents, radii=radii))
    g = np.random.default_rng(8)
    rest = R.rest_pose() * 1.1 + g.normal(0, 0.01, (24, 3))
    for kw in (dict(rest_joints=rest), dict(rest_joints=rest, radii=radii, hops=1, rest_margin=0.02), dict(rest_joints=torch.from_numpy(rest))):
        ref_kw = dict(kw, rest_joints=rest)
        assert np.array_equal(S.self_pairs(**kw), R.self_pairs(**ref_kw)), sorted(kw)
    assert not np.array_equal(S.self_pairs(rest_joints=rest * 0.5), S.self_pairs(rest_joints=rest))
    for bad in (dict(hops=-1), dict(hops=1.0), dict(hops=True), dict(rest_margin=float("nan")), dict(rest_margin="x"), dict(radii=np.ones(23)),
                dict(radii=-np.ones(24)), dict(parents=SMPL_PARENTS[:5]), dict(rest_joints=np.zeros((23, 3))), dict(rest_joints=np.full((24, 3), np.nan))):
        with pytest.raises(L.TcdiffError, match="self_pairs"):
            S.self_pairs(**bad)


def test_self_pairs_is_symmetric_in_left_and_right_for_a_mirrored_rest_pose():
    left = [1, 4, 7, 10, 13, 16, 18, 20, 22]
    mirror = {j: j for j in range(24)}
    mirror.update({j: j + 1 for j in left})
    mirror.update({j + 1: j for j in left})
    rest = R.rest_pose()
    for j in range(24):
        if mirror[j] == j:
            rest[j, 0] = 0.0
    for j in left:
        rest[j + 1] = rest[j] * np.array([-1.0, 1.0, 1.0])
    for kw in (dict(), dict(hops=1), dict(rest_margin=0.1)):
        m = S.self_pairs(rest_joints=rest, **kw)
        listed = {S.pair_of(int(k)) for k in np.flatnonzero(m)}
        assert listed and listed == {tuple(sorted((mirror[i], mirror[j]))) for i, j in listed}, kw
        assert np.array_equal(m, R.self_pairs(rest_joints=rest, **kw))


# ---- csrc/selfcontact_math.h on the host, under the sanitizers -------------------------------------------------------------------------------
def run_host(exe, tmp, J, radii, parents, mask, tolerance):
    T = J.shape[0]
    words = [0, 0, 0, 0]
    for k in np.flatnonzero(mask):
        words[int(k) >> 6] |= 1 << (int(k) & 63)
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([T, 0], np.int32).tobytes() + np.array([tolerance] + list(radii), np.float64).tobytes() +
                np.array([0] + list(parents[1:]), np.int32).tobytes() + np.array(words, np.uint64).tobytes() +
                np.ascontiguousarray(J, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.frombuffer((tmp / "out.bin").read_bytes(), np.float64)
    assert raw.size == 253 + 2 * T + 7 + 253
    return raw[:253], raw[253:253 + T], raw[253 + T:253 + 2 * T], raw[253 + 2 * T:253 + 2 * T + 7], raw[253 + 2 * T + 7:]


def compare_host(exe, tmp, J, **kw):
    """one dancer (T, 24, 3): the host program against the restatement; returns the largest difference of a floating-point output"""
    ref = R.self_contact(J[None, None], **kw)
    args = dict(R.DEFAULTS, **kw)
    radii = R.capsule_radii() if args["radii"] is None else args["radii"]
    parents = R.SMPL_PARENTS if args["parents"] is None else args["parents"]
    mask = args["mask"] if args["mask"] is not None else R.self_pairs(radii=radii, parents=parents, hops=args["hops"], rest_margin=args["rest_margin"])
    table, gap, code, (rate, episodes, gap_min, t, i, j, depth), frames = run_host(exe, tmp, J, radii, parents, mask, args["tolerance"])
    assert table.tolist() == [24 * a + b for a, b in R.PAIRS]          # tci_pair_of's closed form
    assert np.array_equal(code, ref["closest"][0, 0]) and np.array_equal(frames, ref["self_pair_frames"][0, 0])
    assert episodes == ref["self_contact_episodes"][0, 0] and [t, i, j] == ref["self_closest"][0, 0].tolist()
    worst = 0.0
    for mine, theirs in ((gap, ref["gap"][0, 0]), (np.array([rate, gap_min, depth]),
                                                    np.array([ref[k][0, 0] for k in ("self_contact_rate", "self_gap_min", "self_depth_mean")]))):
        assert np.array_equal(np.isnan(mine), np.isnan(theirs))
        if (~np.isnan(theirs)).any():
            worst = max(worst, float(np.nanmax(np.abs(mine - theirs))))
    assert worst <= 1e-12, worst
    return worst


def test_selfcontact_math_on_the_host_under_the_sanitizers_agrees_with_the_restatement(tmp_path):
    """the SAME functions the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined; the gaps are
    expected to be EQUAL (the same float64 operations in the same order), 1e-12 is the bound should a platform round otherwise"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "selfcontact_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "selfcontact_host.cpp")])
    worst = 0.0
    for shape in [(1, 1, 1), (1, 2, 3), (2, 3, 5), (1, 1, 70)]:
        J = R.synth(*shape)
        for c in range(shape[0]):
            for d in range(shape[1]):
                worst = max(worst, compare_host(exe, tmp_path, J[c, d], radii=R.scene_radii()))
                worst = max(worst, compare_host(exe, tmp_path, J[c, d]))          # the default radii, exact ties and all
    for shape, seed, kw in R.parameter_cases():
        J = R.synth(*shape, seed=seed)
        worst = max(worst, compare_host(exe, tmp_path, J[0, 1], **kw))
    a = [1.0, 0.25, 0.25, 1.0, 0.125, 1.0, 0.25, 1.0]
    nan = R.bars(a)
    nan[4, 3, 1] = np.nan
    for J, kw in ((R.bars(a), ONE), (nan, ONE), (R.bars(a, a[::-1]), dict(ONE, mask=R.pair_mask([(1, 3), (1, 5), (3, 5)]))),
                  (R.tie_body(), dict(parents=R.CHAIN, radii=QUARTER, mask=R.pair_mask([(1, 5), (2, 5)]), tolerance=0.0))):
        worst = max(worst, compare_host(exe, tmp_path, J, **kw))
    print(f"[selfcontact] host build against the restatement: {worst:.3e} at most (equal expected, bound 1e-12)")


# ---- the twelfth header ------------------------------------------------------------------------------------------------------------------------
def test_the_twelfth_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_selfcontact()
    assert list(abi.functions) == NAMES and L.SELF.functions == abi.functions and L.SELF.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_SELF_LAUNCHES=2, TC_SELF_PAIRS=253, TC_SELF_WS_FRAME=44)
    I, VP, LONG, D = C.c_int, C.c_void_p, C.c_long, C.c_double
    assert abi.functions["tci_self_contact_workspace"][:2] == (I, [I, I, I, VP])
    assert abi.functions["tci_self_contact"][:2] == (I, [VP, VP, I, I, I, VP, VP, VP, D, VP, LONG] + [VP] * 9)
    assert abi.functions["tci_self_contact"][2][:2] == ["const float*", "const long*"]
    assert abi.functions["tci_self_contact"][2][5:8] == ["const int*", "const double*", "const uint64_t*"]
    with open(_abi.HEADER_SELFCONTACT) as f:
        text = f.read()
    flat = " ".join(text.replace("*", " ").split())
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text and "Not built" in text
    assert "choices, not measurements" in flat and "winding number" in flat
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_", "tcj_", "tck_", "tcg_", "tcp_", "tcf_", "tcm_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_selfcontact.h", prefix=prefix)
    others = (L.ABI, L.EXT, L.GLTF, L.SKIN, L.SHADE, L.MJPEG, L.FOOTLOCK, L.GROUP, L.APART, L.GROUND, L.MESH)
    for names in [a.functions for a in others] + [L.EXPORTS]:
        assert not any(n.startswith("tci_") for n in names)
    assert not any(k.startswith("TC_SELF") for a in others for k in a.constants) and len(L.ABI.functions) == 79
    assert S.PAIRS == 253


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    syms = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    assert sorted(s for s in syms if s.startswith("tci_")) == sorted(NAMES)
    assert not [s for s in syms if "self_contact" in s.lower() and not s.startswith("tci_")]
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    n = C.c_long(-1)
    want = 44 * (2 * 3 * 10)
    assert lib.tci_self_contact_workspace(2, 3, 10, C.addressof(n)) == 0 and n.value == want
    assert lib.tci_self_contact_workspace(1, 1, 1, C.addressof(n)) == 0 and n.value == 48          # 44 rounded up to 48
    assert lib.tci_self_contact_workspace(2, 3, 10, None) == -1
    for bad in ((0, 3, 10), (2, 0, 10), (2, 3, 0), (2, 3, -1), (-1, 3, 10)):
        assert lib.tci_self_contact_workspace(*bad, C.addressof(n)) == -1, bad
    assert lib.tci_self_contact_workspace(2 ** 12, 2 ** 8, 2 ** 12, C.addressof(n)) == -4
    assert lib.tci_self_contact_workspace(1, 1, 2 ** 31 - 1, C.addressof(n)) == 0 and n.value == (44 * (2 ** 31 - 1) + 7) // 8 * 8
    parents, radii = (C.c_int * 24)(*SMPL_PARENTS), (C.c_double * 24)(*R.capsule_radii())
    strides = (C.c_long * 3)(2160, 720, 72)
    words = lambda *w: (C.c_uint64 * 4)(*w)
    full = words(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 61 - 1)

    def call(joints=p, strides=strides, b=2, dn=3, T=10, parents=parents, radii=radii, mask=full, tolerance=0.03, ws=p, ws_bytes=want - 1,
             gap=p, closest=p, rate=p, gap_min=p, episodes=p, closest_min=p, depth_mean=p, pair_frames=p):
        return lib.tci_self_contact(joints, strides, b, dn, T, parents, radii, mask, tolerance, ws, ws_bytes, gap, closest, rate, gap_min,
                                    episodes, closest_min, depth_mean, pair_frames, None)
    assert call() == -1                                                    # good arguments but for one byte of workspace
    assert call(ws=p + 4, ws_bytes=want) == -2
    assert call(gap=None, closest=None) == -1                             # these may be NULL: it is the workspace again
    assert call(gap=None, closest=None, ws=p + 4, ws_bytes=want) == -2
    assert call(gap=p + 4, ws_bytes=want) == -2 and call(closest=p + 2, ws_bytes=want) == -2
    assert call(dn=1, ws_bytes=44 * 20 - 1) == -1 and call(dn=1, ws=p + 4, ws_bytes=44 * 20) == -2          # one dancer is legal
    big = 1 << 40
    nan = float("nan")
    for kw in (dict(joints=None), dict(strides=None), dict(parents=None), dict(radii=None), dict(mask=None), dict(ws=None), dict(rate=None),
               dict(gap_min=None), dict(episodes=None), dict(closest_min=None), dict(depth_mean=None), dict(pair_frames=None), dict(b=0),
               dict(dn=0), dict(T=0), dict(T=-3), dict(tolerance=-1e-6), dict(tolerance=nan), dict(tolerance=float("inf")),
               dict(strides=(C.c_long * 3)(2160, -720, 72)), dict(mask=words(0, 0, 0, 0)), dict(mask=words(1, 0, 0, 2 ** 61)),
               dict(mask=words(0, 0, 0, 2 ** 63)), dict(mask=words(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1))):
        assert call(**dict(dict(ws_bytes=big, ws=p + 4), **kw)) == -1, kw          # every one of them precedes the alignment check
    assert call(mask=words(0, 0, 0, 2 ** 60), ws=p + 4, ws_bytes=big) == -2          # pair 252 alone is a mask
    # the order: a bad tolerance before the size, the size before a stride, a parent, a radius and the mask, the mask before the workspace
    assert call(b=2 ** 12, dn=2 ** 8, T=2 ** 12, ws_bytes=big) == -4 and call(b=2 ** 12, dn=2 ** 8, T=2 ** 12, tolerance=-1.0, ws_bytes=big) == -1
    assert call(b=2 ** 12, dn=2 ** 8, T=2 ** 12, mask=words(0, 0, 0, 0), strides=(C.c_long * 3)(-1, 0, 0), ws_bytes=big) == -4
    for j, parent in ((3, 5), (7, 7), (2, -1)):                             # a parent after its child, itself, none
        wrong = list(SMPL_PARENTS)
        wrong[j] = parent
        assert call(parents=(C.c_int * 24)(*wrong), ws_bytes=big, ws=p + 4) == -1, (j, parent)
    for value in (-0.01, nan, float("inf")):
        wrong = list(R.capsule_radii())
        wrong[11] = value
        assert call(radii=(C.c_double * 24)(*wrong), ws_bytes=big, ws=p + 4) == -1, value
    wrong = list(R.capsule_radii())
    wrong[0] = nan                                                         # entry 0 is unused: the call gets as far as the workspace
    assert call(radii=(C.c_double * 24)(*wrong)) == -1 and call(radii=(C.c_double * 24)(*wrong), ws=p + 4, ws_bytes=want) == -2


def test_the_twelfth_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.SELF.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_selfcontact.h"', '#include "tcdiff_selfcontact.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "self.c", tmp_path / "self"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.SELF.constants[n] for n in names]
    calls = ['#include "tcdiff_selfcontact.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.SELF.functions.items():
        assert restype is C.c_int and argtypes == [C.c_void_p if c.endswith("*") else _abi.SCALARS[c] for c in ctexts], fname
        calls.append(f"  {{ int (*f)({', '.join(ctexts)}) = {fname}; (void)f; }}")
        zeros = [f"({c})0" if c.endswith("*") or c == "hipStream_t" else f"({c})z" for c in ctexts]
        calls.append(f"  (void){fname}({', '.join(zeros)});")
    calls.append("}")
    tu = tmp_path / "calls.c"
    tu.write_text("\n".join(calls))
    r = subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-c", str(tu), "-o", str(tmp_path / "calls.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the public interface ----------------------------------------------------------------------------------------------------------------------
def test_self_contact_refuses_before_any_launch():
    import tcdiff_amd
    for name in ("self_contact", "self_pairs", "pair_index", "pair_of", "pair_mask", "evaluate_self_contact"):
        assert getattr(tcdiff_amd, name) is getattr(S, name) and name in tcdiff_amd.__all__
    sig = inspect.signature(S.self_contact).parameters
    assert list(sig) == ["joints", "radii", "parents", "mask", "rest_joints", "hops", "rest_margin", "tolerance", "return_frames"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, None, None, None, 2, 0.05, 0.03, False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[1:])
    sig = inspect.signature(S.self_pairs).parameters
    assert list(sig) == ["radii", "parents", "rest_joints", "hops", "rest_margin"] and [p.default for p in sig.values()] == [None, None, None, 2, 0.05]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in sig.values())
    assert list(inspect.signature(S.evaluate_self_contact).parameters) == ["samples", "normalizer", "dn", "mode", "kw"]
    J = torch.zeros(2, 3, 6, 24, 3)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        S.self_contact(J)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        S.self_contact(J[:, :1], mask=S.pair_mask([(3, 20)]))             # one dancer is legal, and refused off the device as well
    late = list(SMPL_PARENTS)
    late[3] = 5
    for bad in (dict(joints=J[0]), dict(joints=J.double()), dict(joints=J.numpy()), dict(joints=torch.zeros(2, 3, 6, 23, 3)),
                dict(joints=J[:, :, :0]), dict(joints=J[:0]), dict(joints=J[:, :0]), dict(joints=J.transpose(-1, -2).contiguous().transpose(-1, -2)),
                dict(tolerance=-0.01), dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(tolerance=None), dict(tolerance=True),
                dict(radii=np.ones(23)), dict(radii=-np.ones(24)), dict(radii=np.full(24, np.nan)), dict(radii=np.full(24, np.inf)),
                dict(parents=SMPL_PARENTS[:5]), dict(parents=late), dict(mask=np.zeros(253, bool)), dict(mask=np.ones(252, bool)),
                dict(mask=np.ones(253, np.int64)), dict(mask=[(3, 20)]), dict(hops=-1), dict(hops=1.5), dict(rest_margin=float("nan")),
                dict(rest_joints=np.zeros((23, 3))), dict(rest_margin=10.0), dict(hops=99)):          # the last two leave no pair
        kw = dict(joints=J)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match=r"^self_contact: "):          # its own refusal, not "self_contact runs on MI355X only"
            S.self_contact(kw.pop("joints"), **kw)
    for doc in (S.__doc__, S.self_contact.__doc__, S.self_pairs.__doc__):
        assert "choices, not measurements" in " ".join(doc.split())
    flat = " ".join(S.__doc__.split())
    assert "unpinned" in flat and "Not built" in flat and "winding number" in flat and "bending an arm to dodge" in flat
    for name in ("group_metrics", "apart", "mesh_contact"):             # the three that used to list it as not built
        doc = " ".join(importlib.import_module("tcdiff_amd." + name).__doc__.split())
        assert "self_contact" in doc, name


# ---- what the GPU comparison rests on ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_decision_is_a_near_tie_on_the_seeded_scenes(shape):
    ok, why = R.decisions_clear(R.synth(*shape), radii=R.scene_radii())
    assert ok, why


def test_no_decision_is_a_near_tie_with_other_parameters():
    for shape, seed, kw in R.parameter_cases():
        ok, why = R.decisions_clear(R.synth(*shape, seed=seed), **kw)
        assert ok, (sorted(kw), why)


def test_the_default_radii_scene_stays_under_its_cap():
    """with the default radii exact ties are expected (equal radii on bones that share a joint); the GPU test leaves `closest` out in
    the frames whose lead is <= 1e-9, at most a tenth of them"""
    shape, seed = R.DEFAULT_RADII_SCENE
    ref = R.self_contact(R.synth(*shape, seed=seed), details=True)
    lead = ref["details"]["frame_lead"]
    assert 0.0 < float((lead <= R.MARGIN).mean()) <= 0.10
    assert ref["details"]["tolerance_lead"] > R.MARGIN and ref["details"]["dancer_lead"] > R.MARGIN


def test_the_seeded_scenes_are_not_trivial():
    refs = [R.self_contact(R.synth(*shape), radii=R.scene_radii()) for shape in R.SHAPES]
    cat = lambda key: np.concatenate([r[key].reshape(-1) for r in refs])
    rate, episodes = cat("self_contact_rate"), cat("self_contact_episodes")
    assert ((rate > 0) & (rate < 1)).any() and (rate == 0).any() and (episodes >= 2).any()
    assert (cat("self_gap_min") < -0.03).any() and (cat("self_gap_min") > -0.03).any()
    frames = sum(r["self_pair_frames"].reshape(-1, 253).sum(0) for r in refs)
    assert (frames > 0).sum() >= 10 and not frames[~R.self_pairs(radii=R.scene_radii())].any()
    limbs = {R.PAIRS[int(k)] for k in np.flatnonzero(frames)}
    assert any(j in (18, 19, 20, 21, 22, 23) and i in (3, 6, 9, 15, 1, 2, 4, 5) for i, j in limbs)          # an arm through the trunk, the head or a leg
    for shape in R.SHAPES:
        J = R.synth(*shape)
        bone = np.linalg.norm(J[..., 1:, :] - J[..., R.SMPL_PARENTS[1:], :], axis=-1)
        assert np.allclose(bone, np.linalg.norm(R.OFFSETS[1:], axis=-1), atol=1e-5)          # FK poses: every bone keeps its length
