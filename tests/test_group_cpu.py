"""CPU checks of the group metrics (no GPU): the numpy restatement tests/group_ref.py of include/tcdiff_group.h on cases that can be
checked by hand, the eighth header and its binding, the launchers' refusals, csrc/group_math.h built for the host as a stand-alone
program with the address and undefined-behaviour sanitizers against the restatement, radii_from_body, and the conditions the GPU
comparison rests on: on the seeded inputs no decision of the metrics is a near-tie, and the inputs are not trivial."""
import ctypes as C
import importlib
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import group_ref as R
from group_ref import clip, point_dancer, stepper, stick_dancer
import skin_ref
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd.body import load_body_model
from tcdiff_amd.fk import SMPL_PARENTS

G = importlib.import_module("tcdiff_amd.group_metrics")          # the package's attribute of this name is the function
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcg_group_workspace", "tcg_group_metrics"]
RADII = R.capsule_radii()


# ---- 1. the body gap --------------------------------------------------------------------------------------------------------------------------
def test_two_upright_parallel_bodies_are_their_distance_less_two_radii_apart():
    D = 0.75
    ref = R.group_metrics(clip(stick_dancer(0.0), stick_dancer(D)), radii=np.full(24, 0.125))
    assert ref["gap"][0, 0, 0] == D - 0.25 and ref["body_gap_min"][0, 0] == 0.5
    assert ref["closest"][0, 0, 0] == 24 * 1 + 1                       # every bone pair at a common height ties: the smallest code
    assert ref["body_contact_rate"][0, 0] == 0.0 and ref["body_contact_episodes"][0, 0] == 0
    assert ref["body_closest"][0, 0].tolist() == [0, 1, 1]
    ref = R.group_metrics(clip(stick_dancer(0.0), stick_dancer(D)))    # the default table: the spines, 0.13 each, are the thickest
    assert ref["gap"][0, 0, 0] == (D - 0.13) - 0.13 and ref["closest"][0, 0, 0] == 24 * 3 + 3
    near = R.group_metrics(clip(stick_dancer(0.0), stick_dancer(0.25)))
    assert near["gap"][0, 0, 0] == (0.25 - 0.13) - 0.13 < 0 and near["body_contact_rate"][0, 0] == 1.0
    assert near["body_contact_episodes"][0, 0] == 1


def test_two_crossed_forearms_penetrate_by_both_radii():
    a, b = point_dancer((0, 0, 100)), point_dancer((0, 0, -100))
    a[0, 18], a[0, 20] = (-1, 0, 0), (1, 0, 0)                          # bone 20 of a: left elbow -> left wrist
    b[0, 19], b[0, 21] = (0, -1, 0), (0, 1, 0)                          # bone 21 of b: right elbow -> right wrist; an X at the origin
    ref = R.group_metrics(clip(a, b))
    assert ref["gap"][0, 0, 0] == -(RADII[20] + RADII[21]) == -0.08 and ref["closest"][0, 0, 0] == 24 * 20 + 21
    assert ref["body_closest"][0, 0].tolist() == [0, 20, 21] and ref["body_contact_rate"][0, 0] == 1.0


def test_zero_length_bones_take_their_branches():
    p, q = np.array([0.0, 0.0, 0.0]), np.array([2.0, 0.0, 0.0])
    x = np.array([1.0, 3.0, 0.0])
    assert R.seg_dist(p, p, x, x) == np.sqrt(10.0)                     # both small: two points
    assert R.seg_dist(x, x, p, q) == 3.0 and R.seg_dist(p, q, x, x) == 3.0          # one small: a point and a segment, either order
    far = np.array([5.0, 4.0, 0.0])
    assert R.seg_dist(far, far, p, q) == 5.0 and R.seg_dist(p, q, far, far) == 5.0  # clamped to the end
    assert R.seg_dist(p, q, p + [0, 1, 0], q + [0, 1, 0]) == 1.0                    # parallel: den = 0
    assert R.seg_dist(p, q, [1, -1, 1], [1, 1, 1]) == 1.0                           # skew, both interior
    assert R.seg_dist(p, q, [3, 1, 0], [3, 5, 0]) == np.sqrt(2.0)                   # end to end
    ref = R.group_metrics(clip(point_dancer((0, 0, 0)), point_dancer((3, 4, 0))))
    assert ref["gap"][0, 0, 0] == (5.0 - 0.13) - 0.13 and ref["closest"][0, 0, 0] == 24 * 3 + 3


def test_episodes_the_minimum_and_a_nan_joint():
    xs = [1.0, 0.25, 0.25, 1.0, 0.125, 1.0, 0.25, 1.0]                  # contact on frames 1-2, 4, 6: three episodes
    a = stick_dancer(0.0, T=8)
    b = np.concatenate([stick_dancer(x) for x in xs])
    ref = R.group_metrics(clip(a, b))
    assert ref["body_contact_episodes"][0, 0] == 3 and ref["body_contact_rate"][0, 0] == 0.5
    assert ref["body_gap_min"][0, 0] == (0.125 - 0.13) - 0.13 and ref["body_closest"][0, 0].tolist() == [4, 3, 3]
    b2 = b.copy()
    b2[4] = b2[2]                                                       # frames 1, 2, 4 and 6 now tie: the first frame wins
    assert R.group_metrics(clip(a, b2))["body_closest"][0, 0].tolist() == [1, 3, 3]
    b[4, 7, 1] = np.nan                                                 # the deepest frame loses a joint: it is skipped, not a contact
    ref = R.group_metrics(clip(a, b))
    assert np.isnan(ref["gap"][0, 0, 4]) and ref["closest"][0, 0, 4] == 24 * 1 + 7 and np.isfinite(np.delete(ref["gap"][0, 0], 4)).all()
    assert ref["body_contact_episodes"][0, 0] == 2 and ref["body_contact_rate"][0, 0] == 3 / 8
    assert ref["body_closest"][0, 0].tolist() == [1, 3, 3] and ref["body_gap_min"][0, 0] == (0.25 - 0.13) - 0.13
    b[:, 7, 1] = np.nan
    ref = R.group_metrics(clip(a, b))
    assert np.isnan(ref["body_gap_min"][0, 0]) and ref["body_closest"][0, 0].tolist() == [-1, -1, -1]
    assert ref["body_contact_rate"][0, 0] == 0.0 and ref["body_contact_episodes"][0, 0] == 0


# ---- 2. crossings -----------------------------------------------------------------------------------------------------------------------------
def walker(points):
    """a point dancer whose root visits the floor points (x, y), one a frame, at height 1"""
    J = np.zeros((len(points), 24, 3), np.float32)
    J[:, :, :2] = np.asarray(points, np.float32)[:, None, :]
    J[:, :, 2] = 1.0
    return J


def test_an_x_of_two_paths_is_one_crossing_inside_the_window():
    line = [(-1 + 2 * k / 7, -1 + 2 * k / 7) for k in range(8)]         # the centre lies inside step 3
    a = walker(line + [line[-1]] * 2)
    b = walker([(line[0][0], -line[0][1])] * 2 + [(x, -y) for x, y in line])          # the other diagonal, two frames later: step 5
    for window, want in ((0, 0), (1, 0), (2, 1), (30, 1)):
        ref = R.group_metrics(clip(a, b), window=window)
        assert ref["path_crossings"][0, 0] == want and ref["path_crossing_rate"][0, 0] == want / 9, window
    assert R.crossings_of(R.floor_of(a, 2), R.floor_of(b, 2), 5) == [(3, 5)]
    same = walker([(x, -y) for x, y in line] + [line[-1]] * 2)          # at the same time: they swap places within one frame
    assert R.group_metrics(clip(a, same), window=0)["path_crossings"][0, 0] == 1
    for up, axes in ((0, (1, 2)), (1, (0, 2))):                         # the same walk with another axis up
        moved = []
        for J in (a, b):
            K = np.ones_like(J)
            K[:, :, axes[0]], K[:, :, axes[1]] = J[:, :, 0], J[:, :, 1]
            moved.append(K)
        assert R.group_metrics(clip(*moved), up=up, window=2)["path_crossings"][0, 0] == 1
        assert R.group_metrics(clip(*moved), up=2, window=2)["path_crossings"][0, 0] == 0


def test_touching_end_points_and_a_standing_dancer_are_no_crossings():
    a = walker([(-1, 0), (0, 0), (0, 0), (1, 0)])                        # stops ON b's line, stands, walks on
    b = walker([(0, -1), (0, 1), (0, 2), (0, 3)])
    assert R.group_metrics(clip(a, b), window=30)["path_crossings"][0, 0] == 0
    corner = walker([(0, 0), (1, 1), (2, 0), (3, 1)])                   # the two paths share their first point
    other = walker([(0, 0), (-1, 1), (-2, 0), (-3, 1)])
    assert R.group_metrics(clip(corner, other), window=30)["path_crossings"][0, 0] == 0
    stand = walker([(0.5, 0.5)] * 4)                                    # standing in the middle of the other's step
    ref = R.group_metrics(clip(corner, stand), window=30)
    assert ref["path_crossings"][0, 0] == 0 and ref["path_crossing_rate"][0, 0] == 0.0
    assert R.group_metrics(clip(corner[:1], other[:1]))["path_crossing_rate"][0, 0] == 0.0          # T = 1: no step


# ---- 3. synchrony -----------------------------------------------------------------------------------------------------------------------------
def two_speed(N, k, seed=5):
    """speeds of 1/64 and 3/64 in a seeded balanced order: S over [-k, N), its first k entries a copy of its last k"""
    g = np.random.default_rng(seed)
    s = g.permutation(np.repeat([1 / 64, 3 / 64], N // 2))
    return np.concatenate([s[N - k:], s])


@pytest.mark.parametrize("k", [1, 3, 7])
def test_an_exact_delayed_copy_is_in_step_at_its_delay(k):
    N = 40
    S = two_speed(N, k)
    a, b = stepper(S[k:]), stepper(S[:N])                               # b does at t + k what a did at t: b trails a
    ref = R.group_metrics(clip(a, b))
    assert ref["sync"][0, 0] == 1.0 and ref["sync_lag"][0, 0] == k and ref["sync_zero"][0, 0] < 0.9
    swapped = R.group_metrics(clip(b, a))
    assert swapped["sync"][0, 0] == 1.0 and swapped["sync_lag"][0, 0] == -k
    assert R.group_metrics(clip(a, b), max_lag=k - 1)["sync"][0, 0] < 1.0          # the delay lies outside the range


def test_a_motionless_dancer_and_short_clips_have_no_synchrony():
    a = stepper(two_speed(40, 1)[1:])
    still = stick_dancer(3.0, T=41)
    ref = R.group_metrics(clip(a, still))
    assert np.isnan(ref["sync"][0, 0]) and np.isnan(ref["sync_zero"][0, 0]) and ref["sync_lag"][0, 0] == 0
    for T in (1, 2):                                                    # T < 3: no lag has two terms
        ref = R.group_metrics(clip(a[:T], a[:T] + np.float32(1.0)))
        assert np.isnan(ref["sync"][0, 0]) and np.isnan(ref["sync_zero"][0, 0]) and ref["sync_lag"][0, 0] == 0
    ref = R.group_metrics(clip(a[:3], a[:3] + np.float32(1.0)))         # T = 3: lag 0 alone, two terms
    assert R.lag_range(3, 15) == 0 and ref["sync_lag"][0, 0] == 0 and np.array_equal(ref["sync"], ref["sync_zero"], equal_nan=True)


def test_the_tie_rules_of_the_lag():
    beat = np.tile([1 / 64, 3 / 64], 20)                                 # z = -1, +1, -1, ...: R is exactly 1 at every even lag
    ref = R.group_metrics(clip(stepper(beat), stepper(beat)))
    assert ref["sync"][0, 0] == 1.0 and ref["sync_lag"][0, 0] == 0 and ref["sync_zero"][0, 0] == 1.0
    ref = R.group_metrics(clip(stepper(beat), stepper(beat[::-1])))      # half a period apart: 1 at every odd lag, -1 and +1 tie
    assert ref["sync"][0, 0] == 1.0 and ref["sync_lag"][0, 0] == -1 and ref["sync_zero"][0, 0] == -1.0
    assert R.better_lag(1.0, -1, 1.0, 1) and not R.better_lag(1.0, 1, 1.0, -1) and R.better_lag(1.0, 1, 1.0, -2)
    assert R.better_lag(1.0, 5, 0.5, 0) and not R.better_lag(0.5, 0, 1.0, 5)


def test_formation_travel_does_not_swamp_the_limbs():
    """both dancers travel together and only their hands move, in step: the root's speed is constant (sigma 0: left out) and the
    hands' root-relative speeds carry the score"""
    N, k = 40, 2
    S = two_speed(N, k)
    a, b = stepper(np.full(N, 1 / 8)), stepper(np.full(N, 1 / 8))
    a[:, 22, 2] += np.concatenate([[0.0], np.cumsum(S[k:])]).astype(np.float32)
    b[:, 22, 2] += np.concatenate([[0.0], np.cumsum(S[:N])]).astype(np.float32)
    ref = R.group_metrics(clip(a, b + np.float32(4.0)))
    assert ref["sync"][0, 0] == 1.0 and ref["sync_lag"][0, 0] == k


# ---- csrc/group_math.h on the host, under the sanitizers ---------------------------------------------------------------------------------------
def run_host(exe, tmp, J, up=2, window=30, max_lag=15, sigma_floor=1e-6, radii=None, parents=None):
    dn, T = J.shape[:2]
    radii = RADII if radii is None else radii
    parents = SMPL_PARENTS if parents is None else parents
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([dn, T, up, window, max_lag], np.int32).tobytes() + np.array([sigma_floor] + list(radii), np.float64).tobytes() +
                np.array(parents, np.int32).tobytes() + np.ascontiguousarray(J, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.frombuffer((tmp / "out.bin").read_bytes(), np.float64)
    P = dn * (dn - 1) // 2
    return raw.reshape(P, 2 * T + 4)


def compare_host(out, ref, T):
    worst = 0.0
    for p in range(out.shape[0]):
        gap, code, (cross, sync, lag, zero) = out[p, :T], out[p, T:2 * T], out[p, 2 * T:]
        assert np.array_equal(np.isnan(gap), np.isnan(ref["gap"][0, p])) and np.array_equal(code, ref["closest"][0, p])
        assert cross == ref["path_crossings"][0, p] and lag == ref["sync_lag"][0, p]
        for mine, theirs in ((gap, ref["gap"][0, p]), (np.array([sync, zero]), np.array([ref["sync"][0, p], ref["sync_zero"][0, p]]))):
            assert np.array_equal(np.isnan(mine), np.isnan(theirs))
            if (~np.isnan(theirs)).any():
                worst = max(worst, float(np.nanmax(np.abs(mine - theirs))))
    assert worst <= 1e-12, worst
    return worst


def test_group_math_on_the_host_under_the_sanitizers_agrees_with_the_restatement(tmp_path):
    """the SAME functions the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "group_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "group_host.cpp")])
    worst = 0.0
    for shape in [(1, 2, 1), (1, 2, 2), (1, 2, 3), (2, 3, 5), (1, 5, 70)]:
        J = R.synth(*shape)
        for c in range(shape[0]):
            worst = max(worst, compare_host(run_host(exe, tmp_path, J[c]), R.group_metrics(J[c:c + 1]), shape[2]))
    for shape, kw in R.parameter_cases():
        J = R.synth(*shape)
        args = dict(kw)
        fps = args.pop("fps", 30)                                          # the kernels never see it: it is the default window
        args.setdefault("window", int(round(fps)))
        worst = max(worst, compare_host(run_host(exe, tmp_path, J[0], **args), R.group_metrics(J, **kw), shape[2]))
    a, b = point_dancer((0, 0, 100)), point_dancer((0, 0, -100))       # zero-length bones, an exact tie and a NaN joint
    a[0, 18], a[0, 20], b[0, 19], b[0, 21] = (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)
    for J in (np.stack([a, b]), np.stack([stick_dancer(0.0), stick_dancer(0.75)]), np.stack([a, np.where(np.arange(24)[None, :, None] == 7, np.nan, b)])):
        J = J.astype(np.float32)
        worst = max(worst, compare_host(run_host(exe, tmp_path, J), R.group_metrics(J[None]), 1))
    print(f"[group] host build against the restatement: {worst:.3e} at most (bound 1e-12)")


# ---- the eighth header -------------------------------------------------------------------------------------------------------------------------
def test_the_eighth_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_group()
    assert list(abi.functions) == NAMES and L.GROUP.functions == abi.functions and L.GROUP.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_GROUP_LAUNCHES=3, TC_GROUP_MAX_LAG=64, TC_GROUP_WS_PAIR_FRAME=12, TC_GROUP_WS_DANCER_FRAME=192,
                                 TC_GROUP_WS_DANCER=192)
    I, VP, LONG, D = C.c_int, C.c_void_p, C.c_long, C.c_double
    assert abi.functions["tcg_group_workspace"][:2] == (I, [I, I, I, I, VP])
    assert abi.functions["tcg_group_metrics"][:2] == (I, [VP, VP, I, I, I, I, D, VP, VP, I, I, D, VP, LONG] + [VP] * 12)
    assert abi.functions["tcg_group_metrics"][2][:2] == ["const float*", "const long*"]
    with open(_abi.HEADER_GROUP) as f:
        text = f.read()
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text and "Not built" in text and "GMR" in text
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_", "tcj_", "tck_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_group.h", prefix=prefix)
    for names in (L.ABI.functions, L.EXT.functions, L.GLTF.functions, L.SKIN.functions, L.SHADE.functions, L.MJPEG.functions,
                  L.FOOTLOCK.functions, L.EXPORTS):
        assert not any(n.startswith("tcg_") for n in names)
    frozen = {**L.ABI.constants, **L.EXT.constants, **L.GLTF.constants, **L.SKIN.constants, **L.SHADE.constants, **L.MJPEG.constants,
              **L.FOOTLOCK.constants}
    assert not any(k.startswith("TC_GROUP") for k in frozen) and len(L.ABI.functions) == 79
    assert G.MAX_LAG == 64


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    syms = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    assert sorted(s for s in syms if s.startswith("tcg_")) == sorted(NAMES)
    assert not [s for s in syms if "group_metrics" in s.lower() and s.split("_")[0] in ("tcdiff", "tcx", "tcs", "tcr", "tcj", "tck")]
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    n = C.c_long(-1)
    want = 12 * (2 * 3 * 10) + 192 * (2 * 3 * 10) + 192 * (2 * 3)
    assert lib.tcg_group_workspace(2, 3, 10, 15, C.addressof(n)) == 0 and n.value == want
    assert lib.tcg_group_workspace(1, 2, 1, 0, C.addressof(n)) == 0 and n.value == 16 + 384 + 384          # 12 rounded up to 16
    assert lib.tcg_group_workspace(2, 3, 10, 15, None) == -1
    for bad in ((0, 3, 10, 15), (2, 0, 10, 15), (2, 1, 10, 15), (2, 3, 0, 15), (2, 3, -1, 15), (2, 3, 10, -1), (2, 3, 10, 65)):
        assert lib.tcg_group_workspace(*bad, C.addressof(n)) == -1, bad
    assert lib.tcg_group_workspace(2 ** 12, 2 ** 6, 2 ** 12, 15, C.addressof(n)) == -4
    parents, radii = (C.c_int * 24)(*SMPL_PARENTS), (C.c_double * 24)(*RADII)
    strides = (C.c_long * 3)(2160, 720, 72)

    def call(joints=p, strides=strides, b=2, dn=3, T=10, up=2, fps=30.0, parents=parents, radii=radii, window=30, max_lag=15,
             sigma_floor=1e-6, ws=p, ws_bytes=want - 1, gap=p, closest=p, rate=p, gap_min=p, episodes=p, closest_min=p, crossings=p,
             crossing_rate=p, sync=p, sync_lag=p, sync_zero=p):
        return lib.tcg_group_metrics(joints, strides, b, dn, T, up, fps, parents, radii, window, max_lag, sigma_floor, ws, ws_bytes, gap,
                                     closest, rate, gap_min, episodes, closest_min, crossings, crossing_rate, sync, sync_lag, sync_zero, None)
    assert call() == -1                                                    # good arguments but for one byte of workspace
    assert call(ws=p + 4, ws_bytes=want) == -2
    assert call(gap=None, closest=None) == -1                             # these may be NULL: it is the workspace again
    assert call(gap=None, closest=None, ws=p + 4, ws_bytes=want) == -2
    assert call(gap=p + 4, ws_bytes=want) == -2 and call(closest=p + 2, ws_bytes=want) == -2
    big = 1 << 40
    nan = float("nan")
    for kw in (dict(joints=None), dict(strides=None), dict(parents=None), dict(radii=None), dict(ws=None), dict(rate=None), dict(gap_min=None),
               dict(episodes=None), dict(closest_min=None), dict(crossings=None), dict(crossing_rate=None), dict(sync=None),
               dict(sync_lag=None), dict(sync_zero=None), dict(b=0), dict(dn=0), dict(dn=1), dict(T=0), dict(T=-3), dict(up=-1), dict(up=3),
               dict(fps=0.0), dict(fps=-30.0), dict(fps=nan), dict(window=-1), dict(max_lag=-1), dict(max_lag=65), dict(sigma_floor=-1e-6),
               dict(sigma_floor=nan), dict(strides=(C.c_long * 3)(2160, -720, 72))):
        assert call(ws_bytes=big, **kw) == -1, kw
    assert call(b=2 ** 12, dn=2 ** 6, T=2 ** 12, ws_bytes=big) == -4
    for j, parent in ((3, 5), (7, 7), (2, -1)):                             # a parent after its child, itself, none
        wrong = list(SMPL_PARENTS)
        wrong[j] = parent
        assert call(parents=(C.c_int * 24)(*wrong), ws_bytes=big) == -1, (j, parent)
    for value in (-0.01, nan, float("inf")):
        wrong = list(RADII)
        wrong[11] = value
        assert call(radii=(C.c_double * 24)(*wrong), ws_bytes=big) == -1, value
    wrong = list(RADII)
    wrong[0] = nan                                                         # entry 0 is unused: the call gets as far as the workspace
    assert call(radii=(C.c_double * 24)(*wrong)) == -1 and call(radii=(C.c_double * 24)(*wrong), ws=p + 4, ws_bytes=want) == -2


def test_the_eighth_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.GROUP.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_group.h"', '#include "tcdiff_group.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "group.c", tmp_path / "group"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.GROUP.constants[n] for n in names]
    calls = ['#include "tcdiff_group.h"', '#include "tcdiff_group.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.GROUP.functions.items():
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
def test_group_metrics_refuses_before_any_launch():
    import tcdiff_amd
    for name in ("group_metrics", "pairs", "capsule_radii", "radii_from_body", "evaluate_group"):
        assert getattr(tcdiff_amd, name) is getattr(G, name) and name in tcdiff_amd.__all__
    sig = inspect.signature(G.group_metrics).parameters
    assert list(sig) == ["joints", "fps", "up", "radii", "parents", "window", "max_lag", "sigma_floor", "return_frames"]
    assert [sig[k].default for k in list(sig)[1:]] == [30, 2, None, None, None, 15, 1e-6, False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[1:])
    assert list(inspect.signature(G.evaluate_group).parameters) == ["samples", "normalizer", "dn", "mode", "kw"]
    J = torch.zeros(2, 3, 6, 24, 3)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        G.group_metrics(J)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        G.group_metrics(J[:, :1])                                      # one dancer is refused off the device as well
    late = list(SMPL_PARENTS)
    late[3] = 5
    for bad in (dict(joints=J[0]), dict(joints=J.double()), dict(joints=J.numpy()), dict(joints=torch.zeros(2, 3, 6, 23, 3)),
                dict(joints=J[:, :, :0]), dict(joints=J[:0]), dict(joints=J.transpose(-1, -2).contiguous().transpose(-1, -2)), dict(up=3),
                dict(up=-1), dict(up=True), dict(fps=0), dict(fps=-30), dict(fps=float("nan")), dict(fps="30"), dict(window=-1),
                dict(window=1.5), dict(max_lag=-1), dict(max_lag=65), dict(max_lag=2.0), dict(sigma_floor=-1.0),
                dict(sigma_floor=float("nan")), dict(sigma_floor=None), dict(radii=np.ones(23)), dict(radii=-np.ones(24)),
                dict(radii=np.full(24, np.nan)), dict(radii=np.full(24, np.inf)), dict(parents=SMPL_PARENTS[:5]), dict(parents=late)):
        kw = dict(joints=J)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match="group_metrics"):
            G.group_metrics(kw.pop("joints"), **kw)
    for doc in (G.__doc__, G.group_metrics.__doc__):
        assert "choices, not measurements" in " ".join(doc.split())
    assert "unpinned" in G.__doc__ and "Not built" in G.__doc__ and "GMR" in G.__doc__


def test_pairs_and_the_default_radii():
    assert G.pairs(1) == [] and G.pairs(2) == [(0, 1)] and G.pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert all(len(G.pairs(dn)) == dn * (dn - 1) // 2 and G.pairs(dn) == R.pairs(dn) for dn in range(1, 7))
    for bad in (0, -1, 2.0, True, "3"):
        with pytest.raises(L.TcdiffError, match="pairs"):
            G.pairs(bad)
    r = G.capsule_radii()
    assert r.dtype == np.float64 and r.shape == (24,) and r[0] == 0.0 and np.array_equal(r, RADII)
    want = {0.10: (1, 2, 15), 0.075: (4, 5), 0.05: (7, 8), 0.04: (10, 11, 20, 21), 0.13: (3, 6, 9), 0.06: (12, 16, 17), 0.07: (13, 14),
            0.045: (18, 19), 0.035: (22, 23)}
    assert sorted(j for bones in want.values() for j in bones) == list(range(1, 24))
    assert all(r[j] == value for value, bones in want.items() for j in bones)
    r[3] = 9.0
    assert G.capsule_radii()[3] == 0.13                                 # a fresh table every call


def test_radii_from_a_body_model():
    model = skin_ref.make_model(400, 3, seed=2, smpl_tree=True)
    body = load_body_model(model)
    got = G.radii_from_body(body)
    want = R.radii_from_body(body.v_shaped, body.J, body.weights, body.parents)
    assert got.dtype == np.float64 and got.shape == (24,) and got[0] == 0.0
    assert np.allclose(got, want, rtol=1e-12, atol=0) and (got[1:] > 0).all() and not np.array_equal(got, RADII)
    # a body whose vertices all follow the left wrist: only the bones at that joint are measured, the others keep the table's value
    w = np.zeros((400, 24))
    w[:, 20] = 1.0
    body = load_body_model(dict(model, weights=w))
    got = G.radii_from_body(body)
    d20 = [G._point_segment(v, body.J[18], body.J[20]) for v in body.v_shaped]          # the two bones at joint 20: 18 -> 20 and 20 -> 22
    d22 = [G._point_segment(v, body.J[20], body.J[22]) for v in body.v_shaped]
    assert got[20] == pytest.approx(np.median([x for x, y in zip(d20, d22) if x <= y]), rel=1e-12)
    assert got[22] == pytest.approx(np.median([y for x, y in zip(d20, d22) if y < x]), rel=1e-12)
    assert all(got[j] == RADII[j] for j in range(1, 24) if j not in (20, 22))
    with pytest.raises(L.TcdiffError, match="radii_from_body"):
        G.radii_from_body(model)


# ---- what the GPU comparison rests on ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_decision_is_a_near_tie_on_the_seeded_inputs(shape):
    ok, why = R.decisions_clear(R.synth(*shape))
    assert ok, why


def test_no_decision_is_a_near_tie_with_other_parameters():
    for shape, kw in R.parameter_cases():
        ok, why = R.decisions_clear(R.synth(*shape), **kw)
        assert ok, (kw, why)


def test_the_seeded_inputs_are_not_trivial():
    refs = [R.group_metrics(R.synth(*shape)) for shape in R.SHAPES]
    cat = lambda key: np.concatenate([r[key].reshape(-1) for r in refs])
    rate, episodes, crossings, lag, sync = (cat(k) for k in ("body_contact_rate", "body_contact_episodes", "path_crossings", "sync_lag", "sync"))
    assert ((rate > 0) & (rate < 1)).any() and (episodes >= 2).any() and (crossings > 0).any() and (lag != 0).any()
    assert np.isnan(sync).any() and (sync[~np.isnan(sync)] > 0.8).any()
    assert (cat("body_gap_min") < 0).any() and (cat("body_gap_min") > 0).any()
    for shape in R.SHAPES:                                              # the delayed copy is found at its delay, and b trails a
        if shape[2] >= 70:
            r = R.group_metrics(R.synth(*shape))
            assert (r["sync_lag"][:, 0] == R.DELAY).all() and (r["sync"][:, 0] > 0.8).all()
        J = R.synth(*shape)
        if shape[1] >= 3:
            assert (J[:, -1] == J[:, -1, :1]).all()                       # the last dancer stands still, to the bit
        spine = J[..., [3, 6, 9], :].astype(np.float64) - J[..., [0], :].astype(np.float64)
        bend = np.linalg.norm(np.cross(spine[..., 0, :], spine[..., 2, :]), axis=-1)
        assert bend.max() < 1e-6                                          # the straight spine of synth's docstring
