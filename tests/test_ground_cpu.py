"""CPU checks of putting the dancers on the floor (no GPU): the numpy restatement tests/ground_ref.py of include/tcdiff_ground.h on
cases that can be checked by hand and on what the construction is for, the tenth header and its binding, the launchers' refusals,
render_sample's hook, and the condition the GPU comparison rests on: on the seeded inputs no decision is a near-tie."""
import ctypes as C
import importlib
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ground_ref as R
import group_ref as G
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd.fk import SMPL_PARENTS

P = importlib.import_module("tcdiff_amd.ground")          # the module: the package's attribute `ground` is the function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcf_ground_workspace", "tcf_ground_metrics", "tcf_ground"]
EVEN = np.full(24, 1 / 32)                                   # every capsule 1/32 m: the lows are exact in float32 and float64


def stick(T, depth=0.0):
    """an upright body whose ankles are its lowest joints, at -depth, the toes 1/16 above them, everything else 1/4 m and more up;
    with EVEN radii L = lo_l = lo_r = -depth - 1/32 exactly"""
    J = np.zeros((T, 24, 3), np.float32)
    J[:, :, 0] = np.arange(24, dtype=np.float32) / 64
    J[:, :, 2] = np.float32(0.25) + np.arange(24, dtype=np.float32) / 8 - np.float32(depth)
    J[:, [7, 8], 2] = np.float32(-depth)
    J[:, [10, 11], 2] = np.float32(1 / 16 - depth)
    return J


def run(J, contacts=None, **kw):
    J = np.ascontiguousarray(J, np.float32)
    b, dn, T = J.shape[:3]
    pos = np.ascontiguousarray(np.moveaxis(J[:, :, :, 0], 1, 2).reshape(b, T * dn, 3))
    return R.ground(pos, J, contacts, details=True, **kw)


def all_planted(b, dn, T):
    c = np.zeros((b, dn, T, 4), np.float32)
    c[..., :2] = 1.0
    return c


def cases():
    """every seeded shape with every variant: (name, pos, joints, contacts or None, floor)"""
    for shape in R.SHAPES:
        pos, J, Cn = R.seeded(*shape)
        for name, with_contacts, floor in R.variants():
            yield f"{shape} {name}", pos, J, Cn if with_contacts else None, floor


_refs = {}


def reference(name, pos, J, Cn, floor):
    if name not in _refs:
        _refs[name] = R.ground(pos, J, Cn, floor=floor, details=True)
    return _refs[name]


# ---- cases that can be checked by hand -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3 / 64, -1 / 16], ids=["sunk", "floating"])
def test_a_uniformly_sunk_dancer_planted_throughout_moves_by_exactly_its_depth(depth):
    T = 9
    J = np.stack([stick(T, depth), stick(T, 0.0)])[None]
    out = run(J, all_planted(1, 2, T), floor=-1 / 32, radii=EVEN)
    assert (out["shift"][0, 0] == depth).all() and (out["shift"][0, 1] == 0).all() and out["floor"].tolist() == [-1 / 32]
    assert np.array_equal(out["joints"][0, 0, ..., 2], J[0, 0, ..., 2] + np.float32(depth))
    assert np.array_equal(out["joints"][..., :2].view(np.uint32), J[..., :2].view(np.uint32))          # x and y keep their words
    assert np.array_equal(out["joints"][0, 1].view(np.uint32), J[0, 1].view(np.uint32))
    assert out["before"]["penetration_frames"].tolist() == [[T if depth > 0 else 0, 0]]
    assert out["before"]["float_frames"].tolist() == [[0 if depth > 0 else T, 0]]
    for k in ("penetration_frames", "float_frames"):
        assert out["after"][k].tolist() == [[0, 0]], k
    assert out["after"]["penetration_max"].tolist() == [[0.0, 0.0]] and out["after"]["float_mean"].tolist() == [[0.0, 0.0]]
    assert out["before"]["penetration_max"][0, 0] == max(depth, 0.0) and out["max_shift"][0, 0] == abs(depth) and out["max_step"][0, 0] == 0
    # estimated: the median of the two dancers' feet is halfway between them, and each moves by half its difference
    est = run(J, all_planted(1, 2, T), radii=EVEN)
    assert est["floor"][0] == -1 / 32 - depth / 2 and (est["shift"][0, 0] == depth / 2).all() and (est["shift"][0, 1] == -depth / 2).all()


def test_runs_are_bridged_or_faded_and_the_lift_covers_a_dip():
    T, blend = 40, 3
    J = stick(T)[None, None].copy()
    c = np.zeros((1, 1, T, 4), np.float32)
    c[0, 0, 0:5, 0] = c[0, 0, 11:15, 2] = c[0, 0, 30:34, 1] = 1.0          # gaps of 6 = 2 blend (bridged) and 15 (faded)
    J[0, 0, 0:5, :, 2] -= np.float32(1 / 16)                           # the first run sunk by 1/16, the second by 1/8: B = 1/16 and 1/8
    J[0, 0, 11:30, :, 2] -= np.float32(1 / 8)                          # and the faded gap after it as deep as the second run
    J[0, 0, 5:11, :, 2] += np.float32(1.0)                             # the bridged gap well above the floor: no excess there
    out = run(J, c, floor=-1 / 32, radii=EVEN, blend=blend)
    B = out["planes"]["B"][0, 0]
    assert (B[0:5] == 1 / 16).all() and (B[11:15] == 1 / 8).all() and (B[30:34] == 0).all()
    assert np.array_equal(B[5:11], [1 / 16 + (1 / 8 - 1 / 16) * ((t - 4) / 7) for t in range(5, 11)])          # the bridge
    assert np.array_equal(B[15:19], [1 / 8 * (1 - k / 4) for k in range(1, 4)] + [0.0])                        # the fade
    assert (B[19:30] == 0).all() and (out["planes"]["U"][0, 0, 5:11] == 0).all()
    # frames 15 .. 17 fade from 1/8 while the body stays 1/8 down: the excess is lifted, spread over blend frames to either side
    e = np.zeros(T)
    e[15:30] = 1 / 8 - B[15:30]
    assert np.array_equal(out["planes"]["U"][0, 0], R.envelope(e, blend)) and (out["shift"][0, 0] >= B).all()
    assert out["after"]["penetration_max"][0, 0] == 0.0 and out["capped"][0, 0] == 0


def test_the_far_jump_keeps_its_bits():
    for shape in ((1, 5, 70), (2, 3, 150), (1, 2, 1125)):
        pos, J, Cn = R.seeded(*shape)
        jump = R.windows(shape[2])[1]
        for floor in (None, 0.0):                             # with the contacts: the still rule plants the frames beside the jump
            out = R.ground(pos, J, Cn, floor=floor)
            assert (out["shift"][:, 1, jump] == 0).all(), shape
            assert np.array_equal(out["joints"][:, 1, jump].view(np.uint32), J[:, 1, jump].view(np.uint32))
            assert (J[:, 1, jump[3], 0, 2] - J[:, 1, jump[0] - 1, 0, 2] > 0.19).all()          # it is a jump of 20 cm


def test_every_uncapped_dancer_ends_on_or_above_the_floor():
    """L + D >= F on every uncapped frame: after the float32 rounding of coordinates under 2 m (at most 1.2e-7) the body is at most
    1e-6 m below the floor, far below `tolerance`"""
    worst, seen = 0.0, 0
    for name, pos, J, Cn, floor in cases():
        out = reference(name, pos, J, Cn, floor)
        ok = (out["capped"] == 0) & np.isfinite(out["floor"])[:, None]
        pm = out["after"]["penetration_max"][ok]
        worst, seen = max(worst, float(pm.max()) if pm.size else 0.0), seen + int(ok.sum())
        assert (pm <= 1e-6).all(), (name, pm.max())
        assert (out["after"]["penetration_frames"][ok] == 0).all(), name
        assert (out["capped"][~ok] > 0).all() or not np.isfinite(out["floor"]).all()
    print(f"[ground] {seen} uncapped dancers: the body at most {worst:.3e} m below the floor after (bound 1e-6)")
    assert seen > 50


def planted_runs(planted):
    t, T = 0, planted.shape[0]
    while t < T:
        if planted[t]:
            s = t
            while s < T and planted[s]:
                s += 1
            yield t, s
            t = s
        else:
            t += 1


def test_zero_lift_planted_runs_stand_on_the_floor_on_average():
    """a run whose lift U is 0 throughout is shifted by B alone, the mean of F - Lf over it: afterwards the mean of Lf - F over the run
    is 0 up to the float32 rounding, within 1e-6 m"""
    T = 30
    J = stick(T)[None, None].copy()
    J[0, 0, 0:10, :, 2] -= np.float32(3 / 64)                          # a sunk run, a high gap, a floating run
    J[0, 0, 10:20, :, 2] += np.float32(0.5)
    J[0, 0, 20:30, :, 2] += np.float32(1 / 32)
    c = np.zeros((1, 1, T, 4), np.float32)
    c[0, 0, 0:10, 0] = c[0, 0, 20:30, 3] = 1.0
    checked, worst = 0, 0.0
    outs = [(run(J, c, floor=-1 / 32, radii=EVEN), "hand-made")] + [(reference(*x), x[0]) for x in cases()]
    for out, name in outs:
        F, pl = out["floor"], out["planes"]["planted"]
        for cc in range(pl.shape[0]):
            for d in range(pl.shape[1]):
                for t, s in planted_runs(pl[cc, d]):
                    if (out["planes"]["U"][cc, d, t:s] == 0).all() and np.isfinite(F[cc]):
                        err = abs(float(np.mean(out["planes"]["Lf_after"][cc, d, t:s] - F[cc])))
                        worst, checked = max(worst, err), checked + 1
                        assert err <= 1e-6, (name, cc, d, t, s, err)
    print(f"[ground] {checked} planted runs without lift: their mean foot low within {worst:.3e} m of the floor (bound 1e-6)")
    assert checked >= 2


def test_the_estimated_floor_is_the_median_of_the_planted_foot_lows():
    radii = G.capsule_radii()
    for name, pos, J, Cn, floor in cases():
        if floor is not None:
            continue
        out = reference(name, pos, J, Cn, floor)
        b, dn, T = J.shape[:3]
        for c in range(b):
            feet, body = [], []
            for d in range(dn):
                for t in range(T):
                    Jt = J[c, d, t].astype(np.float64)
                    if not np.isfinite(Jt).all():
                        continue
                    z = Jt[:, 2]
                    body.append(min(min(z[SMPL_PARENTS[i]], z[i]) - radii[i] for i in range(1, 24)))
                    if Cn is not None:
                        left = Cn[c, d, t, 0] > np.float32(0.95) or Cn[c, d, t, 2] > np.float32(0.95)
                        right = Cn[c, d, t, 1] > np.float32(0.95) or Cn[c, d, t, 3] > np.float32(0.95)
                    else:
                        def still(j):
                            if t == T - 1:
                                return True
                            step = J[c, d, t + 1, j].astype(np.float64) - Jt[j]
                            return np.sqrt((step[0] * step[0] + step[1] * step[1]) + step[2] * step[2]) < 0.01
                        left, right = still(7) or still(10), still(8) or still(11)
                    if left:
                        feet.append(min(z[7], z[10]) - radii[10])
                    if right:
                        feet.append(min(z[8], z[11]) - radii[11])
            want = np.median(feet) if feet else np.median(body)
            assert out["floor"][c] == want, (name, c, out["floor"][c], want)
    nothing = R.seeded(2, 3, 150)                              # the last clip has no planted frame: the median of the body lows
    assert (nothing[2][1] == 0).all() and (nothing[2][0] != 0).any()


def test_the_body_low_over_joints_is_the_body_low_over_bones():
    """csrc/ground.hip takes L as the minimum over joints of z - R[j], R[j] the largest radius of a bone ending at j: rounding is monotone,
    so it is the header's minimum over bones to the bit"""
    parents, radii = G.custom_skeleton()
    for par, rad in ((G.SMPL_PARENTS, G.capsule_radii()), (parents, radii)):
        R_j = np.full(24, -1.0)
        for i in range(1, 24):
            R_j[i], R_j[par[i]] = max(R_j[i], rad[i]), max(R_j[par[i]], rad[i])
        for shape in ((1, 5, 70), (2, 3, 150)):
            J = R.seeded(*shape)[1].reshape(-1, 24, 3)
            J = J[np.isfinite(J).all((1, 2))]
            L = R.lows(J, 2, rad, par)[0]
            assert np.array_equal((J[..., 2].astype(np.float64) - R_j).min(1), L)


# ---- the edge cases ---------------------------------------------------------------------------------------------------------------------------------
def test_blend_zero_and_blend_past_the_clip():
    pos, J, Cn = R.seeded(1, 5, 70)
    out = R.ground(pos, J, Cn, blend=0, details=True)
    B, U, pl = out["planes"]["B"], out["planes"]["U"], out["planes"]["planted"]
    assert (B[~pl] == 0).all() and (out["capped"] > 0).any()
    e = np.where(np.isfinite(J).all((-1, -2)), R.pos0((out["floor"][0] - out["planes"]["L"]) - B), 0.0)
    assert np.array_equal(U, e)                                # no spread: the lift of a frame is its own excess
    pos, J, Cn = R.seeded(2, 3, 5)
    for kw in (dict(blend=9), dict(blend=9, floor=0.0)):
        out = R.ground(pos, J, Cn, **kw)
        assert np.isfinite(out["shift"]).all() and (out["after"]["penetration_max"][out["capped"] == 0] <= 1e-6).all()


def test_another_axis_up_gives_the_same_shift():
    base = R.seeded(1, 5, 70)
    want = R.ground(*base)
    for up in (0, 1):
        p2, J2, C2 = R.permuted(*base, up)
        out = R.ground(p2, J2, C2, up=up)
        back = {0: [1, 2, 0], 1: [0, 2, 1]}[up]
        assert np.array_equal(out["shift"], want["shift"]) and np.array_equal(out["floor"], want["floor"])
        assert np.array_equal(out["joints"][..., back].view(np.uint32), want["joints"].view(np.uint32))
        assert np.array_equal(out["pos"][..., back].view(np.uint32), want["pos"].view(np.uint32))
        for k in R.COUNTS + R.VALUES:
            assert np.array_equal(out["after"][k], want["after"][k], equal_nan=True), k


def test_a_single_frame():
    pos, J, Cn = R.seeded(1, 2, 1)
    for c in (Cn, None):
        out = R.ground(pos, J, c)
        assert out["shift"].shape == (1, 2, 1) and out["max_step"].tolist() == [[0.0, 0.0]]
        assert np.array_equal(out["max_shift"], np.abs(out["shift"][..., 0]))
    out = R.ground(pos, J, None)                              # the last frame is still: both dancers planted
    assert out["before"]["planted_frames"].tolist() == [[1, 1]]


def test_a_nan_frame_keeps_its_words_and_leaves_the_metrics():
    pos, J, Cn = R.seeded(1, 5, 70)
    bad = R.windows(70)[4]
    assert not np.isfinite(J[0, 4, bad]).all()
    for c in (Cn, None):
        out = R.ground(pos, J, c, details=True)
        assert out["shift"][0, 4, bad] == 0 and np.array_equal(out["joints"][0, 4, bad].view(np.uint32), J[0, 4, bad].view(np.uint32))
        assert not out["planes"]["planted"][0, 4, bad] and np.isnan(out["joints"]).sum() == 1
        for k in R.VALUES:
            assert np.isfinite(out["before"][k][0, 4]) and np.isfinite(out["after"][k][0, 4]), k
        L = out["planes"]["L"][0, 4]
        good = np.arange(70) != bad
        x = R.pos0(out["floor"][0] - L[good])
        assert out["before"]["penetration_mean"][0, 4] == float(np.cumsum(x)[-1]) / 69
    J2 = np.array(J)
    J2[0, 2] = np.nan                                         # a dancer without a good frame: nothing to measure, nothing moves
    out = R.ground(pos, J2, Cn)
    assert (out["shift"][0, 2] == 0).all() and out["before"]["planted_frames"][0, 2] == 0
    assert out["before"]["penetration_max"][0, 2] == 0 and np.isnan(out["before"]["penetration_mean"][0, 2])
    assert np.isnan(out["before"]["float_mean"][0, 2])


# ---- what the GPU comparison rests on ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", R.variants(), ids=lambda v: v[0].replace(" ", "").replace(",", "-"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_decision_is_a_near_tie_on_the_seeded_inputs(shape, variant):
    pos, J, Cn = R.seeded(*shape)
    name, with_contacts, floor = variant
    ok, why = R.judge(reference(f"{shape} {name}", pos, J, Cn if with_contacts else None, floor))
    assert ok, why


def test_no_decision_is_a_near_tie_with_other_parameters():
    for name, (pos, J, Cn), kw in R.parameter_cases():
        for c in (Cn, None):
            ok, why = R.decisions_clear(pos, J, c, **kw)
            assert ok, (name, why)


def test_the_guard_sees_a_near_tie():
    T = 4
    J = stick(T, -(1 / 32 - 0.005))[None, None]               # the ankles at float32(1/32 - 0.005): L within half a float32 step (1e-9)
    ok, why = R.judge(run(J, all_planted(1, 1, T), floor=0.0, radii=EVEN))          # of F - tolerance
    assert not ok and any("tolerance" in w for w in why)
    c = all_planted(1, 1, T)
    c[..., 0] = np.float32(0.95)                              # exactly at the threshold
    ok, why = R.judge(run(stick(T)[None, None], c, floor=0.0, radii=EVEN))
    assert not ok and any("contact_threshold" in w for w in why)
    assert R.judge(run(stick(T)[None, None], all_planted(1, 1, T), floor=-1 / 32, radii=EVEN))[0]


# ---- the tenth header --------------------------------------------------------------------------------------------------------------------------
def test_the_tenth_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_ground()
    assert list(abi.functions) == NAMES and L.GROUND.functions == abi.functions and L.GROUND.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_GROUND_LAUNCHES=5, TC_GROUND_METRICS_LAUNCHES=3, TC_GROUND_MAX_DANCERS=32, TC_GROUND_MAX_BLEND=1024,
                                 TC_GROUND_WS_PER_FRAME=73, TC_GROUND_MEDIAN_KEYS=4096, TC_GROUND_DIGIT_BITS=4, TC_GROUND_LEFT=1,
                                 TC_GROUND_RIGHT=2, TC_GROUND_GOOD=4, TC_GROUND_CAPPED=8)
    I, VP, LONG, D, F = C.c_int, C.c_void_p, C.c_long, C.c_double, C.c_float
    assert abi.functions["tcf_ground_workspace"][:2] == (I, [I, I, I, VP])
    assert abi.functions["tcf_ground_metrics"][:2] == (I, [VP] * 4 + [I] * 4 + [VP] * 3 + [F, D, D, VP, LONG] + [VP] * 4)
    assert abi.functions["tcf_ground"][:2] == (I, [VP] * 5 + [I] * 4 + [VP] * 3 + [F, D, D, I, D, VP, LONG] + [VP] * 12)
    assert abi.functions["tcf_ground"][2][:5] == ["const float*", "const float*", "const long*", "const float*", "const long*"]
    with open(_abi.HEADER_GROUND) as f:
        text = f.read()
    flat = " ".join(text.replace("*", " ").split())
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text and "Not built" in text
    assert "choices, not measurements" in flat and "penetrate" in flat and "#define TC_GROUND_LAUNCHES 5" in text
    for gone in ("mesh-level soles", "sloped or uneven floors", "a floor per dancer", "bending knees to absorb a correction",
                 "correcting inside the sampler", "drawing the grid at the estimated floor"):
        assert gone in flat, gone
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_", "tcj_", "tck_", "tcg_", "tcp_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_ground.h", prefix=prefix)
    for names in (L.ABI.functions, L.EXT.functions, L.GLTF.functions, L.SKIN.functions, L.SHADE.functions, L.MJPEG.functions,
                  L.FOOTLOCK.functions, L.GROUP.functions, L.APART.functions, L.EXPORTS):
        assert not any(n.startswith("tcf_") for n in names)
    frozen = {**L.ABI.constants, **L.EXT.constants, **L.GLTF.constants, **L.SKIN.constants, **L.SHADE.constants, **L.MJPEG.constants,
              **L.FOOTLOCK.constants, **L.GROUP.constants, **L.APART.constants}
    assert not any(k.startswith("TC_GROUND") for k in frozen) and len(L.ABI.functions) == 79 and len(L.APART.functions) == 2
    assert (P.MAX_DANCERS, P.MAX_BLEND) == (32, 1024)
    for header, words in (("tcdiff_apart.h", "vertical moves"), ("tcdiff_footlock.h", "floor penetration and the height of the anchor")):
        with open(os.path.join(ROOT, "include", header)) as f:
            assert words in " ".join(f.read().replace("*", " ").split())          # the earlier headers are left as they were


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    syms = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    assert sorted(s for s in syms if s.startswith("tcf_")) == sorted(NAMES)
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    n = C.c_long(-1)
    want = (73 * 2 * 3 * 10 + 7) // 8 * 8                                 # 4380 rounded up
    assert lib.tcf_ground_workspace(2, 3, 10, C.addressof(n)) == 0 and n.value == want == 4384
    assert lib.tcf_ground_workspace(1, 1, 1, C.addressof(n)) == 0 and n.value == 80
    assert lib.tcf_ground_workspace(2, 3, 10, None) == -1
    for bad in ((0, 3, 10), (2, 0, 10), (2, 3, 0), (2, 3, -1)):
        assert lib.tcf_ground_workspace(*bad, C.addressof(n)) == -1, bad
    assert lib.tcf_ground_workspace(2, 33, 10, C.addressof(n)) == -4
    assert lib.tcf_ground_workspace(2 ** 14, 32, 2 ** 14, C.addressof(n)) == -4
    parents, radii = (C.c_int * 24)(*SMPL_PARENTS), (C.c_double * 24)(*G.capsule_radii())
    js, cs = (C.c_long * 3)(2160, 720, 72), (C.c_long * 4)(120, 40, 4, 1)
    nan, inf, big = float("nan"), float("inf"), 1 << 40

    def call(pos=p, joints=p, js=js, contacts=p, cs=cs, b=2, dn=3, T=10, up=2, parents=parents, radii=radii, floor_in=p, thr=0.95,
             still=0.01, tol=0.005, blend=5, max_lift=0.5, ws=p, ws_bytes=want - 1, pos_out=p, joints_out=p, shift=p, floor=p, cb=p, vb=p,
             ca=p, va=p, capped=p, max_shift=p, max_step=p):
        return lib.tcf_ground(pos, joints, js, contacts, cs, b, dn, T, up, parents, radii, floor_in, thr, still, tol, blend, max_lift, ws,
                              ws_bytes, pos_out, joints_out, shift, floor, cb, vb, ca, va, capped, max_shift, max_step, None)

    def metrics(joints=p, js=js, contacts=p, cs=cs, b=2, dn=3, T=10, up=2, parents=parents, radii=radii, floor_in=p, thr=0.95, still=0.01,
                tol=0.005, ws=p, ws_bytes=want - 1, floor=p, counts=p, values=p):
        return lib.tcf_ground_metrics(joints, js, contacts, cs, b, dn, T, up, parents, radii, floor_in, thr, still, tol, ws, ws_bytes, floor,
                                      counts, values, None)

    for fn in (call, metrics):                                             # good arguments but for one byte of workspace
        assert fn() == -1 and fn(contacts=None, cs=None, floor_in=None) == -1
        assert fn(ws=p + 4, ws_bytes=want) == -2 and fn(floor_in=p + 4, ws_bytes=want) == -2
        for kw in (dict(joints=None), dict(js=None), dict(cs=None), dict(parents=None), dict(radii=None), dict(ws=None), dict(floor=None),
                   dict(b=0), dict(dn=0), dict(T=0), dict(T=-3), dict(up=-1), dict(up=3), dict(thr=nan), dict(still=-0.01), dict(still=nan),
                   dict(still=inf), dict(tol=-1.0), dict(tol=inf), dict(js=(C.c_long * 3)(2160, -720, 72)), dict(cs=(C.c_long * 4)(0, 0, -4, 1))):
            assert fn(ws_bytes=big, **kw) == -1, (fn.__name__, kw)
        for kw in (dict(dn=33), dict(b=2 ** 14, dn=32, T=2 ** 14)):
            assert fn(ws_bytes=big, **kw) == -4, (fn.__name__, kw)
        for j, parent in ((3, 5), (7, 7), (2, -1)):                         # a parent after its child, itself, none
            wrong = list(SMPL_PARENTS)
            wrong[j] = parent
            assert fn(parents=(C.c_int * 24)(*wrong), ws_bytes=big) == -1, (j, parent)
        for value in (-0.01, nan, inf):
            wrong = list(G.capsule_radii())
            wrong[11] = value
            assert fn(radii=(C.c_double * 24)(*wrong), ws_bytes=big) == -1, value
        wrong = list(G.capsule_radii())
        wrong[0] = nan                                                     # entry 0 is unused: the call gets as far as the workspace
        assert fn(radii=(C.c_double * 24)(*wrong)) == -1 and fn(radii=(C.c_double * 24)(*wrong), ws=p + 4, ws_bytes=want) == -2
    assert call(shift=p + 4, ws_bytes=want) == -2 and call(shift=None, ws=p + 4, ws_bytes=want) == -2          # shift may be NULL
    for kw in (dict(pos=None), dict(pos_out=None), dict(joints_out=None), dict(cb=None), dict(vb=None), dict(ca=None), dict(va=None),
               dict(capped=None), dict(max_shift=None), dict(max_step=None), dict(blend=-1), dict(max_lift=-0.1), dict(max_lift=nan),
               dict(max_lift=inf)):
        assert call(ws_bytes=big, **kw) == -1, kw
    assert call(ws_bytes=big, blend=1025) == -4 and call(ws_bytes=big, blend=1025, up=3) == -1          # the order
    assert call(ws_bytes=big, dn=33, js=(C.c_long * 3)(0, 0, -1)) == -4
    assert metrics(counts=None, ws_bytes=big) == -1 and metrics(values=None, ws_bytes=big) == -1


def test_the_tenth_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.GROUND.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_ground.h"', '#include "tcdiff_ground.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "ground.c", tmp_path / "ground"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.GROUND.constants[n] for n in names]
    calls = ['#include "tcdiff_ground.h"', '#include "tcdiff_ground.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.GROUND.functions.items():
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
def test_ground_and_ground_metrics_refuse_before_any_launch():
    import tcdiff_amd
    assert tcdiff_amd.ground is P.ground and tcdiff_amd.ground_metrics is P.ground_metrics and tcdiff_amd.Ground is P.Ground
    assert {"ground", "ground_metrics", "Ground"} <= set(tcdiff_amd.__all__)
    assert P.Ground._fields == ("pos", "joints", "floor", "before", "after", "capped", "max_shift", "max_step", "shift")
    sig = inspect.signature(P.ground).parameters
    assert list(sig) == ["pos", "joints", "contacts", "dn", "floor", "up", "radii", "parents", "contact_threshold", "still", "tolerance", "blend",
                         "max_lift", "return_shift"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, inspect.Parameter.empty, None, 2, None, None, 0.95, 0.01, 0.005, 5, 0.5, False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[3:])
    sig = inspect.signature(P.ground_metrics).parameters
    assert list(sig) == ["joints", "contacts", "floor", "up", "radii", "parents", "contact_threshold", "still", "tolerance"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, None, 2, None, None, 0.95, 0.01, 0.005]
    J, pos, c = torch.zeros(2, 3, 6, 24, 3), torch.zeros(2, 18, 3), torch.zeros(2, 3, 6, 4)
    for fn, kw in ((P.ground, dict(pos=pos, joints=J, contacts=c, dn=3)), (P.ground_metrics, dict(joints=J, contacts=c))):
        with pytest.raises(L.TcdiffError, match="MI355X only"):
            fn(**kw)
        with pytest.raises(L.TcdiffError, match="MI355X only"):
            fn(**dict(kw, floor=torch.zeros(2, dtype=torch.float64)))
    late = list(SMPL_PARENTS)
    late[3] = 5
    shared = (dict(joints=J[0]), dict(joints=J.double()), dict(joints=J.numpy()), dict(joints=torch.zeros(2, 3, 6, 23, 3)), dict(joints=J[:, :, :0]),
              dict(joints=J.transpose(-1, -2).contiguous().transpose(-1, -2)), dict(joints=torch.zeros(2, 33, 6, 24, 3)),
              dict(contacts=c[..., :3]), dict(contacts=c.double()), dict(contacts=c.numpy()), dict(contacts=c[:1]), dict(up=3), dict(up=-1),
              dict(up=True), dict(floor=float("nan")), dict(floor="0"), dict(floor=True), dict(floor=torch.zeros(3, dtype=torch.float64)),
              dict(floor=torch.zeros(2)), dict(contact_threshold=float("nan")), dict(contact_threshold=None), dict(still=-0.01),
              dict(still=float("inf")), dict(tolerance=-1), dict(tolerance=float("nan")), dict(radii=np.ones(23)), dict(radii=-np.ones(24)),
              dict(radii=np.full(24, np.nan)), dict(radii="abc"), dict(parents=SMPL_PARENTS[:5]), dict(parents=late))
    for bad in shared + (dict(pos=pos[:, :17]), dict(pos=pos.double()), dict(pos=pos.numpy()), dict(dn=2), dict(dn=3.0), dict(dn=True),
                         dict(blend=-1), dict(blend=1025), dict(blend=5.0), dict(max_lift=-0.1), dict(max_lift=float("inf")), dict(max_lift=None)):
        kw = dict(pos=pos, joints=J, contacts=c, dn=3)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match="ground"):
            P.ground(kw.pop("pos"), kw.pop("joints"), **kw)
    for bad in shared:
        kw = dict(joints=J, contacts=c)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match="ground_metrics"):
            P.ground_metrics(kw.pop("joints"), **kw)
    for doc in (P.__doc__, P.ground.__doc__, P.ground_metrics.__doc__):
        assert "choices, not measurements" in " ".join(doc.split())
    assert "unpinned" in P.__doc__ and "Not built" in P.__doc__ and "penetrate" in P.__doc__


# ---- render_sample ----------------------------------------------------------------------------------------------------------------------------
def test_render_sample_grounds_after_keep_apart_and_before_the_foot_lock_and_only_when_asked(monkeypatch, tmp_path):
    from tcdiff_amd import GaussianDiffusion, apart, export, footlock
    ground = P
    assert GaussianDiffusion.ground is False and GaussianDiffusion.keep_apart is False and GaussianDiffusion.foot_lock is False
    params = list(inspect.signature(GaussianDiffusion.render_sample).parameters)
    assert params == ["self", "shape", "cond", "normalizer", "epoch", "render_out", "fk_out", "name", "sound", "mode", "noise", "constraint",
                      "sound_folder", "start_point", "render", "required_dancer_num", "x_0", "render_len", "glb_out", "draw_out"]
    q, pos, poses, contacts = (torch.full((1,), float(k)) for k in range(4))          # stand-ins: only their identity matters
    moved_pos, moved_poses, low_pos, low_poses, locked_q, locked_joints = (torch.full((1,), float(k)) for k in range(10, 16))
    calls = []

    def fake_export(x, normalizer, mode, dn, **kw):
        calls.append(("export", dn))
        return q, pos, poses, contacts

    def fake_apart(pos_, joints_, **kw):
        calls.append(("keep_apart", pos_, joints_, kw["dn"]))
        return apart.Apart(moved_pos, moved_poses, *[None] * 9)

    def fake_ground(pos_, joints_, contacts_=None, **kw):
        calls.append(("ground", pos_, joints_, contacts_, kw["dn"], kw.get("floor")))
        return ground.Ground(low_pos, low_poses, *[None] * 7)

    def fake_lock(q_, pos_, contacts_, **kw):
        calls.append(("foot_lock", q_, pos_, contacts_, kw["dn"]))
        return footlock.FootLock(locked_q, locked_joints, None, None, None)

    def fake_write(folder, mode, epoch, name, q_, pos_, poses_):
        calls.append(("write", q_, pos_, poses_))

    monkeypatch.setattr(export, "export_poses", fake_export)
    monkeypatch.setattr(export, "write_fk_out", fake_write)
    monkeypatch.setattr(apart, "keep_apart", fake_apart)
    monkeypatch.setattr(ground, "ground", fake_ground)
    monkeypatch.setattr(footlock, "foot_lock", fake_lock)
    d = GaussianDiffusion.__new__(GaussianDiffusion)
    torch.nn.Module.__init__(d)
    monkeypatch.setattr(GaussianDiffusion, "_render_samples", lambda self, *a: _FakeSamples())
    monkeypatch.setattr(GaussianDiffusion, "_skeleton", lambda self, dev: (list(SMPL_PARENTS), [[0.0] * 3] * 24))

    def render(**attrs):
        calls.clear()
        for k, v in attrs.items():
            setattr(d, k, v)
        try:
            d.render_sample(None, None, object(), 1, None, fk_out=str(tmp_path), name=["a"], required_dancer_num=3)
        finally:
            for k in attrs:
                delattr(d, k)
        return [c[0] for c in calls]

    assert render() == ["export", "write"]
    assert calls[1][1] is q and calls[1][2] is pos and calls[1][3] is poses          # export_poses' own objects are handed on
    assert render(ground=True) == ["export", "ground", "write"]
    assert calls[1][1] is pos and calls[1][2] is poses and calls[1][3] is contacts and calls[1][4] == 3 and calls[1][5] is None
    assert calls[2][1] is q and calls[2][2] is low_pos and calls[2][3] is low_poses
    assert render(ground=0.25) == ["export", "ground", "write"] and calls[1][5] == 0.25          # a number is the floor
    assert render(keep_apart=True, ground=True, foot_lock=True) == ["export", "keep_apart", "ground", "foot_lock", "write"]
    assert calls[2][1] is moved_pos and calls[2][2] is moved_poses and calls[2][3] is contacts
    assert calls[3][1] is q and calls[3][2] is low_pos and calls[3][3] is contacts          # the lock pins feet that stand on the floor
    assert calls[4][1] is locked_q and calls[4][2] is low_pos and calls[4][3] is locked_joints
    assert render(keep_apart=True, foot_lock=True) == ["export", "keep_apart", "foot_lock", "write"]          # off: as before
    assert calls[2][2] is moved_pos and calls[3][2] is moved_pos


class _FakeSamples:
    """what render_sample asks of the samples before the export: are they on the device"""
    is_cuda = True
    device = torch.device("cpu")
