"""CPU checks of the foot lock (no GPU): the seventh header and its binding, the refusals, the numpy restatement tests/footlock_ref.py
of include/tcdiff_footlock.h held to what the feature is for by a forward kinematics written separately here (rotation matrices, not
quaternions), and csrc/footlock_math.h built for the host as a stand-alone program with the address and undefined-behaviour
sanitizers against the restatement."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import footlock_ref as R
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd import footlock as F
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tck_foot_lock_workspace", "tck_foot_lock"]


# ---- a forward kinematics of its own: Rodrigues matrices, whole arrays at once ---------------------------------------------------------------
def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r, axis=-1)[..., None, None]
    Kx = np.zeros(r.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -r[..., 2], r[..., 1], r[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -r[..., 0], -r[..., 1], r[..., 0]
    small = th < 1e-6
    s = np.where(small, 1.0 - th ** 2 / 6, np.sin(th) / np.where(small, 1.0, th))
    c = np.where(small, 0.5 - th ** 2 / 24, (1 - np.cos(th)) / np.where(small, 1.0, th) ** 2)
    return np.eye(3) + s * Kx + c * (Kx @ Kx)


def fk64(q, pos, offsets=SMPL_OFFSETS, parents=SMPL_PARENTS):
    """q (..., 24, 3), pos (..., 3) -> world positions (..., 24, 3) and world rotation matrices (..., 24, 3, 3), float64"""
    local = rodrigues(q)
    off = np.asarray(offsets, np.float32).astype(np.float64)
    P, W = [None] * 24, [None] * 24
    for j in range(24):
        p = parents[j]
        if p < 0:
            P[j], W[j] = np.asarray(pos, np.float64), local[..., j, :, :]
        else:
            P[j] = P[p] + W[p] @ off[j]
            W[j] = W[p] @ local[..., j, :, :]
    return np.stack(P, -2), np.stack(W, -3)


def frames_of(a, dn=R.DN):
    """(b, T dn, ...) rows -> (b, dn, T, ...)"""
    a = np.asarray(a)
    return np.moveaxis(a.reshape((a.shape[0], a.shape[1] // dn, dn) + a.shape[2:]), 2, 1)


def check_properties(q, pos, ref, dn=R.DN, offsets=SMPL_OFFSETS, tol=1e-12):
    """what the feature is for, on the restatement's unrounded output"""
    P0, W0 = fk64(frames_of(q, dn), frames_of(pos, dn), offsets)
    P1, W1 = fk64(frames_of(ref["q64"], dn), frames_of(pos, dn), offsets)
    for leg, (h, k, a, e) in enumerate(R.LEGS):
        assert np.abs(P1[..., h, :] - P0[..., h, :]).max() == 0.0                     # the hips stay
        assert np.abs(W1[..., a, :, :] - W0[..., a, :, :]).max() <= tol                 # the foot keeps its world orientation
        assert np.abs((P1[..., e, :] - P1[..., a, :]) - (P0[..., e, :] - P0[..., a, :])).max() <= tol
        g, st = ref["g"][:, :, leg], ref["status"][:, :, leg]
        pin = np.where((g == 2)[..., None], P1[..., e, :], P1[..., a, :])
        free = (g != 0) & (st != 2)
        if free.any():
            assert np.linalg.norm(pin - ref["anchor"][:, :, leg], axis=-1)[free].max() <= tol
        shifted = pin - np.where((g == 2)[..., None], P0[..., e, :], P0[..., a, :])
        ok = st == 1
        if ok.any():
            assert np.abs(shifted - ref["d"][:, :, leg])[ok].max() <= tol           # eased frames land on the wanted shift as well
    others = [j for j in range(24) if j not in (1, 2, 4, 5, 7, 8)]
    assert np.array_equal(np.asarray(ref["q"])[:, :, others], np.asarray(q)[:, :, others])
    return P0, P1


# ---- the restatement is held to the construction's purpose -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_the_restatement_pins_the_feet_and_moves_nothing_else(name):
    q, pos, contacts, blend, ref = R.case(name)
    T, _, runs = R.CASES[name]
    P0, P1 = check_properties(q, pos, ref)
    want = np.array([[sum(last - first + 1 for first, last, _ in runs[d][leg]) for leg in range(2)] for d in range(R.DN)])
    assert np.array_equal(ref["planted"][0], want)
    slid = np.linalg.norm(np.diff(P0, axis=2), axis=-1)                                 # the raw motion slides by construction
    if T > 1:
        assert slid[..., [7, 8, 10, 11]].min() >= 5e-3
    if name == "off":
        assert np.array_equal(ref["q"], q) and not ref["planted"].any() and not ref["max_shift"].any()
    else:
        assert ref["max_shift"].max() > 0 or T == 1
    far = np.ones((R.DN, 2, T), bool)                                                  # frames more than blend from any planted frame
    for t in range(T):
        lo, hi = max(0, t - blend), min(T, t + blend + 1)
        far[:, :, t] = ~(ref["g"][0, :, :, lo:hi] != 0).any(-1)
    assert not ref["d"][0][far].any()
    for leg, joints in enumerate(R.LEGS):
        same = frames_of(ref["q"])[0][far[:, leg]][:, list(joints[:3])] == frames_of(q)[0][far[:, leg]][:, list(joints[:3])]
        assert same.all()


def test_both_easing_rules_at_their_border():
    q, pos, contacts, blend, ref = R.case("gaps")
    assert blend == 3
    d = ref["d"][0, 0, 0]                                                              # dancer 0, left leg: runs 0-4, 11-14, 22-25, 34-36
    for t in range(5, 11):                                                             # G - 1 = 6 = 2 blend: bridged linearly
        assert np.allclose(d[t], ((11 - t) * d[4] + (t - 4) * d[11]) / 7, rtol=0, atol=1e-15)
    for t in range(15, 22):                                                            # G - 1 = 7 = 2 blend + 1: two ramps, a frame of rest
        lam0, lam1 = max(0.0, 1 - (t - 14) / 4), max(0.0, 1 - (22 - t) / 4)
        assert np.allclose(d[t], lam0 * d[14] + lam1 * d[22], rtol=0, atol=1e-15) and (lam0 == 0 or lam1 == 0)
    assert not d[18].any() and d[17].any() and d[19].any()
    for t in range(26, 34):                                                            # 8 frames: two frames of rest
        lam0, lam1 = max(0.0, 1 - (t - 25) / 4), max(0.0, 1 - (34 - t) / 4)
        assert np.allclose(d[t], lam0 * d[25] + lam1 * d[34], rtol=0, atol=1e-15)
    assert not d[29].any() and not d[30].any()
    assert np.allclose(d[38], 0.5 * d[36], rtol=0, atol=1e-15) and d[36].any()        # after the last run: one ramp, the other absent
    d0 = R.case("blend0")[4]["d"][0]
    g0 = R.case("blend0")[4]["g"][0]
    assert not d0[g0 == 0].any() and d0[g0 != 0].any()                                 # blend = 0: no easing


def test_an_ankle_run_touching_a_toe_run_is_two_runs():
    ref = R.case("T130-edges")[4]
    A = ref["anchor"][0, 0, 0]
    assert ref["g"][0, 0, 0, 63] == 1 and ref["g"][0, 0, 0, 64] == 2
    assert (A[55:64] == A[55]).all() and (A[64:73] == A[64]).all() and not (A[63] == A[64]).any()
    assert np.isnan(A[54]).all() and np.isnan(A[73]).all()


def test_a_target_beyond_reach_is_clamped_onto_the_ray():
    q, pos, contacts, ref = R.reach_case()
    assert ref["clamped"][0, 0, 0] > 0 and ref["clamped"][0, 1, 1] > 0 and np.isfinite(ref["q64"]).all()
    P0, P1 = check_properties(q, pos, ref)
    l = [R.chain(q[0, 0], pos[0, 0], leg) for leg in range(2)]
    seen = 0
    for (c, dd, leg, t), inf in ref["info"].items():
        if ref["status"][c, dd, leg, t] != 2:
            continue
        seen += 1
        h, k, a, e = R.LEGS[leg]
        H, A1 = P1[c, dd, t, h], P1[c, dd, t, a]
        rmax = (l[leg]["l1"] + l[leg]["l2"]) * (1 - 1e-3)
        assert abs(np.linalg.norm(A1 - H) - inf["rp"]) <= 1e-12 and np.abs(A1 - np.asarray(inf["target"])).max() <= 1e-12
        wanted = P0[c, dd, t, a] + ref["d"][c, dd, leg, t] - H
        assert np.linalg.norm(np.cross(A1 - H, wanted)) <= 1e-12 and np.dot(A1 - H, wanted) > 0
        assert inf["rp"] == pytest.approx(rmax, abs=1e-15) or inf["rp"] > rmax          # r_max, unless the leg was already straighter
    assert seen == ref["clamped"].sum()


def test_the_straight_leg_takes_the_fallback_axis():
    offsets = [list(o) for o in SMPL_OFFSETS]
    for k, a in ((4, 7), (5, 8)):
        offsets[a] = list(offsets[k])                                                # shin parallel to thigh, exactly: a zero knee is a straight leg
    q, pos = R.motion(6, seed=3)
    q = q.copy()
    q[:, :, [4, 5]] = 0.0
    pos = pos.copy()
    pos[0, :, 1] += np.repeat(np.linspace(0.0, 0.05, 6), R.DN).astype(np.float32)     # the root rises and drifts over pinned feet
    contacts = R.contacts_of(6, [[[(0, 5, "a")], [(0, 5, "a")]], [[(0, 5, "a")], [(0, 5, "a")]]])
    ref = R.foot_lock(q, pos, contacts, dn=R.DN, offsets=offsets)
    taken = [inf["fallback"] for inf in ref["info"].values()]
    assert taken and all(taken)
    check_properties(q, pos, ref, offsets=offsets)
    P1, W1 = fk64(frames_of(ref["q64"]), frames_of(pos), offsets)
    bent = 0
    for (c, dd, leg, t), inf in ref["info"].items():
        h, k, a, e = R.LEGS[leg]
        thigh, shin = P1[c, dd, t, k] - P1[c, dd, t, h], P1[c, dd, t, a] - P1[c, dd, t, k]
        axis = W1[c, dd, t, h] @ np.array([1.0, 0.0, 0.0])                              # R_h' . x, made perpendicular to the thigh:
        axis = axis - thigh * (axis @ thigh) / (thigh @ thigh)                          # the knee's hinge after the solve
        axis /= np.linalg.norm(axis)
        n = np.cross(thigh, shin)
        if np.linalg.norm(n) > 1e-6:
            bent += 1
            assert np.linalg.norm(np.cross(n / np.linalg.norm(n), axis)) <= 1e-9        # it bent about the fallback axis
    assert bent > 0


def test_motion_labels_cannot_tie():
    q, pos, ref = R.motion_case()
    assert ref["min_margin"] > 1e-6
    assert (ref["g"][..., -1] == 1).all() and 0 < ref["planted"].min() and ref["planted"].max() < q.shape[1] // R.DN
    check_properties(q, pos, ref)


# ---- csrc/footlock_math.h on the host, under the sanitizers ------------------------------------------------------------------------------------
def run_host(exe, tmp, q, pos, contacts, dn, blend, offsets=SMPL_OFFSETS, thr=0.95, still=0.01, reach=1e-3):
    b, T = q.shape[0], q.shape[1] // dn
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([b, dn, T, contacts is not None, blend], np.int32).tobytes() + np.float32(thr).tobytes() +
                np.array([still, reach], np.float64).tobytes() + np.asarray(offsets, np.float32).tobytes() +
                np.ascontiguousarray(q, np.float32).tobytes() + np.ascontiguousarray(pos, np.float32).tobytes() +
                (b"" if contacts is None else np.ascontiguousarray(contacts, np.float32).tobytes()))
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = (tmp / "out.bin").read_bytes()
    rows, seqs = b * T * dn, b * dn * 2
    sizes = [("q64", np.float64, (b, T * dn, 2, 3, 3)), ("d", np.float64, (b, dn, 2, T, 3)), ("max_shift", np.float64, (b, dn, 2)),
             ("status", np.int32, (b, dn, 2, T)), ("planted", np.int32, (b, dn, 2)), ("clamped", np.int32, (b, dn, 2))]
    out, at = {}, 0
    for key, dt, shape in sizes:
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[key] = np.frombuffer(raw[at:at + n], dt).reshape(shape)
        at += n
    assert at == len(raw) and rows * 18 == out["q64"].size and seqs == out["planted"].size
    return out


def compare_host(out, ref):
    assert np.array_equal(out["planted"], ref["planted"]) and np.array_equal(out["clamped"], ref["clamped"])
    assert np.array_equal(out["status"], ref["status"])
    assert np.allclose(out["max_shift"], ref["max_shift"], rtol=1e-12, atol=0)
    assert np.abs(out["d"] - ref["d"]).max() <= 1e-12
    worst = 0.0
    for leg, joints in enumerate(R.LEGS):
        for k, j in enumerate(joints[:3]):
            theirs, ours = ref["q64"][:, :, j].reshape(-1, 3), out["q64"][:, :, leg, k].reshape(-1, 3)
            worst = max([worst] + [R.angle_between(x, y) for x, y in zip(theirs, ours)])
    assert worst <= 1e-9, worst
    return worst


def test_footlock_math_on_the_host_under_the_sanitizers_agrees_with_the_restatement(tmp_path):
    """the SAME per-frame functions the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "footlock_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "footlock_host.cpp")])
    worst = 0.0
    for name in R.CASES:
        q, pos, contacts, blend, ref = R.case(name)
        worst = max(worst, compare_host(run_host(exe, tmp_path, q, pos, contacts, R.DN, blend), ref))
    q, pos, ref = R.motion_case()
    worst = max(worst, compare_host(run_host(exe, tmp_path, q, pos, None, R.DN, 5), ref))
    q, pos, contacts, ref = R.reach_case()
    worst = max(worst, compare_host(run_host(exe, tmp_path, q, pos, contacts, R.DN, 5), ref))
    print(f"[footlock] host build against the restatement: {worst:.3e} rad at most (bound 1e-9)")


# ---- the seventh header ------------------------------------------------------------------------------------------------------------------------
def test_the_seventh_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_footlock()
    assert list(abi.functions) == NAMES and L.FOOTLOCK.functions == abi.functions and L.FOOTLOCK.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_FOOTLOCK_LAUNCHES=3, TC_FOOTLOCK_CHUNK=64, TC_FOOTLOCK_WS_PER_FRAME=480)
    I, VP, LONG, FL, D = C.c_int, C.c_void_p, C.c_long, C.c_float, C.c_double
    assert abi.functions["tck_foot_lock_workspace"][:2] == (I, [I, I, I, VP])
    assert abi.functions["tck_foot_lock"][:2] == (I, [VP, VP, VP, VP, I, I, I, FL, D, I, D, VP, VP, VP, LONG, VP, VP, VP, VP, VP, VP])
    with open(_abi.HEADER_FOOTLOCK) as f:
        text = f.read()
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text and "Not built" in text
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_", "tcj_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_footlock.h", prefix=prefix)
    for names in (L.ABI.functions, L.EXT.functions, L.GLTF.functions, L.SKIN.functions, L.SHADE.functions, L.MJPEG.functions, L.EXPORTS):
        assert not any(n.startswith("tck_") for n in names)
    frozen = {**L.ABI.constants, **L.EXT.constants, **L.GLTF.constants, **L.SKIN.constants, **L.SHADE.constants, **L.MJPEG.constants}
    assert not any(k.startswith("TC_FOOTLOCK") for k in frozen) and len(L.ABI.functions) == 79


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    syms = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    assert sorted(s for s in syms if s.startswith("tck_")) == sorted(NAMES)
    assert not [s for s in syms if "foot_lock" in s.lower() and s.split("_")[0] in ("tcdiff", "tcx", "tcs", "tcr", "tcj")]
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    n = C.c_long(-1)
    assert lib.tck_foot_lock_workspace(2, 3, 10, C.addressof(n)) == 0 and n.value == 480 * 60
    assert lib.tck_foot_lock_workspace(2, 3, 10, None) == -1
    for bad in ((0, 3, 10), (2, 0, 10), (2, 3, 0), (2, 3, -1)):
        assert lib.tck_foot_lock_workspace(*bad, C.addressof(n)) == -1
    assert lib.tck_foot_lock_workspace(2 ** 16, 2 ** 8, 2 ** 8, C.addressof(n)) == -4
    parents, offsets = (C.c_int * 24)(*SMPL_PARENTS), (C.c_float * 72)(*[v for o in SMPL_OFFSETS for v in o])
    strides = (C.c_long * 4)(80, 40, 4, 1)

    def call(q=p, pos=p, contacts=p, strides=strides, b=1, dn=2, T=10, thr=0.95, still=0.01, blend=5, reach=1e-3, parents=parents,
             offsets=offsets, ws=p, ws_bytes=480 * 20 - 1, q_out=p, joints=p, planted=p, clamped=p, max_shift=p):
        return lib.tck_foot_lock(q, pos, contacts, strides, b, dn, T, thr, still, blend, reach, parents, offsets, ws, ws_bytes, q_out,
                                 joints, planted, clamped, max_shift, None)
    assert call() == -1                                                    # good arguments but for one byte of workspace
    assert call(ws=p + 4, ws_bytes=480 * 20) == -2
    assert call(contacts=None, strides=None, joints=None) == -1           # these may be NULL: it is the workspace again
    assert call(contacts=None, strides=None, joints=None, ws=p + 4, ws_bytes=480 * 20) == -2
    big = 1 << 40
    for kw in (dict(q=None), dict(pos=None), dict(strides=None), dict(parents=None), dict(offsets=None), dict(ws=None), dict(q_out=None),
               dict(planted=None), dict(clamped=None), dict(max_shift=None), dict(b=0), dict(dn=0), dict(T=0), dict(T=-3), dict(blend=-1),
               dict(reach=0.0), dict(reach=0.5), dict(reach=-0.1), dict(reach=float("nan")), dict(still=-1.0), dict(still=float("nan")),
               dict(thr=float("nan")), dict(strides=(C.c_long * 4)(80, 40, -4, 1))):
        assert call(ws_bytes=big, **kw) == -1, kw
    assert call(b=2 ** 16, dn=2 ** 8, T=2 ** 8, ws_bytes=big) == -4 and call(blend=2 ** 26, ws_bytes=big) == -4
    wrong = list(SMPL_PARENTS)
    wrong[7] = 1                                                           # the left ankle hung on the hip: not SMPL's leg
    assert call(parents=(C.c_int * 24)(*wrong), ws_bytes=big) == -4
    wrong = list(SMPL_PARENTS)
    wrong[3] = 5                                                           # a parent after its child
    assert call(parents=(C.c_int * 24)(*wrong), ws_bytes=big) == -1
    flat = [v for o in SMPL_OFFSETS for v in o]
    flat[12:15] = [0.0, 0.0, 0.0]                                          # a thigh of no length
    assert call(offsets=(C.c_float * 72)(*flat), ws_bytes=big) == -4


def test_the_seventh_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.FOOTLOCK.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_footlock.h"', '#include "tcdiff_footlock.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "footlock.c", tmp_path / "footlock"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.FOOTLOCK.constants[n] for n in names]
    calls = ['#include "tcdiff_footlock.h"', '#include "tcdiff_footlock.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.FOOTLOCK.functions.items():
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
def test_foot_lock_refuses_before_any_launch():
    import tcdiff_amd
    assert tcdiff_amd.foot_lock is F.foot_lock and tcdiff_amd.FootLock is F.FootLock
    assert F.FootLock._fields == ("q", "joints", "planted", "clamped", "max_shift")
    sig = inspect.signature(F.foot_lock).parameters
    assert list(sig) == ["q", "pos", "contacts", "dn", "contact_threshold", "still", "blend", "reach", "parents", "offsets", "return_joints"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, inspect.Parameter.empty, 0.95, 0.01, 5, 1e-3, None, None, True]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[3:])
    q, pos, contacts = torch.zeros(2, 6, 24, 3), torch.zeros(2, 6, 3), torch.zeros(2, 2, 3, 4)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        F.foot_lock(q, pos, contacts, dn=2)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        F.foot_lock(q, pos, None, dn=3)
    for bad in (dict(q=q[0]), dict(q=q.double()), dict(q=q.numpy()), dict(q=torch.zeros(2, 6, 23, 3)), dict(pos=pos[:, :5]), dict(pos=pos.half()),
                dict(dn=4), dict(dn=0), dict(dn=2.0), dict(dn=True), dict(contacts=contacts.permute(0, 2, 1, 3)), dict(contacts=contacts.double()),
                dict(contacts=contacts.numpy()), dict(blend=-1), dict(blend=2.0), dict(blend=True), dict(reach=0), dict(reach=0.5),
                dict(reach=float("nan")), dict(reach="x"), dict(still=-0.1), dict(still=None), dict(contact_threshold=float("inf")),
                dict(contact_threshold=None), dict(parents=SMPL_PARENTS[:5]), dict(offsets=SMPL_OFFSETS[:3])):
        kw = dict(q=q, pos=pos, contacts=contacts, dn=2)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match="foot_lock"):
            F.foot_lock(kw.pop("q"), kw.pop("pos"), kw.pop("contacts"), **kw)


def test_the_default_leaves_render_sample_as_it_was():
    from tcdiff_amd import GaussianDiffusion
    assert GaussianDiffusion.foot_lock is False
    params = list(inspect.signature(GaussianDiffusion.render_sample).parameters)
    assert params == ["self", "shape", "cond", "normalizer", "epoch", "render_out", "fk_out", "name", "sound", "mode", "noise", "constraint",
                      "sound_folder", "start_point", "render", "required_dancer_num", "x_0", "render_len", "glb_out", "draw_out"]
    for doc in (F.foot_lock.__doc__, F.__doc__):
        assert "choices, not measurements" in F.foot_lock.__doc__ and "unpinned" in F.__doc__ and doc
