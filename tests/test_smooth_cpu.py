"""CPU checks of the jitter scores and the rotation filter (no GPU): the tap tables of the numpy restatement tests/smooth_ref.py of
include/tcdiff_smooth.h against scipy's savgol_filter, the restatement on cases that can be checked by hand or by purpose, the
thirteenth header and its binding, the launchers' and the Python side's refusals, and csrc/smooth_math.h built for the host as a
stand-alone program with the address and undefined-behaviour sanitizers against the restatement."""
import ctypes as C
import importlib
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import smooth_ref as R
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS

S = importlib.import_module("tcdiff_amd.smooth")                   # the package's attribute of this name is the function
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcw_smoothness", "tcw_smooth_workspace", "tcw_smooth"]


# ---- 1. the tap tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,p", [(21, 3), (9, 3), (5, 2), (7, 1)])
def test_the_tables_are_scipys_interp_mode(W, p):
    signal = pytest.importorskip("scipy.signal")
    g = np.random.default_rng(W * 10 + p)
    for T in (W, W + 1, 40, 150):
        y = np.cumsum(g.normal(size=T))                             # a seeded random walk
        err = float(np.abs(R.filter_signal(y, W, p) - signal.savgol_filter(y, W, p, mode="interp")).max())
        print(f"[smooth] table W={W} p={p} T={T}: {err:.2e} from scipy at a signal scale of {np.abs(y).max():.1f}")
        assert err <= 1e-10 * np.abs(y).max()
    assert np.abs(R.table(W, p).sum(1) - 1.0).max() <= 1e-14


def test_the_packages_table_is_the_restatements():
    for W, p in ((9, 3), (21, 3), (63, 3), (3, 1), (3, 0), (5, 4)):
        assert np.array_equal(S.savgol_table(W, p), R.table(W, p)) and S.savgol_table(W, p).shape == (W, W)
    s, row = R.windows(12, 9)
    assert s.tolist() == [0, 0, 0, 0, 0, 1, 2, 3, 3, 3, 3, 3] and row.tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 5, 6, 7, 8]
    s, row = R.windows(9, 9)
    assert not s.any() and row.tolist() == list(range(9))          # T = W: every frame is a row of the one window


# ---- 2. the restatement ----------------------------------------------------------------------------------------------------------------------
def test_a_polynomial_of_the_order_comes_back_edges_included():
    t = np.arange(30, dtype=np.float64)
    for W, p in ((9, 3), (5, 2), (21, 3), (7, 1)):
        c = np.random.default_rng(p).normal(size=(p + 1, 3)) / 30.0 ** np.arange(p + 1)[:, None]
        y = sum(c[k] * t[:, None] ** k for k in range(p + 1))
        assert np.abs(R.filter_signal(y, W, p) - y).max() <= 1e-12, (W, p)


def test_a_constant_rotation_comes_back():
    q = np.tile(np.random.default_rng(2).normal(0, 0.8, (1, 24, 3)), (20, 1, 1)).astype(np.float32)
    out, copied = R.filter_rot(q, 9, 3)
    assert not copied.any()
    assert max(R.angle_between(out[t, j], q[t, j].astype(np.float64)) for t in range(20) for j in range(24)) <= 1e-12


def test_a_rotation_vector_that_flips_sign_is_filtered_across_the_flip():
    q, pos, ang, axis = R.flip_case()
    T = len(ang)
    out = R.smooth(q, pos, 1)
    err = max(R.angle_between(out["q64"][0, t, 3], ang[t] * axis) for t in range(T))
    print(f"[smooth] sign flip: {err:.2e} rad from the clean rotation (bound 1e-3)")
    assert err <= 1e-3
    # without the sign rule the same taps on the raw vectors err by radians
    raw = R.filter_signal(q[0, :, 3].astype(np.float64), 9, 3)
    assert max(R.angle_between(raw[t], ang[t] * axis) for t in range(T)) > 1.0


def test_the_filter_serves_its_purpose_on_the_seeded_noisy_dance():
    qc, pc, qn, pn = R.noisy_case()
    out = R.smooth(qn, pn, 1)
    joints = lambda q, pos: R.fk(R.frames_of(q, 1), R.frames_of(pos, 1)).astype(np.float32)
    before, after = R.smoothness(joints(qn, pn)), R.smoothness(joints(out["q"], out["pos"]))
    e0, e1 = R.rms_joint_error(qn, pn, qc, pc), R.rms_joint_error(out["q"], out["pos"], qc, pc)
    print(f"[smooth] seeded noisy dance: jitter {before['jitter'][0, 0]:.0f} -> {after['jitter'][0, 0]:.0f} m/s^3 "
          f"(ratio {after['jitter'][0, 0] / before['jitter'][0, 0]:.3f}), accel {before['accel_mean'][0, 0]:.1f} -> "
          f"{after['accel_mean'][0, 0]:.1f} m/s^2, rms joint error {e0:.4f} -> {e1:.4f} m")
    assert after["jitter"][0, 0] <= 0.35 * before["jitter"][0, 0] and e1 < e0
    assert after["accel_mean"][0, 0] < before["accel_mean"][0, 0] and not out["copied"].any()
    wide = R.smooth(qn, pn, 1, window=21)                             # the reference's window: smoother, and further from the clean motion
    assert R.rms_joint_error(wide["q"], wide["pos"], qc, pc) > 2 * e1


def test_smoothness_of_a_uniformly_accelerated_point():
    t = np.arange(12, dtype=np.float64) / 32.0                        # powers of two: every position is exact in float32
    P = np.zeros((1, 1, 12, 24, 3), np.float32)
    P[0, 0, :, :, 0] = (0.5 * 4.0 * t ** 2)[:, None]                  # 4 m/s^2 along x, every joint alike
    P[0, 0, :, :, 1] = np.arange(24) * 0.25
    m = R.smoothness(P, fps=32)
    assert m["accel_mean"][0, 0] == 4.0 and m["accel_max"][0, 0] == 4.0 and m["jitter"][0, 0] == 0.0 and m["jitter_max"][0, 0] == 0.0
    assert m["jitter_local"][0, 0] == 0.0 and m["root_jitter"][0, 0] == 0.0 and m["terms"][0, 0] == 9 * 24
    # every term ties: the lowest frame, then the lowest joint
    assert m["accel_peak"][0, 0].tolist() == [1, 0] and m["jitter_peak"][0, 0].tolist() == [1, 0]


def test_a_peak_tie_goes_to_the_lower_frame_then_the_lower_joint():
    P = np.zeros((1, 1, 8, 24, 3), np.float32)
    P[0, 0, 5, 7, 2] = P[0, 0, 5, 3, 2] = P[0, 0, 3, 9, 2] = 0.5      # three equal kinks
    m = R.smoothness(P)
    assert m["accel_max"][0, 0] == 2 * 0.5 * 900.0 and m["accel_peak"][0, 0].tolist() == [3, 9]
    P[0, 0, 3, 9, 2] = 0.0
    assert R.smoothness(P)["accel_peak"][0, 0].tolist() == [5, 3]
    assert R.smoothness(P)["jitter_peak"][0, 0].tolist() == [4, 3]   # |3 p[5]| at t = 4 and t = 5: the lower frame
    lanes = R.smoothness(np.tile(P, (1, 1, 20, 1, 1)))                # 160 frames: more than one frame a lane
    assert lanes["terms"][0, 0] == 157 * 24 and np.isfinite(lanes["jitter"][0, 0])


def test_a_nan_frame_is_counted_out_and_every_window_that_holds_it_is_copied():
    qc, pc, qn, pn = R.noisy_case(T=40, seed=3)
    q, pos = np.array(qn), np.array(pn)
    q[0, 20, 5, 1] = np.nan
    pos[0, 11, 2] = np.inf
    out = R.smooth(q, pos, 1)
    cq, cp = out["copied_q"][0, 0], out["copied_pos"][0, 0]
    assert np.flatnonzero(cq[:, 5]).tolist() == list(range(16, 25)) and cq.sum() == 9           # the frames whose window holds frame 20
    assert np.flatnonzero(cp).tolist() == list(range(7, 16)) and out["copied"][0, 0] == 18
    assert np.array_equal(out["q"][0, 16:25, 5].view(np.int32), q[0, 16:25, 5].view(np.int32))
    assert np.array_equal(out["pos"][0, 7:16].view(np.int32), pos[0, 7:16].view(np.int32))
    assert np.isfinite(np.delete(out["q"][0].reshape(40, 72), 20, 0)).all() and np.isfinite(np.delete(out["pos"][0], 11, 0)).all()
    assert np.isfinite(out["max_rot_change"]).all() and np.isfinite(out["max_pos_change"]).all()
    edge = np.array(qn)
    edge[0, 1, 0, 0] = np.nan                                        # an edge frame: the first W frames share one window
    assert np.flatnonzero(R.smooth(edge, pn, 1)["copied_q"][0, 0, :, 0]).tolist() == list(range(0, 6))
    J = R.fk(R.frames_of(qn, 1), R.frames_of(pn, 1)).astype(np.float32)
    clean = R.smoothness(J)
    J[0, 0, 20, 5, 1] = np.nan
    m = R.smoothness(J)
    assert m["terms"][0, 0] == clean["terms"][0, 0] - 4 and np.isfinite([m[k][0, 0] for k in R.FLOATS]).all()
    J[0, 0, 20, 0, 1] = np.nan                                       # the root: every root-relative term of four frames goes
    m2 = R.smoothness(J)
    assert m2["terms"][0, 0] == clean["terms"][0, 0] - 8 and np.isfinite(m2["jitter_local"][0, 0])
    J[:] = np.nan
    m = R.smoothness(J)
    assert all(np.isnan(m[k][0, 0]) for k in R.FLOATS) and m["terms"][0, 0] == 0 and m["accel_peak"][0, 0].tolist() == [-1, -1]


def test_masked_out_joints_keep_their_words():
    qc, pc, qn, pn = R.noisy_case(T=40, seed=3)
    mask = sum(1 << j for j in range(16, 24))
    out = R.smooth(qn, pn, 1, joints_mask=mask)
    assert np.array_equal(out["q"][:, :, :16].view(np.int32), qn[:, :, :16].view(np.int32)) and not out["copied"].any()
    assert not np.array_equal(out["q"][:, :, 16:], qn[:, :, 16:])
    assert np.array_equal(out["q"][:, :, 16:], R.smooth(qn, pn, 1)["q"][:, :, 16:])


# ---- 3. csrc/smooth_math.h on the host, under the sanitizers ---------------------------------------------------------------------------------
def run_host(exe, tmp, q, pos, W, p, Wr, pr, mask):
    T = q.shape[0]
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([T, W, Wr, mask], np.int32).tobytes() + R.table(W, p).tobytes() + R.table(Wr, pr).tobytes() +
                np.ascontiguousarray(q, np.float32).tobytes() + np.ascontiguousarray(pos, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp / "in.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    v = np.array([float(x) for x in r.stdout.split()])
    assert v.size == 4 * T + 4 * T * 24 + T * 24 + (T - 2) + (T - 3) + 1
    a, b = 4 * T, 4 * T + 4 * T * 24
    return v[:a].reshape(T, 4), v[a:b].reshape(T, 24, 4), v[b:b + T * 24].reshape(T, 24), v[b + T * 24:b + T * 24 + T - 2], v[-(T - 2):-1], int(v[-1])


def close(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)


def test_smooth_math_on_the_host_under_the_sanitizers_agrees_with_the_restatement(tmp_path):
    """the SAME functions the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined; equal values are
    expected but for the libm behind sin, cos and atan2, rtol 1e-12 is the bound"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "smooth_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "smooth_host.cpp")])
    qc, pc, qn, pn = R.noisy_case(T=40, seed=3)
    holes_q, holes_p = np.array(qn[0]), np.array(pn[0])
    holes_q[20, 5, 1] = np.nan
    holes_p[11, 2] = np.inf
    mask = sum(1 << j for j in range(16, 24)) | 1 << 5
    for q, pos, W, p, Wr, pr, m in ((qn[0], pn[0], 9, 3, 9, 3, R.ALL), (holes_q[:12], holes_p[:12], 5, 2, 11, 3, mask), (holes_q, holes_p, 9, 3, 21, 3, mask)):
        root, rot, change, acc, jerk, top = run_host(exe, tmp_path, q, pos, W, p, Wr, pr, m)
        ref = R.smooth(q[None], pos[None], 1, window=W, polyorder=p, root_window=Wr, root_polyorder=pr, joints_mask=m)
        assert close(root[:, :3], ref["pos64"][0]) and np.array_equal(root[:, 3] != 0, ref["copied_pos"][0, 0])
        assert close(rot[..., :3], ref["q64"][0]) and np.array_equal(rot[..., 3] != 0, ref["copied_q"][0, 0])
        want = R.rot_change(q, ref["q"][0])
        assert np.array_equal(rot[..., :3].astype(np.float32).view(np.int32), ref["q"][0].view(np.int32))
        assert np.array_equal(np.isnan(change), np.isnan(want)) and np.allclose(change, want, rtol=1e-9, atol=1e-15, equal_nan=True)
        track = np.zeros((1, 1, q.shape[0], 24, 3), np.float32)
        track[0, 0, :, 0] = pos
        P = track[0, 0, :, 0].astype(np.float64)
        with np.errstate(invalid="ignore"):
            a = np.sqrt((((P[2:] - 2.0 * P[1:-1]) + P[:-2]) ** 2).sum(-1)) * 900.0
        assert close(acc, a) and close(jerk, np.sqrt(((((P[3:] - 3.0 * P[2:-1]) + 3.0 * P[1:-2]) - P[:-3]) ** 2).sum(-1)) * 27000.0)
        assert top == 1 + int(np.nanargmax(np.where(np.isfinite(a), a, np.nan)))


# ---- 4. the thirteenth header ------------------------------------------------------------------------------------------------------------------
def test_the_thirteenth_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_smooth()
    assert list(abi.functions) == NAMES and L.SMOOTH.functions == abi.functions and L.SMOOTH.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_SMOOTH_LAUNCHES=2, TC_SMOOTH_TILE=64, TC_SMOOTH_MAX_WINDOW=63, TC_SMOOTH_WS_TILE=20)
    I, VP, LONG, D, U = C.c_int, C.c_void_p, C.c_long, C.c_double, C.c_uint
    assert abi.functions["tcw_smoothness"][:2] == (I, [VP, VP, I, I, I, D] + [VP] * 10)
    assert abi.functions["tcw_smooth_workspace"][:2] == (I, [I, I, I, VP])
    assert abi.functions["tcw_smooth"][:2] == (I, [VP, VP, I, I, I, I, VP, I, VP, U, VP, VP, VP, LONG] + [VP] * 8)
    assert abi.functions["tcw_smooth"][2][6] == "const double*" and abi.functions["tcw_smooth"][2][9] == "unsigned"
    with open(_abi.HEADER_SMOOTH) as f:
        text = f.read()
    flat = " ".join(text.replace("*", " ").split())
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text and "Not built" in text
    assert "choices, not measurements" in flat and 'mode="interp"' in flat and "one-euro" in flat
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_", "tcj_", "tck_", "tcg_", "tcp_", "tcf_", "tcm_", "tci_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_smooth.h", prefix=prefix)
    others = (L.ABI, L.EXT, L.GLTF, L.SKIN, L.SHADE, L.MJPEG, L.FOOTLOCK, L.GROUP, L.APART, L.GROUND, L.MESH, L.SELF)
    for names in [a.functions for a in others] + [L.EXPORTS]:
        assert not any(n.startswith("tcw_") for n in names)
    assert not any(k.startswith("TC_SMOOTH") for a in others for k in a.constants) and len(L.ABI.functions) == 79
    from tcdiff_amd import build
    assert os.path.join(ROOT, "tcdiff_amd", "csrc", "smooth.hip") in build.SRC and os.path.join(ROOT, "include", "tcdiff_smooth.h") in build.HDR
    assert os.path.join(ROOT, "tcdiff_amd", "csrc", "smooth_math.h") in build.HDR and S.MAX_WINDOW == 63


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    syms = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    assert sorted(s for s in syms if s.startswith("tcw_")) == sorted(NAMES)
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    n = C.c_long(-1)
    assert lib.tcw_smooth_workspace(2, 3, 10, C.addressof(n)) == 0 and n.value == 120
    assert lib.tcw_smooth_workspace(1, 1, 1, C.addressof(n)) == 0 and n.value == 24         # 20 rounded up to 24
    assert lib.tcw_smooth_workspace(2, 3, 10, None) == -1
    for bad in ((0, 3, 10), (2, 0, 10), (2, 3, 0), (2, 3, -1), (-1, 3, 10)):
        assert lib.tcw_smooth_workspace(*bad, C.addressof(n)) == -1, bad
    assert lib.tcw_smooth_workspace(2 ** 12, 2 ** 8, 2 ** 12, C.addressof(n)) == -4
    assert lib.tcw_smooth_workspace(2, 3, 130, C.addressof(n)) == 0 and n.value == 6 * 3 * 20          # three tiles a dancer
    parents, offsets = (C.c_int * 24)(*SMPL_PARENTS), (C.c_float * 72)(*[v for row in SMPL_OFFSETS for v in row])
    big = 1 << 40

    def call(q=p, pos=p, b=2, dn=3, T=10, window=9, taps=p, root_window=9, root_taps=p, mask=R.ALL, parents=parents, offsets=offsets, ws=p,
             ws_bytes=119, q_out=p, pos_out=p, joints=p, joints_in=p, max_rot=p, max_pos=p, copied=p):
        return lib.tcw_smooth(q, pos, b, dn, T, window, taps, root_window, root_taps, mask, parents, offsets, ws, ws_bytes, q_out, pos_out, joints,
                              joints_in, max_rot, max_pos, copied, None)
    assert call() == -1                                                    # good arguments but for one byte of workspace
    assert call(ws=p + 4, ws_bytes=120) == -2
    assert call(joints=None, joints_in=None) == -1 and call(joints=None, joints_in=None, ws=p + 4, ws_bytes=120) == -2      # these may be NULL
    for kw in (dict(taps=p + 4), dict(root_taps=p + 4), dict(max_rot=p + 4), dict(max_pos=p + 4)):
        assert call(ws_bytes=120, **kw) == -2, kw
    late = list(SMPL_PARENTS)
    late[3] = 5
    for kw in (dict(q=None), dict(pos=None), dict(taps=None), dict(root_taps=None), dict(parents=None), dict(offsets=None), dict(ws=None),
               dict(q_out=None), dict(pos_out=None), dict(max_rot=None), dict(max_pos=None), dict(copied=None), dict(b=0), dict(dn=0), dict(T=0),
               dict(T=-3), dict(window=8), dict(window=1), dict(window=65), dict(window=-9), dict(root_window=10), dict(root_window=65),
               dict(T=8), dict(window=5, root_window=11), dict(mask=1 << 24), dict(mask=2 ** 32 - 1), dict(parents=(C.c_int * 24)(*late))):
        assert call(**dict(dict(ws_bytes=big, ws=p + 4), **kw)) == -1, kw          # every one of them precedes the alignment check
    assert call(window=63, root_window=63, T=63, ws=p + 4, ws_bytes=big) == -2 and call(window=3, root_window=3, T=3, ws=p + 4, ws_bytes=big) == -2
    assert call(mask=0, ws=p + 4, ws_bytes=big) == -2                      # an empty mask is legal: the root alone
    # the order: a bad window before the size, the size before a parent and the workspace
    assert call(b=2 ** 12, dn=2 ** 8, T=2 ** 12, ws_bytes=big) == -4 and call(b=2 ** 12, dn=2 ** 8, T=2 ** 12, window=8, ws_bytes=big) == -1
    assert call(b=2 ** 12, dn=2 ** 8, T=2 ** 12, parents=(C.c_int * 24)(*late), ws_bytes=0) == -4

    strides = (C.c_long * 3)(2160, 720, 72)

    def score(joints=p, strides=strides, b=2, dn=3, T=10, fps=30.0, outs=(p,) * 9):
        return lib.tcw_smoothness(joints, strides, b, dn, T, fps, *outs, None)
    odd = lambda k, by: tuple(p + by if i == k else p for i in range(9))
    assert score(outs=odd(0, 4)) == -2 and score(outs=odd(5, 4)) == -2 and score(outs=odd(6, 2)) == -2 and score(outs=odd(8, 2)) == -2
    nan = float("nan")
    for kw in (dict(joints=None), dict(strides=None), dict(b=0), dict(dn=0), dict(T=3), dict(T=0), dict(fps=0.0), dict(fps=-30.0), dict(fps=nan),
               dict(fps=float("inf")), dict(fps=2e6), dict(strides=(C.c_long * 3)(2160, -720, 72))) + tuple(dict(outs=tuple(None if i == k else p for i in range(9))) for k in range(9)):
        assert score(**dict(dict(outs=odd(0, 4)), **kw)) == -1, kw         # every one of them precedes the alignment check
    assert score(b=2 ** 12, dn=2 ** 8, T=2 ** 12, outs=odd(0, 4)) == -4 and score(b=2 ** 12, dn=2 ** 8, T=2 ** 12, fps=nan) == -1
    assert score(b=2 ** 12, dn=2 ** 8, T=2 ** 12, strides=(C.c_long * 3)(-1, 0, 0)) == -4


def test_the_thirteenth_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.SMOOTH.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_smooth.h"', '#include "tcdiff_smooth.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "smooth.c", tmp_path / "smooth"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.SMOOTH.constants[n] for n in names]
    calls = ['#include "tcdiff_smooth.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.SMOOTH.functions.items():
        assert restype is C.c_int and argtypes == [C.c_void_p if c.endswith("*") else _abi.SCALARS[c] for c in ctexts], fname
        calls.append(f"  {{ int (*f)({', '.join(ctexts)}) = {fname}; (void)f; }}")
        zeros = [f"({c})0" if c.endswith("*") or c == "hipStream_t" else f"({c})z" for c in ctexts]
        calls.append(f"  (void){fname}({', '.join(zeros)});")
    calls.append("}")
    tu = tmp_path / "calls.c"
    tu.write_text("\n".join(calls))
    r = subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-c", str(tu), "-o", str(tmp_path / "calls.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- 5. the public interface -------------------------------------------------------------------------------------------------------------------
def test_smooth_and_smoothness_refuse_before_any_launch():
    import tcdiff_amd
    for name in ("smooth", "smoothness", "evaluate_smoothness", "savgol_table", "Smooth"):
        assert getattr(tcdiff_amd, name) is getattr(S, name) and name in tcdiff_amd.__all__
    sig = inspect.signature(S.smooth).parameters
    assert list(sig) == ["q", "pos", "dn", "window", "polyorder", "root_window", "root_polyorder", "joints_mask", "parents", "offsets", "measure"]
    assert [sig[k].default for k in list(sig)[3:]] == [9, 3, None, None, None, None, None, True]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[2:])
    sig = inspect.signature(S.smoothness).parameters
    assert list(sig) == ["joints", "fps"] and sig["fps"].default == 30 and sig["fps"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(S.evaluate_smoothness).parameters) == ["samples", "normalizer", "dn", "mode", "kw"]
    assert S.Smooth._fields == ("q", "pos", "joints", "max_rot_change", "max_pos_change", "copied", "window", "polyorder", "before", "after")
    q, pos = torch.zeros(2, 60, 24, 3), torch.zeros(2, 60, 3)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        S.smooth(q, pos, dn=3)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        S.smooth(q, pos, dn=3, window=5, polyorder=2, root_window=19, joints_mask=range(16, 24), measure=False)
    late = list(SMPL_PARENTS)
    late[3] = 5
    for bad, message in ((dict(window=8), "window must be an odd int"), (dict(window=65), "window must be an odd int"),
                         (dict(window=1), "window must be an odd int"), (dict(window=9.0), "window must be an odd int"),
                         (dict(window=True), "window must be an odd int"), (dict(polyorder=9), r"polyorder must be an int in \[0, window\)"),
                         (dict(polyorder=-1), "polyorder must be an int"), (dict(polyorder=2.0), "polyorder must be an int"),
                         (dict(window=3), r"polyorder must be an int in \[0, window\) = \[0, 3\), got 3"),
                         (dict(root_window=10), "root_window must be an odd int"), (dict(root_window=3), r"root_polyorder must be an int in \[0, root_window\)"),
                         (dict(root_polyorder=9), "root_polyorder must be an int"), (dict(window=21), "needs T >= 21, got T = 20"),
                         (dict(root_window=21), "needs T >= 21, got T = 20"), (dict(dn=7), "not a whole number of frames of 7 dancers"),
                         (dict(dn=0), "dancers"), (dict(dn=True), "dancers"), (dict(q=q[0]), "q must be"), (dict(q=q.double()), "q must be"),
                         (dict(q=q.numpy()), "must be tensors"), (dict(pos=pos[:, :59]), "pos must be"), (dict(pos=pos.double()), "pos must be"),
                         (dict(joints_mask=1 << 24), "joints_mask must be 24 bits, got 16777216"), (dict(joints_mask=-1), "joints_mask must be 24 bits"),
                         (dict(joints_mask=[24]), "joints_mask lists joints in 0 .. 23, got 24"), (dict(joints_mask=[True]), "joints_mask lists joints"),
                         (dict(joints_mask=1.5), "joints_mask must be 24 bits as an int"), (dict(parents=late), "every parent must precede its child"),
                         (dict(parents=SMPL_PARENTS[:5]), "24 joints"), (dict(offsets=SMPL_OFFSETS[:5]), "24 joints"), (dict(measure=1), "measure must be a bool")):
        kw = dict(q=q, pos=pos, dn=3)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match=r"^smooth: .*" + message):      # its own refusal, not "smooth runs on MI355X only"
            S.smooth(kw.pop("q"), kw.pop("pos"), **kw)
    with pytest.raises(L.TcdiffError, match=r"^smooth: measure=True .* got T = 3"):
        S.smooth(q[:, :9], pos[:, :9], dn=3, window=3, polyorder=1)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        S.smooth(q[:, :9], pos[:, :9], dn=3, window=3, polyorder=1, measure=False)
    with pytest.raises(L.TcdiffError, match=r"^smooth: .*more than 2\^31 - 1"):
        big = torch.zeros(1, 1, 24, 3).expand(2 ** 15, 3 * 2 ** 16, 24, 3)
        S.smooth(big, torch.zeros(1, 1, 3).expand(2 ** 15, 3 * 2 ** 16, 3), dn=3)
    for bad in ((5, 5), (4, 3), (9, -1), (65, 3), (9.0, 3)):
        with pytest.raises(L.TcdiffError, match="^savgol_table: "):
            S.savgol_table(*bad)
    J = torch.zeros(2, 3, 6, 24, 3)
    with pytest.raises(L.TcdiffError, match="smoothness runs on MI355X only"):
        S.smoothness(J)
    for bad, message in ((dict(joints=J[0]), "joints must be"), (dict(joints=J.double()), "float32"), (dict(joints=J.numpy()), "joints must be"),
                         (dict(joints=torch.zeros(2, 3, 6, 23, 3)), "joints must be"), (dict(joints=J[:, :, :3]), "a jerk takes 4 frames, got T = 3"),
                         (dict(joints=J[:0]), "empty"), (dict(joints=J.transpose(-1, -2).contiguous().transpose(-1, -2)), "contiguous"),
                         (dict(fps=0), "fps must be a number in"), (dict(fps=-30), "fps"), (dict(fps=float("nan")), "fps"),
                         (dict(fps=float("inf")), "fps"), (dict(fps=None), "fps"), (dict(fps=True), "fps")):
        kw = dict(joints=J)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match=r"^smoothness: .*" + message):
            S.smoothness(kw.pop("joints"), **kw)
    for doc in (S.__doc__, S.smooth.__doc__):
        assert "choices, not measurements" in " ".join(doc.split())
    flat = " ".join(S.__doc__.split())
    assert "unpinned" in flat and "Not built" in flat and "smooth_data" in flat and "one-euro" in flat


def test_render_sample_has_the_switch_and_says_what_it_does():
    from tcdiff_amd import GaussianDiffusion
    assert GaussianDiffusion.smooth is False and GaussianDiffusion.foot_lock is False
    doc = " ".join(GaussianDiffusion.render_sample.__doc__.split())
    assert "self.smooth" in doc and "tcdiff_amd/smooth.py" in doc
    src = inspect.getsource(GaussianDiffusion.render_sample)
    assert src.index("smooth(") < src.index("keep_apart(") < src.index("ground(") < src.index("foot_lock(")
