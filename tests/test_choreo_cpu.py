"""CPU checks of the choreography planner (no GPU): the numpy restatement tests/choreo_ref.py of include/tcdiff_choreo.h against
scipy's PchipInterpolator, the properties a choreography needs from it (key frames and holds bit for bit, no overshoot, x_0 in the
layout and units of io), csrc/choreo_math.h built for the host as a stand-alone program with the address and undefined-behaviour
sanitizers against the restatement, the fourteenth header and its binding, the launchers' and the Python side's refusals, and the
formations."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import choreo_ref as R
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd import choreo as CH
from tcdiff_amd import io as tio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcc_plan", "tcc_trajectory_error"]
# the largest difference between the restatement (Hermite form) and scipy (power basis) over the cases below, relative to the points'
# scale, as printed by test_the_restatement_is_scipys_pchip and kept in profiles/choreo.txt; the test allows 8 x this for the two
# evaluation orders
PCHIP_REL = 8.3e-16


def scipy_cases():
    """(name, keys, y): counts 2, 3, 4 and 40 with uneven spacing and a spacing of one frame, holds, and the reversals of the end guards"""
    g = np.random.default_rng(2024)
    out = []
    for n in (2, 3, 4, 40):
        for rep in range(3):
            gaps = g.integers(1, 40, n - 1)
            gaps[g.integers(0, n - 1)] = 1                    # a spacing of one frame
            keys = np.concatenate([[0], np.cumsum(gaps)]) + int(g.integers(0, 5))
            out.append((f"n{n}-{rep}", keys, g.uniform(-3, 3, n).astype(np.float32)))
    out.append(("hold-middle", np.array([0, 30, 31, 90, 140]), np.float32([0.5, 2.0, 2.0, -1.0, -1.5])))
    out.append(("hold-first", np.array([0, 45, 60, 100]), np.float32([1.25, 1.25, -2.0, 0.5])))
    out.append(("hold-last", np.array([3, 45, 60, 100]), np.float32([1.0, -2.0, 0.75, 0.75])))
    out.append(("guard-zero-first", np.array([0, 10, 20]), np.float32([0.0, 1.0, 5.0])))          # the formula's sign is not the secant's: 0
    out.append(("guard-zero-last", np.array([0, 10, 20]), np.float32([5.0, 1.0, 0.0])))
    out.append(("guard-3m-first", np.array([0, 10, 20]), np.float32([0.0, 1.0, -9.0])))           # a reversal and |d| > 3 |m|: 3 m
    out.append(("guard-3m-last", np.array([0, 10, 20]), np.float32([-9.0, 1.0, 0.0])))
    return out


# ---- 1. the restatement against scipy -----------------------------------------------------------------------------------------------------------
def test_the_restatement_is_scipys_pchip():
    interp = pytest.importorskip("scipy.interpolate")
    worst = 0.0
    for name, keys, y in scipy_cases():
        d = R.slopes(keys, y)
        t = np.arange(int(keys[0]), int(keys[-1]) + 1)
        mine = np.array([R.evaluate(keys, y, d, int(f)) for f in t])
        theirs = interp.PchipInterpolator(keys.astype(np.float64), y.astype(np.float64))(t.astype(np.float64))
        err = float(np.abs(mine - theirs).max() / np.abs(y).max())
        print(f"[choreo] pchip {name}: {err:.2e} from scipy relative to the points' scale")
        worst = max(worst, err)
        assert err <= 8 * PCHIP_REL, name
    print(f"[choreo] pchip: the largest difference is {worst:.2e} (PCHIP_REL = {PCHIP_REL:.1e}, the bound 8 x that)")


def test_the_slopes_are_scipys_to_4_ulp():
    interp = pytest.importorskip("scipy.interpolate")
    for name, keys, y in scipy_cases():
        mine = np.array(R.slopes(keys, y))
        p = interp.PchipInterpolator(keys.astype(np.float64), y.astype(np.float64))
        theirs = p.c[2]                                       # the derivative at the left end of every segment, as stored
        assert np.all(np.abs(mine[:-1] - theirs) <= 4 * np.spacing(np.abs(theirs))), name
        find = getattr(interp.PchipInterpolator, "_find_derivatives", None)
        if find is not None:                                  # the last key's slope is stored nowhere: scipy's own routine, where it has one
            full = find(keys.astype(np.float64), y.astype(np.float64))
            assert np.all(np.abs(mine - full) <= 4 * np.spacing(np.abs(full))), name
    # the two end guards, both ends, by value
    assert R.slopes([0, 10, 20], [0.0, 1.0, 5.0])[0] == 0.0 and R.slopes([0, 10, 20], [5.0, 1.0, 0.0])[2] == 0.0
    assert R.slopes([0, 10, 20], [0.0, 1.0, -9.0])[0] == 3.0 * 0.1 and R.slopes([0, 10, 20], [-9.0, 1.0, 0.0])[2] == 3.0 * -0.1
    assert R.slopes([4], [2.0]) == [0.0] and R.slopes([4, 8], [2.0, 3.0]) == [0.25, 0.25]


# ---- 2. what a choreography needs from it -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,per_dancer", [((1, 1, 1, 1), False), ((1, 1, 2, 2), True), ((2, 3, 65, 3), True), ((1, 3, 150, 6), False),
                                              ((1, 2, 257, 256), False), ((1, 3, 300, 40), True)])
def test_key_frames_holds_and_overshoot(shape, per_dancer):
    b, dn, frames, K = shape
    keys, points, counts = R.case(b, dn, frames, K, seed=frames, per_dancer=per_dancer)
    out = R.plan(keys, points, frames, counts)
    assert not out["status"].any()
    for c in range(b):
        for d in range(dn):
            n, key = counts[c, d], (keys[c, d] if per_dancer else keys)
            traj = out["traj"][c, d]
            assert np.array_equal(traj[key[:n]].view(np.int32), points[c, d, :n].view(np.int32))          # a key frame is the point, bit for bit
            assert np.array_equal(traj[:key[0] + 1].view(np.int32), np.broadcast_to(points[c, d, 0], (key[0] + 1, 2)).view(np.int32))
            assert np.array_equal(traj[key[n - 1]:].view(np.int32), np.broadcast_to(points[c, d, n - 1], (frames - key[n - 1], 2)).view(np.int32))
            for k in range(n - 1):
                seg = traj[key[k]:key[k + 1] + 1]
                lo, hi = np.minimum(points[c, d, k], points[c, d, k + 1]), np.maximum(points[c, d, k], points[c, d, k + 1])
                if np.array_equal(lo, hi):                    # a hold: every frame is the point
                    assert np.array_equal(seg.view(np.int32), np.broadcast_to(lo, seg.shape).view(np.int32))
                assert np.all(seg >= lo - np.spacing(np.abs(lo))) and np.all(seg <= hi + np.spacing(np.abs(hi)))          # within one float32 ulp
    if K >= 4:
        assert np.array_equal(points[0, dn - 1, 1], points[0, dn - 1, 2])                                  # the case holds a formation


def test_x0_is_ios_layout_and_units():
    g = torch.Generator().manual_seed(5)
    data = torch.randn(400, 151, generator=g) * 2.0
    nrm = tio.Normalizer(data)
    b, dn, frames, K = 2, 3, 65, 5
    keys, points, counts = R.case(b, dn, frames, K, seed=9)
    scale, mn = nrm.scaler.scale_[[4, 5]].tolist(), nrm.scaler.min_[[4, 5]].tolist()
    out = R.plan(keys, points, frames, counts, scale=scale, min_=mn)
    wide = torch.zeros(b, dn, frames, 151)
    wide[..., 4:6] = torch.from_numpy(out["traj"])
    want = tio.x0_from_trajectory(nrm.normalize(wide)[..., 4:6]).numpy()
    got = out["x_0"]
    assert got.shape == want.shape == (b, frames * dn, 3) and got.dtype == np.float32 and not got[..., 2].any()
    # io rounds three times in float32 (traj, the product, the sum), the plan once from float64.  The ulp is that of x_0's range
    # [-1, 1], 2^-23: where traj scale_ + min_ cancels, io's error is set by its operands (below 1 + |min_|), not by the small result
    ulp = float(np.finfo(np.float32).eps)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"[choreo] x_0 against io: at most {float(diff.max() / ulp):.2f} float32 ulp (2^-23) apart, {int(out['clamped'].sum())} frames clamped")
    assert np.all(diff <= ulp)
    nav = tio.Normalizer(torch.randn(100, 3, generator=g) * 0.8)                                           # the Navigator's: columns 0 and 1
    o3 = R.plan(keys, points, frames, counts, scale=nav.scaler.scale_[:2].tolist(), min_=nav.scaler.min_[:2].tolist())
    first = o3["x_0"].reshape(b, frames, dn, 3).transpose(0, 2, 1, 3)[..., :2]
    tri = torch.zeros(b, dn, frames, 3)
    tri[..., :2] = torch.from_numpy(o3["traj"])
    diff = np.abs(first.astype(np.float64) - nav.normalize(tri)[..., :2].numpy())
    print(f"[choreo] x_0 against a 3-column normaliser: at most {float(diff.max() / ulp):.2f} float32 ulp apart, {int(o3['clamped'].sum())} frames clamped")
    assert np.all(diff <= ulp) and o3["clamped"].sum() > 0                                                # some waypoints lie outside this one's range
    metres = R.plan(keys, points, frames, counts)                                                          # without a normaliser: metres
    assert np.array_equal(metres["x_0"].reshape(b, frames, dn, 3)[..., :2].transpose(0, 2, 1, 3).view(np.int32), metres["traj"].view(np.int32))


def test_the_reports_of_the_restatement_by_hand():
    # one dancer walks 3 m along x in 10 frames, straight (two keys): every step 0.3 m, 9 m/s at 30 fps
    out = R.plan([0, 10], np.float32([[[[0, 0], [3, 0]]]]), 12, fps=30.0, max_speed=8.0)
    assert out["status"][0, 0] == 0 and out["too_fast"][0, 0] == 10 and out["speed_peak"][0, 0] in range(10)
    assert abs(out["path_length"][0, 0] - 3.0) < 1e-6 and abs(out["speed_max"][0, 0] - 9.0) < 1e-5
    # statuses: a repeated key, a key equal to frames, a count of 0, an infinite point; the padding is not looked at
    pts = np.float32([[[[0, 0], [1, 1], [2, 0]]] * 5])
    keys = np.array([[[0, 5, 5], [0, 5, 12], [0, 5, 9], [0, 5, 9], [0, 5, 5]]], np.int32)
    pts[0, 3, 1, 0] = np.inf
    pts[0, 4, 2] = np.nan
    out = R.plan(keys, pts, 12, counts=np.array([[3, 3, 0, 3, 2]], np.int32))
    assert out["status"].tolist() == [[1, 1, 1, 2, 0]] and np.isnan(out["traj"][0, :4]).all() and np.isfinite(out["traj"][0, 4]).all()
    assert np.isnan(out["x_0"].reshape(12, 5, 3)[:, :4, :2]).all() and not out["x_0"][..., 2].any()
    assert np.isnan(out["dist_min"][0, :6]).all() and (out["dist_min_frame"][0] == -1).all() and not out["too_close"].any()
    # ties: the lower frame
    two = R.plan([0, 4, 8, 12], np.float32([[[[0, 0], [1, 0], [1, 0], [2, 0]], [[0, 1], [1, 1], [1, 1], [2, 1]]]]), 13, min_distance=1.5)
    assert two["dist_min"][0, 0] == 1.0 and two["dist_min_frame"][0, 0] == 0 and two["too_close"][0, 0] == 13
    e = R.trajectory_error(np.zeros((1, 1, 3, 24, 3), np.float32), np.float32([[[[0.03, 0.04]] * 3]]))
    assert abs(e["traj_err_mean"][0, 0] - 0.05) < 1e-8 and e["traj_err_peak"][0, 0] == 0 and e["traj_frames"][0, 0] == 3


# ---- 3. csrc/choreo_math.h on the host, under the sanitizers ---------------------------------------------------------------------------------
def run_host(exe, tmp, keys, points, frames, counts, fps, norm, min_distance, max_speed):
    b, dn, K, _ = points.shape
    keys = np.asarray(keys, np.int32)
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([b, dn, K, frames, keys.ndim == 3, counts is not None, norm is not None], np.int32).tobytes() +
                np.array([fps, min_distance, max_speed], np.float64).tobytes() +
                np.array([0, 0, 0, 0] if norm is None else list(norm[0]) + list(norm[1]), np.float32).tobytes() + keys.tobytes() +
                (b"" if counts is None else np.asarray(counts, np.int32).tobytes()) + np.ascontiguousarray(points, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp / "in.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    v = np.array([float(x) for x in r.stdout.split()])
    P = dn * (dn - 1) // 2
    n = [b * dn * 6, b * dn * frames * 2, b * dn * frames * 3, b * P * 3]
    assert v.size == sum(n)
    rep, traj, x0, pr = np.split(v, np.cumsum(n)[:-1])
    rep, pr = rep.reshape(b, dn, 6), pr.reshape(b, P, 3)
    return dict(status=rep[..., 0], clamped=rep[..., 1], speed_max=rep[..., 2], speed_peak=rep[..., 3], too_fast=rep[..., 4],
                path_length=rep[..., 5], traj=traj.astype(np.float32).reshape(b, dn, frames, 2), x_0=x0.astype(np.float32).reshape(b, frames * dn, 3),
                dist_min=pr[..., 0], dist_min_frame=pr[..., 1], too_close=pr[..., 2])


def same(a, b):
    """equal values with NaN where NaN is; float32 arrays bit for bit"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32 and b.dtype == np.float32:
        return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.int32)[~np.isnan(a)], b.view(np.int32)[~np.isnan(b)])
    return np.array_equal(a.astype(np.float64), b.astype(np.float64), equal_nan=True)


def test_choreo_math_on_the_host_under_the_sanitizers_reproduces_the_restatement(tmp_path):
    """the SAME functions the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined: traj, x_0, the
    statuses and every report equal the restatement's (sqrt and the division are correctly rounded on both sides)"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "choreo_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "choreo_host.cpp")])
    norm = ([0.4, 0.55], [0.1, -0.2])
    for (b, dn, frames, K), per_dancer, nm in (((1, 1, 1, 1), False, None), ((1, 1, 2, 2), True, norm), ((2, 3, 65, 3), True, norm),
                                                ((1, 3, 150, 6), False, None), ((1, 2, 257, 256), False, norm), ((1, 3, 300, 40), True, norm)):
        keys, points, counts = R.case(b, dn, frames, K, seed=frames + 1, per_dancer=per_dancer)
        if dn == 3 and per_dancer:                            # a status of each kind beside the good dancers
            keys[0, 1, 1] = keys[0, 1, 0]
            points[0, 2, 0, 1] = np.inf
        got = run_host(exe, tmp_path, keys, points, frames, counts, 30.0, nm, 1.0, 2.0)
        ref = R.plan(keys, points, frames, counts, 30.0, None if nm is None else nm[0], None if nm is None else nm[1], 1.0, 2.0)
        for k, v in got.items():
            assert same(v, ref[k]), (k, (b, dn, frames, K))
    keys, points, _ = R.case(1, 2, 40, 4, seed=3, short=False)                                             # without counts
    got = run_host(exe, tmp_path, keys, points, 40, None, 25.0, norm, 0.5, 3.0)
    ref = R.plan(keys, points, 40, None, 25.0, norm[0], norm[1], 0.5, 3.0)
    assert all(same(v, ref[k]) for k, v in got.items())


# ---- 4. the fourteenth header --------------------------------------------------------------------------------------------------------------------
def test_the_fourteenth_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_choreo()
    assert list(abi.functions) == NAMES and L.CHOREO.functions == abi.functions and L.CHOREO.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_CHOREO_LAUNCHES=2, TC_CHOREO_TILE=256, TC_CHOREO_MAX_KEYS=256)
    I, VP, D = C.c_int, C.c_void_p, C.c_double
    assert abi.functions["tcc_plan"][:2] == (I, [VP, VP, I, VP, I, I, I, I, D, VP, VP, D, D] + [VP] * 12)
    assert abi.functions["tcc_trajectory_error"][:2] == (I, [VP, VP, VP, I, I, I, I] + [VP] * 6)
    with open(_abi.HEADER_CHOREO) as f:
        text = f.read()
    flat = " ".join(text.replace("*", " ").split())
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text and "Not built" in text
    assert "choices, not measurements" in flat and "PchipInterpolator" in flat and "Fritsch-Butland" in flat
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_", "tcj_", "tck_", "tcg_", "tcp_", "tcf_", "tcm_", "tci_", "tcw_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_choreo.h", prefix=prefix)
    others = (L.ABI, L.EXT, L.GLTF, L.SKIN, L.SHADE, L.MJPEG, L.FOOTLOCK, L.GROUP, L.APART, L.GROUND, L.MESH, L.SELF, L.SMOOTH)
    for names in [a.functions for a in others] + [L.EXPORTS]:
        assert not any(n.startswith("tcc_") for n in names)
    assert not any(k.startswith("TC_CHOREO") for a in others for k in a.constants) and len(L.ABI.functions) == 79
    from tcdiff_amd import build
    assert os.path.join(ROOT, "tcdiff_amd", "csrc", "choreo.hip") in build.SRC and os.path.join(ROOT, "include", "tcdiff_choreo.h") in build.HDR
    assert os.path.join(ROOT, "tcdiff_amd", "csrc", "choreo_math.h") in build.HDR and CH.MAX_KEYS == 256


def test_the_fourteenth_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.CHOREO.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_choreo.h"', '#include "tcdiff_choreo.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "choreo.c", tmp_path / "choreo"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.CHOREO.constants[n] for n in names]
    calls = ['#include "tcdiff_choreo.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.CHOREO.functions.items():
        assert restype is C.c_int and argtypes == [C.c_void_p if c.endswith("*") else _abi.SCALARS[c] for c in ctexts], fname
        calls.append(f"  {{ int (*f)({', '.join(ctexts)}) = {fname}; (void)f; }}")
        zeros = [f"({c})0" if c.endswith("*") or c == "hipStream_t" else f"({c})z" for c in ctexts]
        calls.append(f"  (void){fname}({', '.join(zeros)});")
    calls.append("}")
    tu = tmp_path / "calls.c"
    tu.write_text("\n".join(calls))
    r = subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-c", str(tu), "-o", str(tmp_path / "calls.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    syms = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    assert sorted(s for s in syms if s.startswith("tcc_")) == sorted(NAMES)
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    two = (C.c_float * 2)(1.0, 1.0)
    nan = float("nan")

    def plan(points=p, keys=p, per=0, counts=p, b=2, dn=3, K=6, frames=150, fps=30.0, scale=two, min_=two, near=0.5, fast=3.0, outs=(p,) * 11):
        return lib.tcc_plan(points, keys, per, counts, b, dn, K, frames, fps, scale, min_, near, fast, *outs, None)
    odd = lambda k, by, n=11: tuple(p + by if i == k else p for i in range(n))
    # outs: traj, x0, status, clamped, speed_max, speed_peak, too_fast, path_length, dist_min, dist_min_frame, too_close
    for k, by in ((2, 2), (3, 2), (4, 4), (5, 2), (6, 2), (7, 4), (8, 4), (9, 2), (10, 2)):
        assert plan(outs=odd(k, by)) == -2, k
    assert plan(counts=None, outs=odd(4, 4)) == -2 and plan(scale=None, min_=None, outs=odd(4, 4)) == -2          # these may be NULL
    for kw in (dict(points=None), dict(keys=None), dict(b=0), dict(dn=0), dict(K=0), dict(K=257), dict(frames=0), dict(frames=-1), dict(fps=0.0),
               dict(fps=nan), dict(fps=2e6), dict(near=-1.0), dict(near=nan), dict(fast=-1.0), dict(fast=nan), dict(scale=None), dict(min_=None)) + \
            tuple(dict(outs=tuple(None if i == k else (p + 4 if i == 4 else p) for i in range(11))) for k in range(11)):
        assert plan(**dict(dict(outs=odd(4, 4)), **kw)) == -1, kw         # every one of them precedes the alignment check
    assert plan(K=256, outs=odd(4, 4)) == -2
    assert plan(b=2 ** 12, dn=2 ** 8, frames=2 ** 12, outs=odd(4, 4)) == -4 and plan(b=2 ** 12, dn=2 ** 8, frames=2 ** 12, fps=nan) == -1
    assert plan(b=2 ** 20, dn=2 ** 7, frames=1, outs=odd(4, 4)) == -4                                      # the pairs alone are too many
    assert plan(b=2 ** 12, dn=2 ** 8, frames=2 ** 12, outs=(p,) * 8 + (None,) * 3) == -4                   # the size before the pair outputs
    assert plan(dn=1, outs=tuple(p + 4 if i == 4 else (None if i > 7 else p) for i in range(11))) == -2    # one dancer: no pair outputs needed

    strides = (C.c_long * 3)(2160, 720, 72)

    def err(joints=p, strides=strides, traj=p, b=2, dn=3, T=10, up=2, outs=(p,) * 5):
        return lib.tcc_trajectory_error(joints, strides, traj, b, dn, T, up, *outs, None)
    for k, by in ((0, 4), (1, 4), (2, 4), (3, 2), (4, 2)):
        assert err(outs=odd(k, by, 5)) == -2, k
    for kw in (dict(joints=None), dict(strides=None), dict(traj=None), dict(b=0), dict(dn=0), dict(T=0), dict(up=3), dict(up=-1),
               dict(strides=(C.c_long * 3)(2160, -720, 72))) + tuple(dict(outs=tuple(None if i == k else p for i in range(5))) for k in range(5)):
        assert err(**dict(dict(outs=odd(0, 4, 5)), **kw)) == -1, kw
    assert err(b=2 ** 12, dn=2 ** 8, T=2 ** 12, outs=odd(0, 4, 5)) == -4 and err(b=2 ** 12, dn=2 ** 8, T=2 ** 12, up=3) == -1
    assert err(b=2 ** 12, dn=2 ** 8, T=2 ** 12, strides=(C.c_long * 3)(-1, 0, 0)) == -4
    assert err(T=1, up=0, outs=odd(0, 4, 5)) == -2


# ---- 5. the public interface -------------------------------------------------------------------------------------------------------------------
class FakeNormalizer:
    def __init__(self, n):
        self.scaler = type("S", (), dict(scale_=torch.ones(n), min_=torch.zeros(n)))()


def test_plan_and_trajectory_error_refuse_before_any_launch():
    import tcdiff_amd
    for name in ("plan", "Plan", "trajectory_error", "formation"):
        assert getattr(tcdiff_amd, name) is getattr(CH, name) and name in tcdiff_amd.__all__
    sig = inspect.signature(CH.plan).parameters
    assert list(sig) == ["keys", "points", "frames", "counts", "fps", "normalizer", "columns", "min_distance", "max_speed", "out"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, 30, None, None, 0.5, 3.0, None]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[3:])
    sig = inspect.signature(CH.trajectory_error).parameters
    assert list(sig) == ["joints", "traj", "up"] and sig["up"].default == 2 and sig["up"].kind is inspect.Parameter.KEYWORD_ONLY
    assert CH.Plan._fields == ("traj", "x_0", "status", "clamped", "speed_max", "speed_peak", "too_fast", "path_length", "dist_min",
                               "dist_min_frame", "too_close", "columns")
    pts, keys = torch.zeros(2, 3, 4, 2), torch.tensor([0, 10, 20, 30], dtype=torch.int32)
    with pytest.raises(L.TcdiffError, match="runs on MI355X only"):
        CH.plan(keys, pts, 40)                                                  # an input off the GPU
    if not torch.cuda.is_available():
        with pytest.raises(L.TcdiffError, match="runs on MI355X only"):
            CH.plan([0, 10, 20, 30], pts.numpy(), 40, normalizer=FakeNormalizer(151), counts=[[4, 4, 3]] * 2)
    for bad, message in ((dict(points=pts[0]), r"points must be \(b, dn, K, 2\)"), (dict(points=pts.double()), "points must be float32"),
                         (dict(points=torch.zeros(2, 3, 4, 3)), "points must be"), (dict(points=pts[:0]), "points must be"),
                         (dict(points="line"), "points must"), (dict(points=np.zeros((2, 3, 4, 2), bool)), "real numbers"),
                         (dict(points=torch.zeros(1, 1, 257, 2), keys=torch.zeros(257, dtype=torch.int32)), "more than TC_CHOREO_MAX_KEYS = 256"),
                         (dict(keys=keys[:3]), r"keys must be \(4,\) or \(2, 3, 4\)"), (dict(keys=keys.long()), "keys must be int32"),
                         (dict(keys=[0.5, 1, 2, 3]), "keys must hold integers"), (dict(keys=[0, 1, 2, 2 ** 40]), "fit int32"),
                         (dict(counts=torch.ones(2, 2, dtype=torch.int32)), r"counts must be \(2, 3\)"),
                         (dict(counts=torch.ones(2, 3)), "counts must be int32"), (dict(frames=0), "frames must be an int >= 1"),
                         (dict(frames=40.0), "frames must be"), (dict(frames=True), "frames must be"), (dict(fps=0), "fps must be a number in"),
                         (dict(fps=2e6), "fps"), (dict(fps=float("nan")), "fps"), (dict(fps=None), "fps"),
                         (dict(min_distance=-1), "min_distance must be a number >= 0"), (dict(max_speed=float("nan")), "max_speed must be"),
                         (dict(normalizer=FakeNormalizer(5)), "too few columns"), (dict(normalizer=FakeNormalizer(2)), "too few columns"),
                         (dict(normalizer=FakeNormalizer(3), columns=(4, 5)), "too few columns"), (dict(normalizer=object()), "scaler"),
                         (dict(normalizer=FakeNormalizer(151), columns=(4,)), "columns must be two ints"), (dict(columns=(0, 1)), "columns without"),
                         (dict(out=torch.zeros(2, 119, 3)), r"out must be a contiguous float32 \(2, 120, 3\)"),
                         (dict(out=torch.zeros(2, 120, 3, dtype=torch.float64)), "out must be"), (dict(out=np.zeros((2, 120, 3), np.float32)), "out must be")):
        kw = dict(keys=keys, points=pts, frames=40)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match=r"^plan: .*" + message):          # its own refusal, not "plan runs on MI355X only"
            CH.plan(kw.pop("keys"), kw.pop("points"), kw.pop("frames"), **kw)
    J, T = torch.zeros(2, 3, 6, 24, 3), torch.zeros(2, 3, 6, 2)
    with pytest.raises(L.TcdiffError, match="trajectory_error runs on MI355X only"):
        CH.trajectory_error(J, T)
    for bad, message in ((dict(joints=J[0]), "joints must be"), (dict(joints=J.double()), "joints must be float32"), (dict(joints=J.numpy()), "joints must be"),
                         (dict(joints=J[:, :, :0]), "joints must be"), (dict(joints=J.transpose(-1, -2).contiguous().transpose(-1, -2)), "contiguous"),
                         (dict(traj=T[:, :, :5]), r"traj must be \(2, 3, 6, 2\)"), (dict(traj=T.double()), "traj must be float32"),
                         (dict(traj=T.numpy()), "traj must be"), (dict(up=3), "up must be 0, 1 or 2"), (dict(up=True), "up must be"), (dict(up=1.0), "up must be")):
        kw = dict(joints=J, traj=T)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match=r"^trajectory_error: .*" + message):
            CH.trajectory_error(kw.pop("joints"), kw.pop("traj"), **kw)
    for doc in (CH.__doc__, CH.plan.__doc__):
        assert "choices, not measurements" in " ".join(doc.split())
    flat = " ".join(CH.__doc__.split())
    assert "unpinned" in flat and "Not built" in flat and "PchipInterpolator" in flat and "keep_apart" in flat


# ---- 6. the formations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", [1, 2, 3, 5])
@pytest.mark.parametrize("name", ["line", "column", "circle", "v", "grid"])
def test_formations_are_centred_spaced_and_turned(name, dn):
    s, centre = 1.5, (2.0, -1.0)
    p = CH.formation(name, dn, spacing=s, center=centre)
    assert p.shape == (dn, 2) and p.dtype == np.float32
    assert np.abs(p.astype(np.float64).mean(0) - centre).max() <= 1e-6                                     # the centroid
    gap = lambda i, j: float(np.linalg.norm(p[i].astype(np.float64) - p[j]))
    if name in ("line", "column"):
        near = [(i, i + 1) for i in range(dn - 1)]
        axis = 0 if name == "line" else 1
        assert np.abs(p[:, 1 - axis] - centre[1 - axis]).max() <= 1e-6                                     # along one axis
    elif name == "circle":
        near = [(i, (i + 1) % dn) for i in range(dn)] if dn > 1 else []
        r = np.linalg.norm(p.astype(np.float64) - centre, axis=1)
        assert np.abs(r - r[0]).max() <= 1e-6
    elif name == "v":
        near = [(0, 1)] * (dn > 1) + [(0, 2)] * (dn > 2) + [(i, i + 2) for i in range(1, dn - 2)]          # along each arm
        assert all(p[0, 1] > p[i, 1] for i in range(1, dn))                                                # dancer 0 is the tip
    else:
        c = int(np.ceil(np.sqrt(dn)))
        near = [(i, i + 1) for i in range(dn - 1) if (i + 1) % c] + [(i, i + c) for i in range(dn - c)]    # along rows and columns
    assert all(abs(gap(i, j) - s) <= 1e-6 for i, j in near), (name, dn, [gap(i, j) for i, j in near])
    if dn > 1:
        assert len({tuple(np.round(q, 4)) for q in p}) == dn                                              # no two dancers on one spot
    a = 0.7
    turned = CH.formation(name, dn, spacing=s, center=centre, angle=a)
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    assert np.abs(turned - ((p.astype(np.float64) - centre) @ rot.T + centre)).max() <= 1e-6               # counter-clockwise about the centre
    for bad in (dict(name="ring"), dict(dn=0), dict(dn=True), dict(dn=2.0), dict(spacing=-1), dict(spacing="x"), dict(center=(0,)), dict(angle=float("nan"))):
        kw = dict(name=name, dn=dn)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match="^formation: "):
            CH.formation(kw.pop("name"), kw.pop("dn"), **kw)
