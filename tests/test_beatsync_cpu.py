"""CPU checks of the beat synchroniser (no GPU): the numpy restatement tests/beatsync_ref.py of include/tcdiff_beatsync.h -- the
properties a time warp needs (monotone, pinned ends, anchors hit bit for bit, the identity cases), its speed curve against scipy's
gaussian_filter1d, the matching, the tie rules, the rate bound and the closing back-off on hand-built cases, the seeded late dancers
under the numpy beat_align of tests/metrics_ref.py --, csrc/beatsync_math.h built for the host as a stand-alone program with the
address and undefined-behaviour sanitizers against the restatement, the fifteenth header and its binding, and the launchers' and the
Python side's refusals."""
import ctypes as C
import importlib
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import beatsync_ref as R
import metrics_ref as MR
import smooth_ref as SR
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L

B = importlib.import_module("tcdiff_amd.beat_sync")               # the package's attribute of this name is the function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcb_beat_sync_workspace", "tcb_motion_beats", "tcb_beat_sync"]
# the largest difference between the restatement's speed curve (ascending taps to 0.0) and scipy.ndimage.gaussian_filter1d (its own
# correlation order), relative to the curve's largest value, as printed by test_the_speed_curve_is_scipys_gaussian_filter and kept in
# profiles/beatsync.txt; the test allows 8 x this for the two summation orders
SPEED_REL = 5.6e-16
SHAPES = [(1, 1, 2), (1, 1, 4), (2, 3, 65), (1, 2, 257), (1, 3, 300)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


# ---- 1. what a time warp needs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_warp_is_monotone_pinned_and_hits_its_anchors(shape, share):
    b, dn, T = shape
    q, pos, contacts, beats = R.case(b, dn, T)
    out = R.beat_sync(q, pos, beats, dn, contacts=contacts, share=share)
    W = 1 if share else dn
    assert out["warp"].shape == (b, W, T) and out["speed"].shape == (b, W, T - 1) and out["kin"].shape == (b, W, T)
    J = R.joints_of(q, pos, dn)
    for c in range(b):
        music = [m for m in range(1, T - 1) if beats[c, m]]
        for w in range(W):
            warp = out["warp"][c, w]
            assert warp[0] == 0.0 and warp[T - 1] == float(T - 1) and np.all(np.diff(warp) >= 0.0)
            kin = [int(t) for t in np.nonzero(out["kin"][c, w])[0]]
            keys, vals, dropped = R.anchors(R.match(kin, music, 7), T, 1.0, 1.5)
            assert np.array_equal(bits(warp[keys]), bits(np.array(vals)))                              # every kept anchor, bit for bit
            assert out["anchors"][c, w] == len(keys) - 2 and out["matched"][c, w] == out["anchors"][c, w] + dropped
            assert out["kin_count"][c, w] == len(kin) and out["music_count"][c, w] == len(music) and out["status"][c, w] == 0
            if not share:                                                                              # beat_align's own minima
                assert np.array_equal(kin, MR.minima(MR.smooth(MR.speed(J[c, w]), 5.0))) or T < 4
    if T >= 65:
        assert out["anchors"].sum() > 0 and out["moved"].sum() > 0 and not np.array_equal(out["q"], q)
        assert out["copied"].sum() == 0


@pytest.mark.parametrize("what", ["strength0", "silent", "still", "T1", "T2", "T3"])
def test_the_identity_cases_return_the_input_bit_for_bit(what):
    T = dict(T1=1, T2=2, T3=3).get(what, 65)
    q, pos, contacts, beats = R.case(1, 2, T)
    kw = {}
    if what == "strength0":
        kw = dict(strength=0.0)
    if what == "silent":
        beats = np.zeros_like(beats)
    if what == "still":                                       # every frame the same pose: the speed is 0 and has no strict minimum
        q, pos = np.tile(q[:, :2], (1, T, 1, 1)), np.tile(pos[:, :2], (1, T, 1))
    for share in (True, False):
        out = R.beat_sync(q, pos, beats, 2, contacts=contacts, share=share, **kw)
        assert np.array_equal(out["warp"], np.broadcast_to(np.arange(T, dtype=np.float64), out["warp"].shape))
        for k, src in (("q", q), ("pos", pos), ("contacts", contacts)):
            assert np.array_equal(bits(out[k]), bits(src)), k
        assert not out["moved"].any() and not out["copied"].any() and not out["shift_max"].any() and not out["status"].any()
        if what == "strength0":
            assert out["anchors"].sum() > 0                   # anchors (m, m): the PCHIP through the diagonal is the diagonal, exactly
        if what in ("still", "T1", "T2", "T3"):
            assert not out["kin_count"].any() and not out["matched"].any()
        if T >= 2:
            assert np.all(out["rate_min"] == 1.0) and np.all(out["rate_max"] == 1.0) and not out["rate_min_frame"].any()
        else:
            assert np.isnan(out["rate_min"]).all() and np.all(out["rate_max_frame"] == -1)


def test_a_non_finite_speed_makes_the_warp_the_identity_and_touches_no_other_dancer():
    q, pos, contacts, beats = R.case(1, 3, 65)
    J = np.array(R.joints_of(q, pos, 3))
    clean = R.beat_sync(q, pos, beats, 3, contacts=contacts, share=False, joints_in=J)
    J[0, 1, 30, 5, 1] = np.nan
    out = R.beat_sync(q, pos, beats, 3, contacts=contacts, share=False, joints_in=J)
    assert out["status"].tolist() == [[0, 1, 0]] and np.isnan(out["speed"][0, 1]).all() and not out["kin"][0, 1].any()
    fq, fo = SR.frames_of(q, 3), SR.frames_of(out["q"], 3)
    assert np.array_equal(bits(fo[0, 1]), bits(fq[0, 1])) and np.array_equal(bits(out["contacts"][0, 1]), bits(contacts[0, 1]))
    for d in (0, 2):
        assert np.array_equal(bits(fo[0, d]), bits(SR.frames_of(clean["q"], 3)[0, d])) and np.array_equal(out["warp"][0, d], clean["warp"][0, d])
    pooled = R.beat_sync(q, pos, beats, 3, share=True, joints_in=J)
    assert pooled["status"].tolist() == [[1]] and np.array_equal(bits(pooled["q"]), bits(q)) and not pooled["moved"].any()


def test_outputs_with_a_non_finite_source_frame_are_copied_through():
    q, pos, _, beats = R.case(1, 1, 65)
    clean = R.beat_sync(q, pos, beats, 1)
    J = R.joints_of(q, pos, 1)                                # the speed of the clean poses, so that the warp stays
    q2, pos2 = np.array(q), np.array(pos)
    q2[0, 20, 4, 0] = np.nan
    pos2[0, 40, 2] = np.inf
    out = R.beat_sync(q2, pos2, beats, 1, joints_in=J)
    assert np.array_equal(out["warp"], clean["warp"])
    warp = out["warp"][0, 0]
    i, a = np.floor(warp).astype(int), warp - np.floor(warp)
    hit_q = (a != 0) & ((i == 20) | (i + 1 == 20))
    hit_p = (a != 0) & ((i == 40) | (i + 1 == 40))
    assert hit_q.sum() >= 1 and hit_p.sum() >= 1 and out["copied"][0, 0] == hit_q.sum() + hit_p.sum()
    assert np.array_equal(bits(out["q"][0, hit_q, 4]), bits(q2[0, hit_q, 4])) and np.array_equal(bits(out["pos"][0, hit_p]), bits(pos2[0, hit_p]))
    rest = np.ones_like(q2, bool)
    rest[0, hit_q, 4] = False
    rest[0, i[a == 0][i[a == 0] == 20], 4] = False            # a frame that copies source frame 20 carries its NaN
    assert np.array_equal(bits(out["q"][rest]), bits(clean["q"][rest]))


# ---- 2. the speed curve against scipy -------------------------------------------------------------------------------------------------------
def test_the_speed_curve_is_scipys_gaussian_filter():
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(7)
    worst = 0.0
    cases = [(f"N{n}-s{s}", g.uniform(0, 0.05, n), s) for n in (1, 2, 3, 7, 64, 149, 299, 1199) for s in (1.0, 5.0, 7.3)]
    q, pos, _, _ = R.case(1, 3, 300)
    cases += [(f"dance-{d}", R.speed_of(R.joints_of(q, pos, 3)[0, d]), 5.0) for d in range(3)]
    for name, v, sigma in cases:
        mine = R.filtered(v, R.gaussian_table(sigma))
        theirs = ndi.gaussian_filter1d(v, sigma, mode="reflect")
        err = float(np.abs(mine - theirs).max() / np.abs(v).max())
        print(f"[beatsync] speed {name}: {err:.2e} from scipy relative to the curve's largest value")
        worst = max(worst, err)
        assert err <= 8 * SPEED_REL, name
    print(f"[beatsync] speed: the largest difference is {worst:.2e} (SPEED_REL = {SPEED_REL:.1e}, the bound 8 x that)")
    assert np.array_equal(B.gaussian_table(5.0), R.gaussian_table(5.0)) and len(B.gaussian_table(5.0)) == 41
    assert abs(B.gaussian_table(7.3).sum() - 1.0) < 1e-15 and np.array_equal(B.gaussian_table(2), B.gaussian_table(2.0))


# ---- 3. hand-built cases, by value ----------------------------------------------------------------------------------------------------------------
def test_matching_ties_the_rate_bound_and_the_closing_back_off_by_hand():
    # two music beats claim one kinematic beat: the nearer keeps it, the other is unmatched and takes no second choice
    assert R.match([10, 30], [8, 11], 7) == [(11, 10)]
    assert R.match([10, 30], [8, 11, 25], 7) == [(11, 10), (25, 30)]
    # equal distance -> the lower k; equal claims -> the lower m
    assert R.match([10, 14], [12], 7) == [(12, 10)]
    assert R.match([10], [8, 12], 7) == [(8, 10)]
    assert R.match([10], [18], 7) == [] and R.match([10], [17], 7) == [(17, 10)] and R.match([], [5], 7) == []
    # strength scales the shift
    assert R.anchors([(20, 24)], 100, 0.5, 1.5) == ([0, 20, 99], [0.0, 22.0, 99.0], 0)
    # a candidate dropped by the rate bound: from (20, 24), (24, 31) needs a rate of 7 / 4
    keys, vals, dropped = R.anchors([(20, 24), (24, 31), (60, 57)], 100, 1.0, 1.5)
    assert (keys, vals, dropped) == ([0, 20, 60, 99], [0.0, 24.0, 57.0, 99.0], 1)
    # the first one refused against the fixed start: 6 / 3 = 2
    assert R.anchors([(3, 6)], 100, 1.0, 1.5) == ([0, 99], [0.0, 99.0], 1)
    # the back-off at the closing anchor: (95, 90) leaves a rate of 9 / 4 to the end, and after it (90, 83) one of 16 / 9
    keys, vals, dropped = R.anchors([(50, 50), (90, 83), (95, 90)], 100, 1.0, 1.5)
    assert (keys, vals, dropped) == ([0, 50, 99], [0.0, 50.0, 99.0], 2)
    keys, vals, dropped = R.anchors([(50, 50), (90, 88), (95, 90)], 100, 1.0, 1.5)
    assert (keys, vals, dropped) == ([0, 50, 90, 99], [0.0, 50.0, 88.0, 99.0], 1)
    assert R.anchors([(10, 10)], 100, 1.0, 1.0) == ([0, 10, 99], [0.0, 10.0, 99.0], 0) and R.anchors([(10, 11)], 100, 1.0, 1.0)[2] == 1
    # the warp through one anchor: the key frame is the value, the ends are pinned, the rate stays within PCHIP's overshoot-free range
    warp = R.warp_of([0, 20, 99], [0.0, 24.0, 99.0], 100)
    assert warp[20] == 24.0 and warp[0] == 0.0 and warp[99] == 99.0 and np.all(np.diff(warp) > 0)
    assert np.array_equal(R.warp_of([0, 99], [0.0, 99.0], 100), np.arange(100.0))
    # the contacts come from the nearer frame, the root is linear
    q = np.zeros((4, 24, 3), np.float32)
    pos = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 4], [3, 0, 0]])
    con = np.float32([[0] * 4, [1] * 4, [2] * 4, [3] * 4])
    _, _, p, c, moved, copied = R.resample_one(q, pos, con, np.array([0.0, 1.25, 2.5, 3.0]))
    assert p.tolist() == [[0, 0, 0], [1.25, 0, 1], [2.5, 0, 2], [3, 0, 0]] and c[:, 0].tolist() == [0, 1, 3, 3] and (moved, copied) == (2, 0)


def test_the_slerp_is_the_rotation_between_and_takes_the_short_way():
    axis = np.float32([0.6, 0.0, 0.8])
    qa, qb = np.tile(axis * np.float32(0.2), (24, 1)), np.tile(axis * np.float32(1.0), (24, 1))
    r = R.slerp(qa, qb, 0.25)
    assert np.abs(r - axis.astype(np.float64) * (0.2 + 0.25 * 0.8)).max() < 1e-7           # the same axis: the angle is interpolated
    near = R.slerp(qa, (qa * np.float32(1.01)).astype(np.float32), 0.5)                       # the linear fallback
    assert np.abs(near - qa.astype(np.float64) * 1.005).max() < 1e-6
    flip = np.tile(axis * np.float32(-(2 * np.pi - 1.0)), (24, 1)).astype(np.float32)         # the same rotation as qb, written the long way round
    assert np.abs(R.slerp(qa, flip, 0.25) - r).max() < 1e-6


# ---- 4. what it is for ----------------------------------------------------------------------------------------------------------------------------
def test_the_late_dancers_come_onto_the_beat():
    q, pos, beats, lags = R.late_dancers()
    dn, T = len(lags), beats.shape[1]
    for share in (False, True):
        out = R.beat_sync(q, pos, beats, dn, share=share)
        J0, J1 = R.joints_of(q, pos, dn), R.joints_of(out["q"], out["pos"], dn)
        music = np.nonzero(beats[0])[0]
        for d in range(dn):
            before, _, _, M0 = MR.beat_one(J0[0, d], beats[0], 5.0, 3.0)
            after, _, _, M1 = MR.beat_one(J1[0, d], beats[0], 5.0, 3.0)
            r0 = [int(np.abs(M0 - m).min()) for m in music]
            r1 = [int(np.abs(M1 - m).min()) for m in music]
            print(f"[beatsync] late dancer {d} (lag {lags[d]}, share={share}): beat_align {before:.3f} -> {after:.3f}, residual beat distances "
                  f"{r0} -> {r1} frames")
            assert after > before
        assert out["matched"].min() > 0 and out["anchors"].min() > 0 and out["moved"].min() > 0 and 3.0 <= out["shift_max"].max() <= 4.0


# ---- 5. csrc/beatsync_math.h on the host, under the sanitizers ---------------------------------------------------------------------------------
def run_host(exe, tmp, q, pos, beats, dn, contacts, share, max_shift, max_rate, strength, sigma, joints):
    b, T = q.shape[0], q.shape[1] // dn
    w = R.gaussian_table(sigma)
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([b, dn, T, share, max_shift, contacts is not None, (len(w) - 1) // 2], np.int32).tobytes() +
                np.array([max_rate, strength], np.float64).tobytes() + w.tobytes() + np.ascontiguousarray(beats, np.uint8).tobytes() +
                np.ascontiguousarray(joints, np.float32).tobytes() + np.ascontiguousarray(q, np.float32).tobytes() +
                np.ascontiguousarray(pos, np.float32).tobytes() + (b"" if contacts is None else np.ascontiguousarray(contacts, np.float32).tobytes()))
    r = subprocess.run([exe, str(tmp / "in.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    v = np.array([float(x) for x in r.stdout.split()])
    W = 1 if share else dn
    per = 11 + T + (T - 1) + T
    n = [b * W * per, b * dn * 2, b * T * dn * 72, b * T * dn * 3, 0 if contacts is None else b * dn * T * 4]
    assert v.size == sum(n)
    wp, mc, oq, op, oc = np.split(v, np.cumsum(n)[:-1])
    wp, mc = wp.reshape(b, W, per), mc.reshape(b, dn, 2)
    names = ("status", "kin_count", "music_count", "matched", "dropped", "anchors", "rate_min_frame", "rate_max_frame", "shift_max", "rate_min", "rate_max")
    out = {k: wp[..., i] for i, k in enumerate(names)}
    out.update(warp=wp[..., 11:11 + T], speed=wp[..., 11 + T:10 + 2 * T], kin=wp[..., 10 + 2 * T:], moved=mc[..., 0], copied=mc[..., 1],
               q=oq.astype(np.float32).reshape(q.shape), pos=op.astype(np.float32).reshape(pos.shape))
    if contacts is not None:
        out["contacts"] = oc.astype(np.float32).reshape(contacts.shape)
    return out


def test_beatsync_math_on_the_host_under_the_sanitizers_reproduces_the_restatement(tmp_path):
    """the SAME functions the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined: every decision
    (the integers, kin), warp, speed, the rates, pos and the contacts equal the restatement's (sqrt and the division are correctly
    rounded on both sides); the rotations pass through libm's acos, sin, cos and atan2 on one side and numpy's on the other, which may
    differ in the last bit of a double, so they are held to one float32 ulp at pi, 2^-22, where the two round apart"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "beatsync_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "beatsync_host.cpp")])
    runs = [(shape, share, with_c, {}) for shape in SHAPES for share, with_c in ((True, True), (False, False))]
    runs += [((1, 1, 1), True, True, {}), ((1, 2, 3), False, True, {}), ((1, 3, 300), False, True, dict(strength=0.5, max_shift=3, max_rate=1.2, sigma=3.0)),
             ((2, 3, 65), True, False, dict(strength=0.0)), ((1, 3, 65), False, True, dict(nan=True)), ("late", False, False, {}), ("late", True, False, {})]
    worst = 0.0
    for shape, share, with_c, kw in runs:
        if shape == "late":
            q, pos, beats, lags = R.late_dancers()
            b, dn, contacts = 1, len(lags), None
        else:
            b, dn, T = shape
            q, pos, contacts, beats = R.case(b, dn, T)
            contacts = contacts if with_c else None
        J = np.array(R.joints_of(q, pos, dn))
        q, pos = np.array(q), np.array(pos)
        if kw.get("nan"):
            J[0, 1, 30, 5, 1] = np.nan                        # a status of 1 beside good dancers
            q[0, 20 * dn + 2, 4, 0] = np.nan                  # and outputs copied through
            pos[0, 40 * dn, 2] = np.inf
        args = dict(max_shift=kw.get("max_shift", 7), max_rate=kw.get("max_rate", 1.5), strength=kw.get("strength", 1.0))
        sigma = kw.get("sigma", 5.0)
        got = run_host(exe, tmp_path, q, pos, beats, dn, contacts, share, sigma=sigma, joints=J, **args)
        ref = R.beat_sync(q, pos, beats, dn, contacts=contacts, share=share, sigma_smooth=sigma, joints_in=J, **args)
        for k, v in got.items():
            if k == "q":
                keep = np.isnan(ref["q"])
                assert np.array_equal(np.isnan(v), keep), (shape, share)
                err = float(np.abs(v.astype(np.float64) - ref["q"])[~keep].max())
                worst = max(worst, err)
                assert err <= 2.0 ** -22, (shape, share, err)
            elif v.dtype == np.float32:
                assert np.array_equal(np.isnan(v), np.isnan(ref[k])) and np.array_equal(bits(v)[~np.isnan(v)], bits(ref[k])[~np.isnan(v)]), (k, shape, share)
            else:
                assert np.array_equal(v, np.asarray(ref[k], np.float64), equal_nan=True), (k, shape, share)
    print(f"[beatsync] host build: rotations at most {worst:.2e} rad from the restatement (bound 2^-22 = {2.0 ** -22:.2e})")


# ---- 6. the fifteenth header ---------------------------------------------------------------------------------------------------------------------
def test_the_fifteenth_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_beatsync()
    assert list(abi.functions) == NAMES and L.BEATSYNC.functions == abi.functions and L.BEATSYNC.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_BEATSYNC_LAUNCHES=3, TC_BEATSYNC_TILE=64, TC_BEATSYNC_MAX_FRAMES=4096, TC_BEATSYNC_MAX_RADIUS=512,
                                 TC_BEATSYNC_WS_FRAME=12)
    I, VP, D, LG = C.c_int, C.c_void_p, C.c_double, C.c_long
    assert abi.functions["tcb_beat_sync_workspace"][:2] == (I, [I, I, I, VP])
    assert abi.functions["tcb_motion_beats"][:2] == (I, [VP, VP, I, I, I, I, I, VP, VP, LG, VP, VP, VP, VP])
    assert abi.functions["tcb_beat_sync"][:2] == (I, [VP] * 4 + [I] * 5 + [D, D, I] + [VP] * 4 + [LG] + [VP] * 22)
    with open(_abi.HEADER_BEATSYNC) as f:
        text = f.read()
    flat = " ".join(text.replace("*", " ").split())
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text and "Not built" in text and "Not promised" in text
    assert "choices, not measurements" in flat and "one lane's serial pass over at most T / 2 items" in flat and "No atomics" in flat
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_", "tcj_", "tck_", "tcg_", "tcp_", "tcf_", "tcm_", "tci_", "tcw_", "tcc_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_beatsync.h", prefix=prefix)
    others = (L.ABI, L.EXT, L.GLTF, L.SKIN, L.SHADE, L.MJPEG, L.FOOTLOCK, L.GROUP, L.APART, L.GROUND, L.MESH, L.SELF, L.SMOOTH, L.CHOREO)
    for names in [a.functions for a in others] + [L.EXPORTS]:
        assert not any(n.startswith("tcb_") for n in names)
    assert not any(k.startswith("TC_BEATSYNC") for a in others for k in a.constants) and len(L.ABI.functions) == 79
    from tcdiff_amd import build
    assert os.path.join(ROOT, "tcdiff_amd", "csrc", "beatsync.hip") in build.SRC and os.path.join(ROOT, "include", "tcdiff_beatsync.h") in build.HDR
    assert os.path.join(ROOT, "tcdiff_amd", "csrc", "beatsync_math.h") in build.HDR and B.MAX_FRAMES == 4096 >= 2 * 1200


def test_the_fifteenth_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.BEATSYNC.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_beatsync.h"', '#include "tcdiff_beatsync.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "beatsync.c", tmp_path / "beatsync"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.BEATSYNC.constants[n] for n in names]
    calls = ['#include "tcdiff_beatsync.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.BEATSYNC.functions.items():
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
    assert sorted(s for s in syms if s.startswith("tcb_")) == sorted(NAMES)
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    nan = float("nan")
    parents = (C.c_int * 24)(*([-1] + list(range(23))))
    offsets = (C.c_float * 72)()
    strides = (C.c_long * 3)(21600, 7200, 72)
    n = C.c_long(0)
    assert lib.tcb_beat_sync_workspace(2, 3, 150, C.byref(n)) == 0 and n.value == 2 * 3 * 150 * 12
    assert lib.tcb_beat_sync_workspace(1, 1, 1, C.byref(n)) == 0 and n.value == 16                        # rounded up to 8
    assert lib.tcb_beat_sync_workspace(2, 3, 150, None) == -1 and lib.tcb_beat_sync_workspace(0, 3, 150, C.byref(n)) == -1
    assert lib.tcb_beat_sync_workspace(2, 3, 4097, C.byref(n)) == -4 and lib.tcb_beat_sync_workspace(2 ** 20, 2 ** 10, 4096, C.byref(n)) == -4
    big = 2 * 3 * 150 * 12

    def beats(joints=p, strides=strides, b=2, dn=3, T=150, share=0, rad=20, weights=p, ws=p, ws_bytes=big, speed=p, kin=p, count=p):
        return lib.tcb_motion_beats(joints, strides, b, dn, T, share, rad, weights, ws, ws_bytes, speed, kin, count, None)
    odd = dict(speed=p + 4)                                               # every check before the alignment check must come first
    assert beats(**odd) == -2 and beats(weights=p + 4) == -2 and beats(ws=p + 4) == -2 and beats(count=p + 2) == -2 and beats(kin=p + 1, **odd) == -2
    for kw in (dict(joints=None), dict(strides=None), dict(weights=None), dict(ws=None), dict(speed=None), dict(kin=None), dict(count=None), dict(b=0),
               dict(dn=0), dict(T=0), dict(share=2), dict(share=-1), dict(rad=-1), dict(strides=(C.c_long * 3)(21600, -1, 72)), dict(ws_bytes=big - 1)):
        assert beats(**dict(odd, **kw)) == -1, kw
    assert beats(T=4097, ws_bytes=2 ** 40, **odd) == -4 and beats(rad=513, **odd) == -4 and beats(b=2 ** 20, dn=2 ** 10, T=4096, ws_bytes=2 ** 60, **odd) == -4
    assert beats(T=4097, share=2) == -1 and beats(T=4097, strides=(C.c_long * 3)(-1, 0, 0)) == -4 and beats(T=4097, ws_bytes=0) == -4   # the stated order

    def sync(q=p, pos=p, contacts=p, beats=p, b=2, dn=3, T=150, share=1, max_shift=7, max_rate=1.5, strength=1.0, rad=20, weights=p, parents=parents,
             offsets=offsets, ws=p, ws_bytes=big, q_out=p, pos_out=p, contacts_out=p, joints=p, joints_in=p, outs=(p,) * 16):
        return lib.tcb_beat_sync(q, pos, contacts, beats, b, dn, T, share, max_shift, max_rate, strength, rad, weights, parents, offsets, ws, ws_bytes,
                                 q_out, pos_out, contacts_out, joints, joints_in, *outs, None)
    # outs: warp, speed, kin, status, kin_count, music_count, matched, dropped, anchors, shift_max, rate_min, rate_max, rate_min_frame, rate_max_frame,
    # moved, copied
    off = lambda k, by: tuple(p + by if i == k else p for i in range(16))
    for k, by in ((0, 4), (1, 4), (3, 2), (4, 2), (5, 2), (6, 2), (7, 2), (8, 2), (9, 4), (10, 4), (11, 4), (12, 2), (13, 2), (14, 2), (15, 2)):
        assert sync(outs=off(k, by)) == -2, k
    assert sync(ws=p + 4) == -2 and sync(weights=p + 4) == -2
    odd = dict(outs=off(0, 4))
    assert sync(contacts=None, contacts_out=None, **odd) == -2 and sync(joints_in=None, **odd) == -2      # these may be NULL
    bad_parents = (C.c_int * 24)(*([-1, 1] + list(range(1, 23))))
    for kw in (dict(q=None), dict(pos=None), dict(beats=None), dict(weights=None), dict(parents=None), dict(offsets=None), dict(ws=None), dict(q_out=None),
               dict(pos_out=None), dict(joints=None), dict(contacts=None), dict(contacts_out=None), dict(b=0), dict(dn=0), dict(T=0), dict(share=2),
               dict(rad=-1), dict(max_shift=-1), dict(max_rate=0.99), dict(max_rate=nan), dict(max_rate=2e6), dict(strength=-0.1), dict(strength=1.1),
               dict(strength=nan), dict(parents=bad_parents), dict(ws_bytes=big - 1)) + \
            tuple(dict(outs=tuple(None if i == k else (p + 4 if i == 0 else p) for i in range(16))) for k in range(16)):
        assert sync(**dict(odd, **kw)) == -1, kw
    assert sync(T=4097, ws_bytes=2 ** 40, **odd) == -4 and sync(rad=513, **odd) == -4 and sync(b=2 ** 20, dn=2 ** 10, T=4096, ws_bytes=2 ** 60, **odd) == -4
    assert sync(T=4097, strength=nan) == -1 and sync(T=4097, parents=bad_parents) == -4 and sync(T=4097, ws_bytes=0) == -4               # the stated order
    assert sync(T=1, ws_bytes=72, **odd) == -2 and sync(T=4096, ws_bytes=2 * 3 * 4096 * 12, **odd) == -2


# ---- 7. the public interface -------------------------------------------------------------------------------------------------------------------
def test_motion_beats_and_beat_sync_refuse_before_any_launch():
    import tcdiff_amd
    from tcdiff_amd.diffusion import GaussianDiffusion
    for name in ("BeatSync", "beat_sync", "motion_beats", "gaussian_table"):
        assert getattr(tcdiff_amd, name) is getattr(B, name) and name in tcdiff_amd.__all__
    assert GaussianDiffusion.beat_sync is False
    sig = inspect.signature(B.beat_sync).parameters
    assert list(sig) == ["q", "pos", "beats", "dn", "contacts", "share", "max_shift", "max_rate", "strength", "sigma_smooth", "fps", "parents",
                         "offsets", "measure"]
    assert [sig[k].default for k in list(sig)[4:]] == [None, True, 7, 1.5, 1.0, 5.0, 30, None, None, True]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[3:])
    sig = inspect.signature(B.motion_beats).parameters
    assert list(sig) == ["joints", "fps", "sigma_smooth", "share"] and [sig[k].default for k in list(sig)[1:]] == [30, 5.0, False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[1:])
    assert B.BeatSync._fields == ("q", "pos", "joints", "contacts", "warp", "status", "kin_count", "music_count", "matched", "dropped", "anchors",
                                  "shift_max", "rate_min", "rate_min_frame", "rate_max", "rate_max_frame", "moved", "copied", "speed", "kin", "before",
                                  "after")
    q, pos, beats, con = torch.zeros(2, 30, 24, 3), torch.zeros(2, 30, 3), torch.zeros(2, 10, dtype=torch.uint8), torch.zeros(2, 3, 10, 4)
    with pytest.raises(L.TcdiffError, match="beat_sync runs on MI355X only"):
        B.beat_sync(q, pos, beats, dn=3, contacts=con)                      # inputs off the GPU
    for bad, message in ((dict(q=q[0]), r"q must be \(b, frames \* dancers, 24, 3\)"), (dict(q=q.double()), "q must be"), (dict(q=q.numpy()), "must be tensors"),
                         (dict(pos=pos[:, :29]), r"pos must be \(2, 30, 3\)"), (dict(pos=pos.double()), "pos must be"), (dict(dn=4), "not a whole number of frames"),
                         (dict(dn=0), "not a whole number"), (dict(dn=True), "not a whole number"), (dict(dn=3.0), "not a whole number"),
                         (dict(beats=beats[:, :9]), r"beats must be \(2, 10\) uint8"), (dict(beats=beats.bool()), "beats must be"),
                         (dict(contacts=con[:, :2]), r"contacts must be \(2, 3, 10, 4\)"), (dict(contacts=con.double()), "contacts must be"),
                         (dict(contacts=con.numpy()), "contacts must be"), (dict(share=1), "share must be a bool"), (dict(max_shift=-1), "max_shift must be an int"),
                         (dict(max_shift=2.0), "max_shift must be"), (dict(max_shift=True), "max_shift must be"), (dict(max_rate=0.9), r"max_rate must be a number in \[1"),
                         (dict(max_rate=float("nan")), "max_rate"), (dict(max_rate=None), "max_rate"), (dict(strength=1.5), r"strength must be a number in \[0, 1\]"),
                         (dict(strength=-0.1), "strength"), (dict(strength=float("nan")), "strength"), (dict(sigma_smooth=0), "sigma_smooth must be a positive number"),
                         (dict(sigma_smooth=float("inf")), "sigma_smooth"), (dict(sigma_smooth=200.0), "radius above TC_BEATSYNC_MAX_RADIUS = 512"),
                         (dict(fps=0), "fps must be a number in"), (dict(fps=None), "fps"), (dict(measure=1), "measure must be a bool"),
                         (dict(parents=[0] * 24), "every parent must precede"), (dict(parents=[-1] * 23), "24 joints"),
                         (dict(q=torch.zeros(1, 4097, 24, 3), pos=torch.zeros(1, 4097, 3), beats=torch.zeros(1, 4097, dtype=torch.uint8), dn=1, contacts=None),
                          "more than TC_BEATSYNC_MAX_FRAMES = 4096")):
        kw = dict(q=q, pos=pos, beats=beats, dn=3, contacts=con)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match=r"^beat_sync: .*" + message):          # its own refusal, not "runs on MI355X only"
            B.beat_sync(kw.pop("q"), kw.pop("pos"), kw.pop("beats"), **kw)
    J = torch.zeros(2, 3, 6, 24, 3)
    with pytest.raises(L.TcdiffError, match="motion_beats runs on MI355X only"):
        B.motion_beats(J)
    for bad, message in ((dict(joints=J[0]), "joints must be"), (dict(joints=J.double()), "joints must be float32"), (dict(joints=J.numpy()), "joints must be"),
                         (dict(joints=J[:, :, :0]), "empty dimension"), (dict(joints=J.transpose(-1, -2).contiguous().transpose(-1, -2)), "contiguous"),
                         (dict(fps=-1), "fps must be"), (dict(sigma_smooth=-1.0), "sigma_smooth must be"), (dict(share=0), "share must be a bool"),
                         (dict(joints=torch.zeros(1, 1, 4097, 24, 3)), "more than TC_BEATSYNC_MAX_FRAMES")):
        kw = dict(joints=J)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match=r"^motion_beats: .*" + message):
            B.motion_beats(kw.pop("joints"), **kw)
    for name in ("gaussian_table",):
        with pytest.raises(L.TcdiffError, match="^gaussian_table: sigma_smooth must be"):
            B.gaussian_table(0.0)
    for doc in (B.__doc__, B.beat_sync.__doc__):
        assert "choices, not measurements" in " ".join(doc.split())
    flat = " ".join(B.__doc__.split())
    assert "unpinned" in flat and "Not built" in flat and "Not promised" in flat and "keep_apart" in flat and "no counterpart" in flat
