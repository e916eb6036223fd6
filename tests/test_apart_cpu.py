"""CPU checks of keeping the dancers apart (no GPU): the numpy restatement tests/apart_ref.py of include/tcdiff_apart.h on cases that
can be checked by hand and on the convergence the construction is for, the ninth header and its binding, the launchers' refusals,
csrc/apart_math.h built for the host as a stand-alone program with the address and undefined-behaviour sanitizers against the
restatement, render_sample's hook, and the condition the GPU comparison rests on: on the seeded inputs no decision is a near-tie."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import apart_ref as A
import group_ref as R
from group_ref import clip, stick_dancer
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd import apart as P
from tcdiff_amd.fk import SMPL_PARENTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcp_keep_apart_workspace", "tcp_keep_apart"]
RADII = R.capsule_radii()
THICK = np.full(24, 0.125)                                   # every capsule 1/8 m: two sticks D apart have the gap D - 1/4


def run(J, **kw):
    J = np.ascontiguousarray(J, np.float32)
    return A.keep_apart(A.pos_of(J), J, details=True, **kw)


def sticks(xa, xb, T=1):
    return clip(stick_dancer(xa, T=T), stick_dancer(xb, T=T))


# ---- cases that can be checked by hand -----------------------------------------------------------------------------------------------------------
def test_two_upright_parallel_bodies_are_pushed_apart_by_half_the_need_each():
    T, D, margin = 4, 0.25 + 1 / 64, 1 / 32                   # gap 1/64, need 1/64: 1/128 each, all exact in float32
    J = sticks(0.0, D, T)
    out = run(J, radii=THICK, margin=margin, iterations=1, rounds=1)
    assert (out["gap_before"] == 1 / 64).all() and (out["gap_after"] == margin).all()
    assert np.array_equal(out["shift"][0, 0], np.tile([-1 / 128, 0.0], (T, 1))) and np.array_equal(out["shift"][0, 1], np.tile([1 / 128, 0.0], (T, 1)))
    assert (out["joints"][0, 0, :, :, 0] == -1 / 128).all() and (out["joints"][0, 1, :, :, 0] == np.float32(D + 1 / 128)).all()
    assert out["pushed"][0, 0] == T and out["capped"][0, 0] == 0 and out["contact_before"][0, 0] == 0 == out["contact_after"][0, 0]
    assert np.array_equal(out["joints"][..., 1:].view(np.uint32), J[..., 1:].view(np.uint32))          # y and the `up` words
    assert np.array_equal(out["pos"], A.pos_of(out["joints"])) and (out["max_shift"] == 1 / 128).all() and (out["max_step"] == 0).all()
    # eight iterations find nothing more to do, three rounds neither: the first step was exact
    again = run(J, radii=THICK, margin=margin)
    assert np.array_equal(again["shift"], out["shift"]) and again["pushed"][0, 0] == T
    # a real contact: the sticks overlap by 1/8
    deep = run(sticks(0.0, 0.125, T), radii=THICK, margin=margin)
    assert (deep["gap_before"] == -0.125).all() and (deep["gap_after"] == margin).all() and deep["contact_before"][0, 0] == T
    assert deep["contact_after"][0, 0] == 0 and deep["gap_min_before"][0, 0] == -0.125 and deep["gap_min_after"][0, 0] == margin
    assert (deep["shift"][0, 1, :, 0] == (0.125 + margin) / 2).all() and (deep["shift"][0, :, :, 1] == 0).all()


def test_mobility_shares_the_push_and_two_pinned_dancers_are_left_alone():
    T, D, margin = 3, 0.25 + 1 / 64, 1 / 32
    J = sticks(0.0, D, T)
    out = run(J, radii=THICK, margin=margin, mobility=(0, 1))
    assert (out["shift"][0, 0] == 0).all() and (out["shift"][0, 1, :, 0] == 1 / 64).all() and (out["gap_after"] == margin).all()
    assert np.array_equal(out["joints"][0, 0].view(np.uint32), J[0, 0].view(np.uint32)) and out["max_shift"].tolist() == [[0.0, 1 / 64]]
    out = run(J, radii=THICK, margin=margin, mobility=(3, 1))
    assert (out["shift"][0, 0, :, 0] == -0.75 / 64).all() and (out["shift"][0, 1, :, 0] == 0.25 / 64).all()
    out = run(J, radii=THICK, margin=margin, mobility=(0, 0))
    assert (out["shift"] == 0).all() and out["pushed"][0, 0] == 0 and (out["gap_before"] == 1 / 64).all() and (out["gap_after"] == 1 / 64).all()
    assert np.array_equal(out["joints"].view(np.uint32), J.view(np.uint32))
    three = clip(stick_dancer(0.0, T=T), stick_dancer(D, T=T), stick_dancer(4.0, T=T))          # the pinned pair beside a free dancer
    out = run(three, radii=THICK, margin=margin, mobility=(0, 0, 1))
    assert (out["shift"] == 0).all() and out["pushed"].tolist() == [[0, 0, 0]]


def test_coincident_roots_take_the_fallback_direction():
    out = run(sticks(0.5, 0.5), radii=THICK, margin=1 / 32, max_push=1.0)
    assert out["gap_before"][0, 0, 0] == -0.25 and out["shift"][0, :, 0].tolist() == [[-(0.25 + 1 / 32) / 2, 0.0], [(0.25 + 1 / 32) / 2, 0.0]]
    J = sticks(0.5, 0.5)
    J[0, 0, :, :, 1] = 2.0 ** -31                             # a root distance of 2^-31: its square is below 1e-18
    out = run(J, radii=THICK, margin=1 / 32, max_push=1.0, iterations=1, rounds=1)
    assert out["shift"][0, 1, 0].tolist() == [(0.25 + 1 / 32 - 2.0 ** -31) / 2, 0.0]          # along x, across the root line
    J[0, 0, :, :, 1] = 2.0 ** -20                             # above it: the push follows the root line, along -y
    out = run(J, radii=THICK, margin=1 / 32, max_push=1.0, iterations=1, rounds=1)
    assert out["shift"][0, 1, 0, 0] == 0.0 and out["shift"][0, 1, 0, 1] < -0.14


def test_a_pair_too_deep_is_capped_at_exactly_max_push():
    T = 2
    out = run(sticks(0.0, 1 / 64, T), radii=THICK, margin=1 / 32, max_push=1 / 8, rounds=1)
    assert out["capped"][0, 0] == T and out["pushed"][0, 0] == T and (out["shift"][0, 1, :, 0] == 1 / 16).all() and (out["shift"][0, 0, :, 0] == -1 / 16).all()
    assert (out["gap_after"] == (1 / 64 + 1 / 8) - 0.25).all() and out["contact_after"][0, 0] == T
    assert out["gap_min_after"][0, 0] > out["gap_min_before"][0, 0] and out["max_shift"].tolist() == [[1 / 16, 1 / 16]]
    out = run(sticks(0.0, 1 / 64, T), radii=THICK, margin=1 / 32, max_push=1 / 8, rounds=2)          # capped again: the gap is now 1/64
    assert out["capped"][0, 0] == T and (out["shift"][0, 1, :, 0] == 1 / 8).all() and (out["gap_after"] == 1 / 64).all()
    out = run(sticks(0.0, 1 / 64, T), radii=THICK, margin=1 / 32, max_push=1 / 8, rounds=3)          # the third round finishes: 1/64 more
    assert out["capped"][0, 0] == T and (out["shift"][0, 1, :, 0] == 1 / 8 + 1 / 128).all() and (out["gap_after"] == 1 / 32).all()
    assert out["contact_after"][0, 0] == 0 and out["pushed"][0, 0] == T


def test_a_single_contact_frame_gives_the_tent():
    T, t0, blend, D = 21, 9, 3, 0.5
    b = stick_dancer(D, T=T)
    b[t0, :, 0] = 0.25 - 1 / 16                               # one frame of contact: gap -1/16, m = 1/16 + 1/32
    m = 1 / 16 + 1 / 32
    out = run(clip(stick_dancer(0.0, T=T), b), radii=THICK, margin=1 / 32, blend=blend, rounds=1)
    want = np.array([m * (1 - abs(t - t0) / (blend + 1)) if abs(t - t0) <= blend else 0.0 for t in range(T)])
    assert np.array_equal(out["shift"][0, 1, :, 0], want / 2) and np.array_equal(out["shift"][0, 0, :, 0], -want / 2)
    assert out["pushed"][0, 0] == 1 and out["max_step"][0, 1] == m / 2 / (blend + 1) and out["max_shift"][0, 1] == m / 2
    still = want == 0
    assert still.sum() == T - 2 * blend - 1
    J = clip(stick_dancer(0.0, T=T), b)
    assert np.array_equal(out["joints"][0, :, still].view(np.uint32), J[0, :, still].view(np.uint32))
    assert np.array_equal(A.envelope(np.eye(1, T, t0)[0] * m, blend), want)
    flat = run(clip(stick_dancer(0.0, T=T), b), radii=THICK, margin=1 / 32, blend=0, rounds=1)          # blend = 0: e = m
    assert np.array_equal(flat["shift"][0, 1, :, 0], np.eye(1, T, t0)[0] * m / 2)
    m2 = np.array([0.0, 0.5, 0.0, 0.0, 0.25, 0.0])
    assert np.array_equal(A.envelope(m2, 0), m2) and np.array_equal(A.envelope(m2, 1), [0.25, 0.5, 0.25, 0.125, 0.25, 0.125])
    assert (A.envelope(m2, 50) >= m2).all() and A.envelope(m2, 50)[0] == 0.5 * (1 - 1 / 51)          # blend past the clip's ends


def test_without_contact_and_without_rounds_the_input_comes_back_bit_for_bit():
    pos, J = A.spread(1, 2, 7)
    for kw in (dict(), dict(rounds=0)):
        out = A.keep_apart(pos, J, **kw)
        assert np.array_equal(out["joints"].view(np.uint32), J.view(np.uint32)) and np.array_equal(out["pos"].view(np.uint32), pos.view(np.uint32))
        assert (out["shift"] == 0).all() and out["pushed"].sum() == 0 and (out["max_shift"] == 0).all() and (out["max_step"] == 0).all()
        assert np.array_equal(out["gap_min_before"], out["gap_min_after"]) and (out["gap_min_before"] > 0.02).all()
    pos, J = A.spread(2, 3, 5, by=0.0)                        # dancers in contact, and no round: counted, not moved
    out = A.keep_apart(pos, J, rounds=0)
    assert np.array_equal(out["joints"].view(np.uint32), J.view(np.uint32)) and out["contact_before"].sum() > 0
    assert np.array_equal(out["contact_before"], out["contact_after"]) and np.array_equal(out["gap_min_before"], out["gap_min_after"])
    ref = R.group_metrics(J)
    assert np.array_equal(out["contact_before"], np.rint(ref["body_contact_rate"] * 5)) and np.array_equal(out["gap_min_before"], ref["body_gap_min"])


def test_a_nan_joint_is_neither_pushed_nor_changed():
    T, t0 = 5, 2
    J = sticks(0.0, 0.125, T)
    J.view(np.uint32)[0, 0, t0, 7, 1] = 0x7FC12345          # a NaN with a payload
    out = run(J, radii=THICK, margin=1 / 32, blend=0)
    assert np.isnan(out["gap_before"][0, 0, t0]) and np.isnan(out["gap_after"][0, 0, t0]) and out["pushed"][0, 0] == T - 1
    assert (out["shift"][0, :, t0] == 0).all() and np.array_equal(out["joints"][0, :, t0].view(np.uint32), J[0, :, t0].view(np.uint32))
    assert out["contact_before"][0, 0] == T - 1 and out["contact_after"][0, 0] == 0 and out["gap_min_after"][0, 0] == 1 / 32
    out = run(J, radii=THICK, margin=1 / 32, blend=2)         # inside its neighbours' envelope the frame moves; the NaN stays a NaN
    assert out["flags"][0, 0].tolist() == [1, 1, 0, 1, 1] and (out["shift"][0, 1, t0] != 0).any()
    assert np.isnan(out["joints"][0, 0, t0, 7, 1]) and np.isnan(out["joints"]).sum() == 1
    J[0, 0, :, 7, 1] = np.nan                                 # in every frame: nothing to go by
    out = run(J, radii=THICK, margin=1 / 32)
    assert np.isnan(out["gap_min_before"][0, 0]) and np.isnan(out["gap_min_after"][0, 0]) and out["pushed"][0, 0] == 0
    assert out["contact_before"][0, 0] == 0 and np.array_equal(out["joints"].view(np.uint32), J.view(np.uint32))


def test_a_single_frame():
    out = run(sticks(0.0, 0.125, 1), radii=THICK, margin=1 / 32)
    assert out["shift"].shape == (1, 2, 1, 2) and out["max_step"].tolist() == [[0.0, 0.0]] and out["gap_after"][0, 0, 0] == 1 / 32
    assert out["max_shift"].tolist() == [[(0.125 + 1 / 32) / 2] * 2] and out["pushed"][0, 0] == 1


def test_another_axis_up_moves_the_other_two_components():
    pos, J = A.spread(2, 3, 5, by=0.0)
    base = A.keep_apart(pos, J)
    for up in (0, 1):
        p2, J2 = A.permuted(pos, J, up)
        out = A.keep_apart(p2, J2, up=up)
        back = {0: [1, 2, 0], 1: [0, 2, 1]}[up]
        # the distance's dot products add the components in another order: the same shift up to the last places
        assert np.abs(out["joints"][..., back] - base["joints"]).max() <= 2e-7 and np.abs(out["pos"][..., back] - base["pos"]).max() <= 2e-7
        assert np.abs(out["shift"] - base["shift"]).max() <= 1e-12 and np.array_equal(out["joints"][..., up].view(np.uint32), J2[..., up].view(np.uint32))


# ---- what the construction is for --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 70), (2, 3, 150)], ids=lambda s: "x".join(map(str, s)))
def test_dancers_that_meet_now_and_then_are_kept_apart(shape):
    """group_ref.synth with dancer d moved 0.8 d metres along x, at the defaults.  A throw-away prototype of the definition gave
    24 -> 0 contact frames on the first input and 44 -> 2 on the second, its deepest gap -0.093 -> -0.015 m"""
    pos, J = A.spread(*shape)
    out = A.keep_apart(pos, J)
    before, after = int(out["contact_before"].sum()), int(out["contact_after"].sum())
    roots = np.linalg.norm(np.diff(J[:, :, :, 0].astype(np.float64), axis=2), axis=-1).max()
    print(f"[apart] {shape}: contact frames {before} -> {after}, deepest gap {np.nanmin(out['gap_min_before']):.4f} -> "
          f"{np.nanmin(out['gap_min_after']):.4f} m, largest shift {out['max_shift'].max():.4f} m, largest step {out['max_step'].max():.4f} m "
          f"a frame (the roots' own: {roots:.4f}), capped {int(out['capped'].sum())}")
    assert before > 0 and after <= before / 10
    touched = out["contact_before"] > 0
    assert touched.any() and (out["gap_min_after"][touched] > out["gap_min_before"][touched]).all()
    assert abs(before - {(1, 5, 70): 24, (2, 3, 150): 44}[shape]) <= 2 and abs(after - {(1, 5, 70): 0, (2, 3, 150): 2}[shape]) <= 2
    assert out["capped"].sum() == 0


def test_dancers_that_walk_through_each_other_are_helped_but_not_repaired():
    """the unspread inputs: the prototype gave 407 -> 24 contact frames with steps of up to 0.30 m; no small shift repairs that"""
    pos, J = A.spread(2, 3, 150, by=0.0)
    out = A.keep_apart(pos, J, details=True)
    before, after = int(out["contact_before"].sum()), int(out["contact_after"].sum())
    print(f"[apart] unspread (2, 3, 150): contact frames {before} -> {after}, capped {int(out['capped'].sum())}, largest step "
          f"{out['max_step'].max():.3f} m")
    assert out["capped"].sum() > 0 and 0 < after < before
    # the statistics agree with the planes and with each other
    assert np.array_equal(out["contact_before"], (out["gap_before"] < 0).sum(-1)) and np.array_equal(out["contact_after"], (out["gap_after"] < 0).sum(-1))
    assert np.array_equal(out["gap_min_before"], out["gap_before"].min(-1)) and np.array_equal(out["gap_min_after"], out["gap_after"].min(-1))
    assert (out["capped"] <= out["pushed"]).all() and (out["pushed"] >= out["contact_before"]).all() and (out["pushed"] <= 150).all()
    S = out["shift"]
    assert np.array_equal(out["max_shift"], np.sqrt(S[..., 0] ** 2 + S[..., 1] ** 2).max(-1)) and (out["max_step"] <= 2 * out["max_shift"]).all()
    assert (out["max_shift"] <= 3 * 2 * 0.6).all()            # three rounds, two partners, max_push each at the most
    ref = R.group_metrics(out["joints"])
    assert np.array_equal(ref["body_contact_rate"], out["contact_after"] / 150) and np.array_equal(ref["body_gap_min"], out["gap_min_after"])
    moved = (S != 0).any(-1)
    assert np.array_equal(out["joints"][~moved].view(np.uint32), J[~moved].view(np.uint32)) and moved.any() and not moved.all()


# ---- what the GPU comparison rests on ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", [A.SPREAD, 0.0], ids=["spread", "unspread"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_decision_is_a_near_tie_on_the_seeded_inputs(shape, by):
    ok, why = A.decisions_clear(*A.spread(*shape, by=by))
    assert ok, why


def test_no_decision_is_a_near_tie_with_other_parameters():
    for name, (pos, J), kw in A.parameter_cases():
        ok, why = A.decisions_clear(pos, J, **kw)
        assert ok, (name, why)
    pos, clean = A.spread(2, 3, 5, by=0.0)                    # the GPU test's input with a NaN joint
    J = clean.copy()
    J.view(np.uint32)[1, 0, 2, 20, 1] = 0x7FC12345
    ok, why = A.decisions_clear(pos, J, blend=0)
    assert ok, why


def test_the_guard_sees_a_near_tie():
    J = sticks(0.0, 0.25 + 1 / 32 + 2.0 ** -32, 2)            # a gap a quarter of a nanometre above the margin
    ok, why = A.judge(run(J, radii=THICK, margin=1 / 32))
    assert not ok and "need" in why[0]
    ok, why = A.judge(run(sticks(0.0, 0.125 + 2.0 ** -32, 2), radii=THICK, margin=1 / 32, max_push=0.125 + 1 / 32))
    assert not ok and any("max_push" in w for w in why)
    assert A.judge(run(sticks(0.0, 0.125, 2), radii=THICK, margin=1 / 32))[0]


# ---- csrc/apart_math.h on the host, under the sanitizers ---------------------------------------------------------------------------------------
def run_host(exe, tmp, pos, J, up=2, radii=None, parents=None, margin=0.02, iterations=8, rounds=3, blend=5, max_push=0.6, mobility=None):
    dn, T = J.shape[:2]
    radii = RADII if radii is None else radii
    parents = SMPL_PARENTS if parents is None else parents
    mobility = np.ones(dn) if mobility is None else mobility
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([dn, T, up, iterations, rounds, blend], np.int32).tobytes() +
                np.array([margin, max_push] + list(radii) + list(mobility), np.float64).tobytes() + np.array(parents, np.int32).tobytes() +
                np.ascontiguousarray(pos, np.float32).tobytes() + np.ascontiguousarray(J, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = (tmp / "out.bin").read_bytes()
    npairs = dn * (dn - 1) // 2
    nd = dn * T * 2 + npairs * 3 * T
    d = np.frombuffer(raw[:8 * nd], np.float64)
    fl = np.frombuffer(raw[8 * nd:], np.float32)
    planes = d[dn * T * 2:].reshape(npairs, 3, T)
    return dict(shift=d[:dn * T * 2].reshape(dn, T, 2), before=planes[:, 0], after=planes[:, 1], flags=planes[:, 2].astype(np.int64),
                pos=fl[:T * dn * 3].reshape(T * dn, 3), joints=fl[T * dn * 3:].reshape(dn, T, 24, 3))


def compare_host(out, ref, c=0):
    assert np.array_equal(out["flags"], ref["flags"][c])
    worst = float(np.abs(out["shift"] - ref["shift"][c]).max())
    for mine, theirs in ((out["before"], ref["gap_before"][c]), (out["after"], ref["gap_after"][c])):
        assert np.array_equal(np.isnan(mine), np.isnan(theirs))
        if (~np.isnan(theirs)).any():
            worst = max(worst, float(np.nanmax(np.abs(mine - theirs))))
    assert worst <= 1e-12, worst
    assert np.array_equal(out["joints"].view(np.uint32), ref["joints"][c].view(np.uint32))
    assert np.array_equal(out["pos"].view(np.uint32), ref["pos"][c].view(np.uint32))
    return worst


def test_apart_math_on_the_host_under_the_sanitizers_agrees_with_the_restatement(tmp_path):
    """the SAME functions the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "apart_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "apart_host.cpp")])
    worst = 0.0
    for shape, by in [((1, 2, 1), 0.0), ((1, 2, 2), 0.0), ((1, 2, 7), 0.0), ((1, 2, 7), A.SPREAD), ((2, 3, 5), A.SPREAD), ((2, 3, 5), 0.0),
                      ((1, 5, 70), A.SPREAD)]:
        pos, J = A.spread(*shape, by=by)
        ref = A.keep_apart(pos, J, details=True)
        for c in range(shape[0]):
            worst = max(worst, compare_host(run_host(exe, tmp_path, pos[c], J[c]), ref, c))
    for name, (pos, J), kw in A.parameter_cases():
        ref = A.keep_apart(pos, J, details=True, **kw)
        for c in range(J.shape[0]):
            worst = max(worst, compare_host(run_host(exe, tmp_path, pos[c], J[c], **kw), ref, c))
    nan = sticks(0.0, 0.125, 5)                               # exact cases: a NaN joint, coincident roots, a capped pair, a pinned dancer
    nan.view(np.uint32)[0, 0, 2, 7, 1] = 0x7FC12345
    for J, kw in ((nan, dict(blend=0)), (nan, dict(blend=2)), (sticks(0.5, 0.5, 2), dict(max_push=1.0)), (sticks(0.0, 1 / 64, 2), dict(max_push=1 / 8)),
                  (sticks(0.0, 0.125, 3), dict(mobility=(0, 1))), (sticks(0.0, 0.125, 3), dict(mobility=(0, 0)))):
        J = np.ascontiguousarray(J, np.float32)
        kw = dict(kw, radii=THICK, margin=1 / 32)
        worst = max(worst, compare_host(run_host(exe, tmp_path, A.pos_of(J)[0], J[0], **kw), A.keep_apart(A.pos_of(J), J, details=True, **kw)))
    print(f"[apart] host build against the restatement: {worst:.3e} at most (bound 1e-12)")


# ---- the ninth header --------------------------------------------------------------------------------------------------------------------------
def test_the_ninth_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_apart()
    assert list(abi.functions) == NAMES and L.APART.functions == abi.functions and L.APART.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_APART_MAX_DANCERS=32, TC_APART_MAX_BLEND=65536, TC_APART_MAX_ROUNDS=64, TC_APART_WS_PAIR_FRAME=41,
                                 TC_APART_WS_DANCER_FRAME=16, TC_APART_PUSHED=1, TC_APART_CAPPED=2)
    I, VP, LONG, D = C.c_int, C.c_void_p, C.c_long, C.c_double
    assert abi.functions["tcp_keep_apart_workspace"][:2] == (I, [I, I, I, VP])
    assert abi.functions["tcp_keep_apart"][:2] == (I, [VP, VP, VP, I, I, I, I, VP, VP, VP, D, I, I, I, D, VP, LONG] + [VP] * 12)
    assert abi.functions["tcp_keep_apart"][2][:3] == ["const float*", "const float*", "const long*"]
    with open(_abi.HEADER_APART) as f:
        text = f.read()
    flat = " ".join(text.replace("*", " ").split())
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text and "Not built" in text
    assert "choices, not measurements" in flat and "can close another" in flat and "#define TC_APART_LAUNCHES(rounds) (2 * (rounds) + 3)" in text
    for gone in ("vertical moves", "changing a pose to dodge", "resolving inside the sampler", "mesh-level contact",
                 "contact between parts of one dancer", "smoothing beyond the envelope"):
        assert gone in flat, gone
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_", "tcj_", "tck_", "tcg_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_apart.h", prefix=prefix)
    for names in (L.ABI.functions, L.EXT.functions, L.GLTF.functions, L.SKIN.functions, L.SHADE.functions, L.MJPEG.functions,
                  L.FOOTLOCK.functions, L.GROUP.functions, L.EXPORTS):
        assert not any(n.startswith("tcp_") for n in names)
    frozen = {**L.ABI.constants, **L.EXT.constants, **L.GLTF.constants, **L.SKIN.constants, **L.SHADE.constants, **L.MJPEG.constants,
              **L.FOOTLOCK.constants, **L.GROUP.constants}
    assert not any(k.startswith("TC_APART") for k in frozen) and len(L.ABI.functions) == 79 and len(L.GROUP.functions) == 2
    assert (P.MAX_DANCERS, P.MAX_BLEND, P.MAX_ROUNDS) == (32, 65536, 64)
    with open(os.path.join(ROOT, "include", "tcdiff_group.h")) as f:
        assert "resolving a contact" in f.read()              # the eighth header is left as it was


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    syms = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    assert sorted(s for s in syms if s.startswith("tcp_")) == sorted(NAMES)
    assert not [s for s in syms if "keep_apart" in s.lower() and s.split("_")[0] in ("tcdiff", "tcx", "tcs", "tcr", "tcj", "tck", "tcg")]
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    n = C.c_long(-1)
    want = 41 * (2 * 3 * 10) + 16 * (2 * 3 * 10) + 4                        # 3420 rounded up
    assert lib.tcp_keep_apart_workspace(2, 3, 10, C.addressof(n)) == 0 and n.value == want and want % 8 == 0
    assert lib.tcp_keep_apart_workspace(1, 2, 1, C.addressof(n)) == 0 and n.value == 80          # 41 + 32 = 73, rounded up
    assert lib.tcp_keep_apart_workspace(2, 3, 10, None) == -1
    for bad in ((0, 3, 10), (2, 0, 10), (2, 1, 10), (2, 3, 0), (2, 3, -1)):
        assert lib.tcp_keep_apart_workspace(*bad, C.addressof(n)) == -1, bad
    assert lib.tcp_keep_apart_workspace(2, 33, 10, C.addressof(n)) == -4
    assert lib.tcp_keep_apart_workspace(2 ** 14, 32, 2 ** 14, C.addressof(n)) == -4
    parents, radii = (C.c_int * 24)(*SMPL_PARENTS), (C.c_double * 24)(*RADII)
    strides = (C.c_long * 3)(2160, 720, 72)
    ones = (C.c_double * 32)(*([1.0] * 32))

    def call(pos=p, joints=p, strides=strides, b=2, dn=3, T=10, up=2, parents=parents, radii=radii, mobility=ones, margin=0.02, iterations=8,
             rounds=3, blend=5, max_push=0.6, ws=p, ws_bytes=want - 1, pos_out=p, joints_out=p, shift=p, cb=p, ca=p, gb=p, ga=p, pushed=p,
             capped=p, max_shift=p, max_step=p):
        return lib.tcp_keep_apart(pos, joints, strides, b, dn, T, up, parents, radii, mobility, margin, iterations, rounds, blend, max_push, ws,
                                  ws_bytes, pos_out, joints_out, shift, cb, ca, gb, ga, pushed, capped, max_shift, max_step, None)
    assert call() == -1                                                    # good arguments but for one byte of workspace
    assert call(ws=p + 4, ws_bytes=want) == -2 and call(shift=p + 4, ws_bytes=want) == -2
    assert call(shift=None) == -1 and call(shift=None, ws=p + 4, ws_bytes=want) == -2          # shift may be NULL: the workspace again
    big = 1 << 40
    nan, inf = float("nan"), float("inf")
    for kw in (dict(pos=None), dict(joints=None), dict(strides=None), dict(parents=None), dict(radii=None), dict(mobility=None), dict(ws=None),
               dict(pos_out=None), dict(joints_out=None), dict(cb=None), dict(ca=None), dict(gb=None), dict(ga=None), dict(pushed=None),
               dict(capped=None), dict(max_shift=None), dict(max_step=None), dict(b=0), dict(dn=0), dict(dn=1), dict(T=0), dict(T=-3),
               dict(up=-1), dict(up=3), dict(iterations=-1), dict(rounds=-1), dict(blend=-1), dict(margin=-0.01), dict(margin=nan),
               dict(margin=inf), dict(max_push=-1.0), dict(max_push=nan), dict(max_push=inf),
               dict(strides=(C.c_long * 3)(2160, -720, 72))):
        assert call(ws_bytes=big, **kw) == -1, kw
    for kw in (dict(dn=33), dict(blend=65537), dict(rounds=65), dict(b=2 ** 14, dn=32, T=2 ** 14)):
        assert call(ws_bytes=big, **kw) == -4, kw
    assert call(ws_bytes=big, dn=33, strides=(C.c_long * 3)(0, 0, -1)) == -4 and call(ws_bytes=big, dn=33, up=3) == -1          # the order
    for j, parent in ((3, 5), (7, 7), (2, -1)):                             # a parent after its child, itself, none
        wrong = list(SMPL_PARENTS)
        wrong[j] = parent
        assert call(parents=(C.c_int * 24)(*wrong), ws_bytes=big) == -1, (j, parent)
    for value in (-0.01, nan, inf):
        wrong = list(RADII)
        wrong[11] = value
        assert call(radii=(C.c_double * 24)(*wrong), ws_bytes=big) == -1, value
        assert call(mobility=(C.c_double * 3)(1.0, value, 1.0), ws_bytes=big) == -1, value
    wrong = list(RADII)
    wrong[0] = nan                                                         # entry 0 is unused: the call gets as far as the workspace
    assert call(radii=(C.c_double * 24)(*wrong)) == -1 and call(radii=(C.c_double * 24)(*wrong), ws=p + 4, ws_bytes=want) == -2
    assert call(mobility=(C.c_double * 4)(0.0, 0.0, 0.0, nan), ws=p + 4, ws_bytes=want) == -2          # only dn of them are read


def test_the_ninth_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.APART.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_apart.h"', '#include "tcdiff_apart.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ['  printf("%d\\n", TC_APART_LAUNCHES(3));', "  return 0;", "}"]
    cfile, exe = tmp_path / "apart.c", tmp_path / "apart"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.APART.constants[n] for n in names] + [9]
    calls = ['#include "tcdiff_apart.h"', '#include "tcdiff_apart.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.APART.functions.items():
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
def test_keep_apart_refuses_before_any_launch():
    import tcdiff_amd
    assert tcdiff_amd.keep_apart is P.keep_apart and tcdiff_amd.Apart is P.Apart and {"keep_apart", "Apart"} <= set(tcdiff_amd.__all__)
    assert P.Apart._fields == ("pos", "joints", "contact_before", "contact_after", "gap_min_before", "gap_min_after", "pushed", "capped",
                               "max_shift", "max_step", "shift")
    sig = inspect.signature(P.keep_apart).parameters
    assert list(sig) == ["pos", "joints", "dn", "up", "radii", "parents", "margin", "iterations", "rounds", "blend", "max_push", "mobility",
                         "return_shift"]
    assert [sig[k].default for k in list(sig)[2:]] == [inspect.Parameter.empty, 2, None, None, 0.02, 8, 3, 5, 0.6, None, False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[2:])
    J, pos = torch.zeros(2, 3, 6, 24, 3), torch.zeros(2, 18, 3)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        P.keep_apart(pos, J, dn=3)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        P.keep_apart(pos[:, :6], J[:, :1], dn=1)                       # one dancer is refused off the device as well
    late = list(SMPL_PARENTS)
    late[3] = 5
    for bad in (dict(joints=J[0]), dict(joints=J.double()), dict(joints=J.numpy()), dict(joints=torch.zeros(2, 3, 6, 23, 3)), dict(joints=J[:, :, :0]),
                dict(joints=J.transpose(-1, -2).contiguous().transpose(-1, -2)), dict(pos=pos[:, :17]), dict(pos=pos.double()), dict(pos=pos.numpy()),
                dict(dn=2), dict(dn=3.0), dict(dn=True), dict(joints=torch.zeros(1, 33, 1, 24, 3), pos=torch.zeros(1, 33, 3), dn=33), dict(up=3),
                dict(up=-1), dict(up=True), dict(margin=-0.01), dict(margin=float("nan")), dict(margin=None), dict(max_push=-1), dict(max_push=float("inf")),
                dict(max_push="1"), dict(iterations=-1), dict(iterations=2.0), dict(iterations=True), dict(rounds=-1), dict(rounds=65), dict(rounds=1.5),
                dict(blend=-1), dict(blend=65537), dict(blend=5.0), dict(radii=np.ones(23)), dict(radii=-np.ones(24)), dict(radii=np.full(24, np.nan)),
                dict(parents=SMPL_PARENTS[:5]), dict(parents=late), dict(mobility=[1, 1]), dict(mobility=[1, -1, 1]),
                dict(mobility=[1, float("nan"), 1]), dict(mobility=[1, float("inf"), 1]), dict(mobility="abc"), dict(mobility=1.0)):
        kw = dict(pos=pos, joints=J, dn=3)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match="keep_apart"):
            P.keep_apart(kw.pop("pos"), kw.pop("joints"), **kw)
    for doc in (P.__doc__, P.keep_apart.__doc__):
        assert "choices, not measurements" in " ".join(doc.split())
    assert "unpinned" in P.__doc__ and "Not built" in P.__doc__ and "can close another" in " ".join(P.__doc__.split())


# ---- render_sample ----------------------------------------------------------------------------------------------------------------------------
def test_render_sample_keeps_apart_before_the_foot_lock_and_only_when_asked(monkeypatch, tmp_path):
    from tcdiff_amd import GaussianDiffusion, apart, export, footlock
    assert GaussianDiffusion.keep_apart is False and GaussianDiffusion.foot_lock is False
    params = list(inspect.signature(GaussianDiffusion.render_sample).parameters)
    assert params == ["self", "shape", "cond", "normalizer", "epoch", "render_out", "fk_out", "name", "sound", "mode", "noise", "constraint",
                      "sound_folder", "start_point", "render", "required_dancer_num", "x_0", "render_len", "glb_out", "draw_out"]
    q, pos, poses, contacts = (torch.full((1,), float(k)) for k in range(4))          # stand-ins: only their identity matters
    moved_pos, moved_poses, locked_q, locked_joints = (torch.full((1,), float(k)) for k in range(10, 14))
    calls = []

    def fake_export(x, normalizer, mode, dn, **kw):
        calls.append(("export", dn))
        return q, pos, poses, contacts

    def fake_apart(pos_, joints_, **kw):
        calls.append(("keep_apart", pos_, joints_, kw["dn"]))
        return apart.Apart(moved_pos, moved_poses, *[None] * 9)

    def fake_lock(q_, pos_, contacts_, **kw):
        calls.append(("foot_lock", q_, pos_, contacts_, kw["dn"]))
        return footlock.FootLock(locked_q, locked_joints, None, None, None)

    def fake_write(folder, mode, epoch, name, q_, pos_, poses_):
        calls.append(("write", q_, pos_, poses_))

    monkeypatch.setattr(export, "export_poses", fake_export)
    monkeypatch.setattr(export, "write_fk_out", fake_write)
    monkeypatch.setattr(apart, "keep_apart", fake_apart)
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
    assert render(keep_apart=True) == ["export", "keep_apart", "write"]
    assert calls[1][1] is pos and calls[1][2] is poses and calls[1][3] == 3
    assert calls[2][1] is q and calls[2][2] is moved_pos and calls[2][3] is moved_poses
    assert render(keep_apart=True, foot_lock=True) == ["export", "keep_apart", "foot_lock", "write"]
    assert calls[2][1] is q and calls[2][2] is moved_pos and calls[2][3] is contacts          # the lock re-pins from the shifted motion
    assert calls[3][1] is locked_q and calls[3][2] is moved_pos and calls[3][3] is locked_joints
    assert render(foot_lock=True) == ["export", "foot_lock", "write"]
    assert calls[1][2] is pos and calls[2][2] is pos and calls[2][3] is locked_joints


class _FakeSamples:
    """what render_sample asks of the samples before the export: are they on the device"""
    is_cuda = True
    device = torch.device("cpu")
