"""CPU checks of the motion metrics (no GPU): the numpy float64 restatement tests/metrics_ref.py against scipy's smoothing
and minima and against hand-checkable motions, the seeded GPU inputs against the near-tie conditions, beats_from_cond
against a plain loop, and the host side of tcdiff_amd.metrics (validation, no CPU fallback, summarize)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter1d
from scipy.signal import argrelextrema

import metrics_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import metrics as M


@pytest.mark.parametrize("n", [2, 5, 19, 20, 21, 44, 150, 1124])
@pytest.mark.parametrize("sigma", [5.0, 1.3])
def test_smoothing_and_minima_are_scipys(n, sigma):
    """N = 2, 5, 19 are shorter than the filter radius (20 at sigma 5): the reflection wraps more than once"""
    g = np.random.default_rng(n)
    v = g.uniform(0.0, 0.05, n) + 0.01 * np.sin(np.arange(n) * 0.7)
    s = R.smooth(v, sigma)
    want = gaussian_filter1d(v, sigma)
    assert s.shape == want.shape and float(np.abs(s - want).max()) <= 1e-13
    assert np.array_equal(R.minima(want), argrelextrema(want, np.less)[0])
    assert np.array_equal(R.minima(v), argrelextrema(v, np.less)[0])
    if n > 20:
        assert len(R.minima(v)) > 0


def test_filter_radius_and_weights_are_scipys():
    for sigma in (5.0, 3.0, 0.8, 2.37):
        w, r = R.gaussian_weights(sigma)
        assert r == int(4.0 * sigma + 0.5) and len(w) == 2 * r + 1
        impulse = np.zeros(2 * r + 1)
        impulse[r] = 1.0
        assert float(np.abs(w - gaussian_filter1d(impulse, sigma, mode="constant")).max()) <= 1e-16
        assert gaussian_filter1d(np.r_[impulse, 0.0, 0.0], sigma, mode="constant")[-1] == 0.0      # nothing beyond the radius


def _body(T, dn=1):
    """a rigid T-pose-like body standing still: (1, dn, T, 24, 3)"""
    g = np.random.default_rng(5)
    pose = g.uniform(-0.5, 0.5, (24, 3))
    J = np.broadcast_to(pose, (1, dn, T, 24, 3)).copy()
    J[..., 2] += 0.9
    return J


def test_a_static_dancer():
    J = _body(40).astype(np.float32)
    beats = np.zeros((1, 40), np.uint8)
    beats[0, ::10] = 1
    m = R.metrics(J, np.ones((1, 1, 40, 4), np.float32), beats)
    assert m["pfc"][0, 0] == 0.0
    assert m["motion_beats"][0, 0] == 0 and math.isnan(m["beat_align"][0, 0])
    assert m["contact_slide"][0, 0] == 0.0 and m["contact_break"][0, 0] == 0.0 and m["contact_frames"][0, 0] == 39 * 4
    assert m["collision_rate"][0] == 0.0                                   # a single dancer
    assert math.isnan(R.metrics(J[:, :, :2])["pfc"][0, 0])                 # T < 3


def test_a_sliding_foot_in_contact():
    J = _body(11)
    J[0, 0, :, 8, 0] += 0.02 * np.arange(11)                               # the right ankle slides 0.02 m per frame
    contacts = np.zeros((1, 1, 11, 4), np.float32)
    contacts[..., 1] = 1.0                                                 # channel 1 = joint 8
    m = R.metrics(J.astype(np.float32), contacts)
    assert m["contact_slide"][0, 0] == pytest.approx(0.02, abs=1e-7)
    assert m["contact_break"][0, 0] == 1.0 and m["contact_frames"][0, 0] == 10
    contacts[..., 1] = 0.95                                                # not above the threshold
    m = R.metrics(J.astype(np.float32), contacts)
    assert m["contact_frames"][0, 0] == 0 and m["contact_slide"][0, 0] == 0.0 and m["contact_break"][0, 0] == 0.0


def test_two_dancers_close_for_half_the_frames():
    J = _body(20, dn=2)
    J[0, 1, :10, :, 0] += 0.2
    J[0, 1, 10:, :, 0] += 1.0
    J[0, 1, :, :, 2] += 5.0                                                # height does not count
    assert R.metrics(J.astype(np.float32))["collision_rate"][0] == 0.5
    assert R.metrics(J.astype(np.float32), up=0)["collision_rate"][0] == 0.0
    J3 = np.concatenate([J, J[:, :1] + np.array([0.0, 50.0, 0.0])], 1)     # a third dancer far away: 3 pairs
    assert R.metrics(J3.astype(np.float32))["collision_rate"][0] == pytest.approx(0.5 / 3, abs=1e-15)


def test_beat_alignment_of_a_sinusoidal_speed_profile():
    T, period = 151, 30
    t = np.arange(T - 1)
    v = 0.02 + 0.01 * np.cos(2 * np.pi * t / period)                       # minima at 15, 45, 75, 105, 135
    J = _body(T)
    J[0, 0, 1:, :, 0] += np.cumsum(v)[:, None]
    J = J.astype(np.float32)
    on = np.zeros((1, T), np.uint8)
    on[0, [45, 75, 105]] = 1
    m = R.metrics(J, beats=on)
    assert m["motion_beats"][0, 0] == 5 and m["beat_align"][0, 0] == 1.0
    _, _, _, mins = R.beat_one(J[0, 0], on[0], 5.0, 3.0)
    assert list(mins) == [15, 45, 75, 105, 135]
    m = R.metrics(J, beats=np.roll(on, 3, axis=1))
    assert m["beat_align"][0, 0] == pytest.approx(math.exp(-0.5), abs=1e-15)
    assert math.isnan(R.metrics(J, beats=np.zeros((1, T), np.uint8))["beat_align"][0, 0])      # no music beats


def test_pfc_by_hand():
    """three frames: one acceleration sample, so a / A = 1 and pfc = min(left) * min(right) of the second step"""
    J = _body(3)
    J[0, 0, 1, :, 0] += 0.01
    J[0, 0, 2, :, 0] += 0.04                                               # every joint: steps of 0.01 then 0.03 along x
    J[0, 0, 2, 10, 1] += 0.04                                              # the left toe moves further than the left ankle
    J = J.astype(np.float32)
    J64 = J.astype(np.float64)
    step = {j: abs(J64[0, 0, 2, j, 0] - J64[0, 0, 1, j, 0]) for j in (7, 8, 11)}       # 0.03 up to the float32 rounding
    assert R.metrics(J)["pfc"][0, 0] == pytest.approx(step[7] * min(step[8], step[11]), rel=1e-12)
    assert R.metrics(J)["pfc"][0, 0] == pytest.approx(9e-4, rel=1e-5)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_seeded_inputs_keep_clear_of_every_decision(shape):
    joints, contacts, beats = R.synth(*shape)
    assert joints.shape == shape + (24, 3) and joints.dtype == np.float32 and beats.dtype == np.uint8
    assert 0.0 <= contacts.min() and contacts.max() <= 1.0
    assert R.decisions_clear(joints, contacts, beats)
    bad = contacts.copy()
    bad[0, 0, 0, 0] = np.float32(0.95)
    assert not R.decisions_clear(joints, bad, beats)
    if shape[2] >= 45:
        m = R.metrics(joints, contacts, beats)
        assert int(m["motion_beats"].min()) >= 1 and 0 < float(m["contact_break"].min()) and float(m["contact_break"].max()) < 1
        assert 0 < float(m["collision_rate"].max()) < 1 and not np.isnan(m["beat_align"]).any()
    if shape[2] >= 150:
        assert 1 / 30 < float(beats.mean()) < 1 / 8                          # about one beat per 15 frames


def test_the_short_case_wraps_the_reflection_more_than_once():
    joints, contacts, beats = R.short_wrap_case()
    n = joints.shape[2] - 1
    assert R.gaussian_weights(5.0)[1] > 2 * n and R.decisions_clear(joints, contacts, beats)
    idx = R.reflect_index(np.arange(-20, n + 20), n)
    assert idx.min() == 0 and idx.max() == n - 1 and list(idx[20 - 2 * n:20]) == list(range(n)) + list(range(n - 1, -1, -1))
    m = R.metrics(joints, contacts, beats)
    assert m["motion_beats"].tolist() == [[1, 0]] and math.isnan(m["beat_align"][0, 1])
    assert m["beat_align"][0, 0] == pytest.approx((1 + math.exp(-4 / 18)) / 2, abs=1e-15)
    s = gaussian_filter1d(R.speed(joints[0, 0]), 5.0)
    assert list(argrelextrema(s, np.less)[0]) == [3]


def test_beats_from_cond_is_the_plain_loop():
    g = torch.Generator().manual_seed(1)
    cond = torch.rand(4, 301, 438, generator=g)
    cond[..., 53] = (torch.rand(4, 301, generator=g) < 0.1).float()
    got = M.beats_from_cond(cond, 150)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, 150)
    assert np.array_equal(got.numpy(), R.beats_from_cond_loop(cond.numpy(), 150))
    assert 0 < int(got.sum()) < got.numel()
    assert np.array_equal(M.beats_from_cond(cond, 60).numpy(), R.beats_from_cond_loop(cond.numpy(), 60))
    # long mode: b = 3 half-overlapping windows of 20 motion frames -> one song of 40
    cond3 = (torch.rand(3, 40, 438, generator=g) < 0.3).float()
    got = M.beats_from_cond(cond3, 40, long=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 40)
    want = R.beats_from_cond_loop(cond3.numpy(), 40, long=True)
    assert np.array_equal(got.numpy(), want) and 0 < int(want.sum()) < 40
    assert want[0, 25] == (cond3[2, 10, 53] > 0.5 or cond3[2, 11, 53] > 0.5)          # frame 25 = window 2, local frame 5
    assert want[0, 39] == (cond3[2, 38, 53] > 0.5 or cond3[2, 39, 53] > 0.5)          # the last window runs to its end
    with pytest.raises(L.TcdiffError):
        M.beats_from_cond(cond, 151)                                                   # 302 music frames needed
    with pytest.raises(L.TcdiffError):
        M.beats_from_cond(cond3, 41, long=True)
    with pytest.raises(L.TcdiffError):
        M.beats_from_cond(cond3[..., :50], 10)


def test_motion_metrics_has_no_cpu_fallback_and_checks_its_inputs():
    with pytest.raises(L.TcdiffError, match="MI355X"):
        M.motion_metrics(torch.zeros(1, 2, 5, 24, 3))
    with pytest.raises(L.TcdiffError, match="joints must be"):
        M.motion_metrics(torch.zeros(1, 2, 5, 72))
    with pytest.raises(L.TcdiffError, match="joints must be"):
        M.motion_metrics(torch.zeros(1, 2, 5, 22, 3))
    with pytest.raises(L.TcdiffError, match="float32"):
        M.motion_metrics(torch.zeros(1, 2, 5, 24, 3, dtype=torch.float64))
    with pytest.raises(L.TcdiffError, match="contiguous"):
        M.motion_metrics(torch.zeros(1, 2, 5, 3, 24).transpose(-1, -2))
    with pytest.raises(L.TcdiffError):
        M.evaluate_samples(torch.zeros(1, 6, 151), None, torch.zeros(1, 6, 438), 2)


def test_launcher_validates_its_arguments_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    lib = L.load()
    assert "tcdiff_motion_metrics" in L.EXPORTS
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    s3 = (C.c_long * 3)(0, 0, 0)

    def rc(joints=p, js=s3, contacts=None, cs=None, beats=None, b=1, dn=1, T=1, up=2, fps=30.0, sig=5.0, sb=3.0, ws=p, pfc=p,
           slide=None, balign=None):
        return lib.tcdiff_motion_metrics(joints, js, contacts, cs, beats, b, dn, T, up, fps, 0.95, 0.01, 0.3, sig, sb, ws, p, pfc,
                                         slide, slide, slide, p, balign, balign, None)
    assert rc(joints=None) == -1 and rc(js=None) == -1 and rc(ws=None) == -1 and rc(pfc=None) == -1
    assert rc(b=0) == -1 and rc(dn=0) == -1 and rc(T=0) == -1 and rc(up=3) == -1 and rc(up=-1) == -1
    assert rc(fps=0.0) == -1 and rc(sig=0.0) == -1 and rc(sb=-1.0) == -1 and rc(sig=float("nan")) == -1
    assert rc(contacts=p, cs=s3) == -1 and rc(contacts=p, slide=p) == -1               # contacts need their strides and outputs
    assert rc(beats=p) == -1                                                            # beats need their outputs
    assert rc(sig=128.0) == -4                                                          # radius 512 is the last one supported
    assert L.METRICS_MAX_RADIUS == 512 and int(4.0 * 127.875 + 0.5) == 512


def test_summarize_takes_nan_means_and_scales_pfc():
    nan = float("nan")
    res = {"pfc": torch.tensor([[1e-4, 3e-4]], dtype=torch.float64), "collision_rate": torch.tensor([0.25, 0.75], dtype=torch.float64),
           "beat_align": torch.tensor([[nan, 0.5], [0.25, nan]], dtype=torch.float64),
           "motion_beats": torch.tensor([[0, 4]]), "contact_slide": torch.tensor([[nan]], dtype=torch.float64)}
    s = M.summarize(res)
    assert set(s) == set(res) and all(type(v) is float for v in s.values())
    assert s["pfc"] == pytest.approx(2.0) and s["collision_rate"] == 0.5 and s["beat_align"] == 0.375 and s["motion_beats"] == 2.0
    assert math.isnan(s["contact_slide"])


def test_the_package_exports_the_metrics():
    import tcdiff_amd
    for name in ("motion_metrics", "beats_from_cond", "evaluate_samples", "summarize"):
        assert getattr(tcdiff_amd, name) is getattr(M, name) and name in tcdiff_amd.__all__
