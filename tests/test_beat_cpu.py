"""CPU checks of the beat track (no GPU): the numpy restatement tests/beat_ref.py -- the yardstick of tests/test_beat_gpu.py --
against things that can be checked by hand, the property the kernel's block-parallel programme rests on, the margin condition of
every GPU case, and the host side of tcdiff_amd.music.beat_track (tables, validation, no CPU fallback)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import beat_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import music as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_tab = {}


def _package_tables(period, tightness=100.0):
    """The restatement is only a yardstick for the kernel if the tables the package uploads are the ones it uses: row ``period``
    of music.beat_tables holds the restatement's window and transition score bit for bit, the latter h = rint(period / 2) short
    of two periods."""
    if tightness not in _tab:
        _tab[tightness] = MU.beat_tables(tightness)
    tab, at = _tab[tightness], period * period - 1
    d, txwt = R.transition(period, tightness)
    assert len(txwt) == 2 * period - R.half_period(period) + 1 and np.array_equal(tab[1, at:at + len(txwt)], txwt)
    assert np.array_equal(tab[0, at:at + 2 * period + 1], np.exp(-0.5 * (np.arange(-period, period + 1) * 32.0 / period) ** 2))
    return tab[0, at:at + 2 * period + 1], tab[1, at:at + len(txwt)]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [30, 25, 27, 12])
def test_beats_fall_on_the_clicks_when_the_tempo_is_given(every):
    T = 600
    o = R.make_envelope(T, every, seed=0)
    assert o.dtype == np.float32 and (o[:3] == 0).all() and o[7] >= 1.0 and o[7 + every] >= 1.0 and o[8] <= 0.05
    r = R.beat_track(o, bpm=3600.0 / every)
    assert r["period"] == every and r["tempo"] == 3600.0 / every
    _package_tables(every)
    assert r["n_beats"] >= T // every - 4 and r["beats"][0] == 7
    assert ((r["beats"] - 7) % every == 0).all() and (np.diff(r["beats"]) == every).all()
    assert r["onset_beat"].dtype == np.float32 and r["onset_beat"].sum() == r["n_beats"] and (r["onset_beat"][r["beats"]] == 1).all()
    untrimmed = R.beat_track(o, bpm=3600.0 / every, trim=False)
    assert set(r["beats"]) <= set(untrimmed["beats"])      # (strictly more: test_trim_changes_the_kept_beats_of_the_cases_that_test_it)


def test_tempo_estimate_and_the_prior():
    prior = R.tempo_prior()
    assert np.isneginf(prior[:12]).all() and np.isfinite(prior[12:]).all()          # 3600 / 11 = 327 >= 320 > 3600 / 12
    assert int(np.argmax(prior)) == 30 and prior[30] == 0.0                         # 120 beats per minute
    assert np.abs(MU.tempo_prior(120.0, 1.0, 320.0)[12:] - prior[12:]).max() == 0 and np.isneginf(MU.tempo_prior(120.0, 1.0, 320.0)[:12]).all()
    for every in (30, 25, 27):
        bpm, lag, gap = R.tempo(R.make_envelope(600, every, seed=0))
        assert lag == every and bpm == 3600.0 / every and gap > 0.1
    bpm, lag, gap = R.tempo(R.make_envelope(600, 12, seed=0))                       # 300 per minute: the prior prefers half of it
    assert lag == 24 and bpm == 150.0
    g = R.mean_autocorrelation(R.make_envelope(64, 12, seed=0))
    assert g.shape == (480,) and g[0] == pytest.approx(1.0, abs=1e-12) and np.abs(g).max() <= 1.0 + 1e-12


def test_quirks_kept_from_librosa():
    assert [R.half_period(p) for p in (24, 25, 27, 30, 1)] == [12, 12, 14, 15, 0]   # 12.5 -> 12, 13.5 -> 14: half to even
    d, txwt = R.transition(25, 100.0)
    assert [len(_package_tables(p)[1]) for p in (24, 25, 27, 30)] == [2 * p - h + 1 for p, h in ((24, 12), (25, 12), (27, 14), (30, 15))]
    assert d[0] == -50 and d[-1] == -12 and len(txwt) == 2 * 25 - 12 + 1 and txwt[25] == 0.0 and (txwt <= 0).all()
    ls = np.array([0.0, 5.0, 1.0, 5.0, 5.0, 0.2, 5.0])
    beats = np.arange(7)
    kept, _ = R.trim_beats(ls, beats, trim=True)            # s = (2.5, 5.5, 6, 8, 7.6, 5.2, 5.1), half their rms is 2.97: s[0] is below
    assert list(kept) == [1, 2, 3, 4, 5]                    # ... and the end of the slice is exclusive: beat 6 goes too
    assert list(R.trim_beats(ls, beats, trim=False)[0]) == [0, 1, 2, 3, 4, 5]
    one, _ = R.trim_beats(np.array([3.0]), np.array([0]), trim=False)
    assert len(one) == 0
    # the symmetric 5-point Hann is (0, 0.5, 1, 0.5, 0): three taps
    v = np.array([1.0, 2.0, 4.0])
    _, margin = R.trim_beats(v, np.arange(3), trim=False)
    assert margin == 2.0                                   # s = (2, 4, 5): the smallest |s - 0|


def test_local_score_by_direct_evaluation():
    o = R.make_envelope(40, 30, seed=3)
    for period in (3, 12, 30):
        ls = R.local_score(o, period)
        w, _ = _package_tables(period)
        assert w[period] == 1.0 and np.array_equal(w, w[::-1])
        x = o.astype(np.float64) / o.astype(np.float64).std(ddof=1)
        for i in (0, 7, 39):
            want = sum(np.exp(-0.5 * (32.0 * j / period) ** 2) * x[i - j] for j in range(-period, period + 1) if 0 <= i - j < 40)
            assert ls[i] == pytest.approx(want, rel=1e-13)


@pytest.mark.parametrize("name", ["B", "C", "D", "E", "F", "G"])
def test_programme_in_blocks_of_half_a_period_reads_no_frame_of_its_block(name):
    """the kernel runs h = rint(period / 2) frames between two barriers: they must not read one another's cumulative score"""
    o, ref = R.case(name)
    h = R.half_period(ref["period"])
    assert len(_package_tables(ref["period"])[1]) == 2 * ref["period"] - h + 1     # the kernel's candidates end h frames back
    cum, back, _, _ = R.programme(ref["local_score"], ref["period"], 100.0, block=h)
    assert np.array_equal(cum, ref["cum_score"]) and np.array_equal(back, ref["backlink"])
    cum, _, _, _ = R.programme(ref["local_score"], ref["period"], 100.0, block=2 * ref["period"])
    assert not np.array_equal(cum, ref["cum_score"])        # (blocks as long as the window do differ: the check can fail)


@pytest.mark.parametrize("name", list(R.CASES))
def test_margin_condition_of_the_gpu_cases(name):
    """every decision of the reference is farther from its alternative than the kernel's rounding error can reach"""
    for trim in (True, False):
        o, ref = R.case(name, trim)
        assert len(o) == R.CASES[name][0]
        _package_tables(ref["period"])
        print(name, trim, ref["period"], ref["n_beats"], float(np.abs(ref["cum_score"]).max()), ref["margins"])
        assert R.margin_failures(ref) == []
    if name in "DEF":
        assert ref["period"] == R.CASES[name][1]            # the estimated lag is the clicks' distance


def test_margin_condition_of_the_gpu_batch():
    rows, refs = R.batch_rows()
    assert [len(o) for o in rows] == [600] * 3 and [r["period"] for r in refs] == [30, 0, 27]
    assert refs[1]["tempo"] == 0.0 and refs[1]["n_beats"] == 0 and not refs[1]["onset_beat"].any()
    for r in (refs[0], refs[2]):
        _package_tables(r["period"])
        assert R.margin_failures(r) == [] and r["n_beats"] > 5


def test_trim_changes_the_kept_beats_of_the_cases_that_test_it():
    for name in ("C", "D"):
        a, b = R.case(name, True)[1], R.case(name, False)[1]
        _package_tables(a["period"])
        assert b["n_beats"] > a["n_beats"] and np.array_equal(a["cum_score"], b["cum_score"])


# ---- the host side -----------------------------------------------------------------------------------------------------------------
def test_tables():
    tab = MU.beat_tables(100.0)
    assert tab.shape == (2, 480 * 480 - 1) and tab.dtype == np.float64 and L.BEAT_TABLE == 480 * 480 - 1
    for p in (1, 2, 12, 25, 27, 479):
        at = p * p - 1
        w = np.exp(-0.5 * (np.arange(-p, p + 1) * 32.0 / p) ** 2)
        d, txwt = R.transition(p, 100.0)
        assert np.array_equal(tab[0, at:at + 2 * p + 1], w) and tab[0, at + p] == 1.0
        assert np.array_equal(tab[1, at:at + len(txwt)], txwt) and len(txwt) <= 2 * p + 1
    assert np.isneginf(tab[1, 2]) and np.isfinite(tab[1, 3:]).all()                 # period 1: d = 0
    assert np.array_equal(MU.beat_tables(50.0)[1, 3:] * 2, tab[1, 3:])
    dev = MU._beat_tables(100.0, "cpu")
    assert MU._beat_tables(100.0, "cpu") is dev and dev["tables"].shape == (2, 480 * 480 - 1) and dev["window"].shape == (480,)
    assert np.abs(dev["window"].numpy() - R.hann(480)).max() <= 2.0 ** -24


def test_argument_errors_and_no_cpu_fallback():
    ok = torch.zeros(2, 64)
    for bad in (ok.double(), ok[:, :4], torch.zeros(1, 2, 64), torch.zeros(()), ok[:, ::2], np.zeros(64, np.float32), ok[:0]):
        with pytest.raises(L.TcdiffError):
            MU.beat_track(bad)
    for kw in (dict(tightness=0), dict(tightness=-1.0), dict(tightness=float("nan")), dict(tightness="x"), dict(start_bpm=0),
               dict(std_bpm=-1), dict(max_tempo=7.0), dict(bpm=0), dict(bpm=-120.0), dict(bpm=float("inf")), dict(bpm=7.0),
               dict(bpm=8000.0), dict(bpm=[120.0]), dict(bpm=[120.0, 90.0, 60.0]), dict(bpm=[120.0, "x"])):
        with pytest.raises(L.TcdiffError):
            MU.beat_track(ok, **kw)
    for kw in ({}, dict(bpm=120.0), dict(bpm=[120.0, 90.0], return_parts=True)):
        with pytest.raises(L.TcdiffError, match="no CPU fallback"):
            MU.beat_track(ok, **kw)
    with pytest.raises(L.TcdiffError, match="no CPU fallback"):
        MU.beat_track(ok[0])
    with pytest.raises(L.TcdiffError, match="no CPU fallback"):
        MU.music_cond(torch.zeros(4096), torch.zeros(1, 9, 12))


def test_launchers_validate_before_any_launch():
    from tcdiff_amd import build
    build.build(verbose=False)
    lib = L.load()
    for sym in ("tcdiff_beat_tempo", "tcdiff_beat_track"):
        assert sym in L.EXPORTS and hasattr(lib, sym)
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    per = (C.c_int * 2)(30, 27)
    assert lib.tcdiff_beat_tempo(None, 64, 1, 64, p, p, None) == -1 and lib.tcdiff_beat_tempo(p, 64, 1, 64, p, None, None) == -1
    assert lib.tcdiff_beat_tempo(p, 64, 0, 64, p, p, None) == -1 and lib.tcdiff_beat_tempo(p, 64, 1, 4, p, p, None) == -1
    assert lib.tcdiff_beat_tempo(p, 64, 65536, 64, p, p, None) == -4 and lib.tcdiff_beat_tempo(p, 64, 1, (1 << 20) + 1, p, p, None) == -4
    track = lambda *a: lib.tcdiff_beat_track(*a)
    out = (p,) * 8
    assert track(None, 64, 2, 64, None, None, p, per, 1, *out, None) == -1
    assert track(p, 64, 2, 64, None, None, None, per, 1, *out, None) == -1
    assert track(p, 64, 2, 64, None, None, p, None, 1, *out, None) == -1            # neither partial sums nor periods
    assert track(p, 64, 2, 64, p, p, p, per, 1, *out, None) == -1                   # both
    assert track(p, 64, 2, 64, p, None, p, None, 1, *out, None) == -1               # partial sums without the prior
    assert track(p, 64, 2, 4, None, None, p, per, 1, *out, None) == -1 and track(p, 64, 0, 64, None, None, p, per, 1, *out, None) == -1
    for bad in ((0, 27), (30, 480), (-3, 27)):
        assert track(p, 64, 2, 64, None, None, p, (C.c_int * 2)(*bad), 1, *out, None) == -1
    assert track(p, 64, 65536, 64, p, p, p, None, 1, *out, None) == -4 and track(p, 64, 2, (1 << 20) + 1, p, p, p, None, 1, *out, None) == -4
    for i in range(8):
        assert track(p, 64, 2, 64, p, p, p, None, 1, *(out[:i] + (None,) + out[i + 1:]), None) == -1
    hdr = open(os.path.join(ROOT, "include", "tcdiff_hip.h")).read()
    for name, val in (("WIN", L.BEAT_WIN), ("CHUNK", L.BEAT_CHUNK)):
        assert f"#define TC_BEAT_{name} {val}" in hdr
    assert "music features: the beat track" in hdr
