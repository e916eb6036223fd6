"""csrc/beat.hip and tcdiff_amd.music.beat_track on an MI355X against the float64 restatement tests/beat_ref.py.

Bound, per case, in float64: max |kernel - ref| <= 1e-12 max |ref| for local_score and cum_score.  Derived, not measured: a
cumulative score carries at most T / period + 2 period + 2 roundings of 2.2e-16 each, at most 2.4e-13 at these shapes.  The
observed ratio is printed before it is asserted (recorded in profiles/beat.txt).

Condition, not measurement: every decision margin of the reference run (each frame's top-two gap, the first-beat threshold, the
flags, the median test, the trim threshold) is >= 1e-10 max |cum|, a hundred times the bound, and the tempo score's top-two gap
is >= 1e-3 (the fp32 autocorrelation moves log1p(1e6 g) by about 1e-6); tests/test_beat_cpu.py checks that before any GPU run
and it is asserted again here.  Under it period, backlink, n_beats and onset_beat equal the reference exactly, no frame left out.

Cases (tests/beat_ref.py CASES): A 5 frames, the smallest legal clip; B 40 < 2 period: every frame's window reaches before frame
0; C the smallest period the prior allows, h = 6; D 451 frames, shorter than the 480-lag window: every tempo frame sees padding,
h = 15; E h = rint(13.5) = 14, F h = rint(12.5) = 12 (half to even), F also longer than the window with several frame chunks in
launch 1; G many blocks of 6."""
import numpy as np
import pytest
import torch

import beat_ref as R
import music_ref
from tcdiff_amd import kernels as K
from tcdiff_amd import music as MU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(o):
    return torch.from_numpy(np.ascontiguousarray(o)).to(DEV)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def _against(tag, ref, tempo, beat, parts, b=0):
    """row b of a kernel run against the reference run of that clip"""
    assert R.margin_failures(ref) == [], tag
    failed = []
    for name in ("local_score", "cum_score"):
        got, want = parts[name][b].cpu().numpy(), ref[name]
        assert got.dtype == np.float64 and got.shape == want.shape and np.isfinite(got).all(), (tag, name)
        err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
        print(f"beat case {tag} {name:11s} err {err:.3e} of {scale:.3e} ratio {err / scale if scale else 0.0:.2e} (bound {R.BOUND:.0e})")
        if not err <= R.BOUND * scale:
            failed.append((name, err, scale))
    assert not failed, (tag, failed)
    assert int(parts["period"][b]) == ref["period"], tag
    assert float(tempo[b]) == ref["tempo"], tag
    assert np.array_equal(parts["backlink"][b].cpu().numpy(), ref["backlink"]), tag
    assert int(parts["n_beats"][b]) == ref["n_beats"], tag
    got = beat[b].cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, ref["onset_beat"]), tag
    assert np.array_equal(np.nonzero(got)[0], ref["beats"]), tag


@pytest.mark.parametrize("name", list(R.CASES))
def test_against_float64(name):
    T, every, bpm, seed = R.CASES[name]
    o, ref = R.case(name)
    tempo, beat, parts = MU.beat_track(_dev(o), bpm=bpm, return_parts=True)
    assert tempo.shape == (1,) and tempo.dtype == torch.float64 and beat.shape == (1, T) and beat.dtype == torch.float32 and beat.is_cuda
    assert parts["period"].dtype == torch.int32 and parts["backlink"].dtype == torch.int32 and parts["n_beats"].shape == (1,)
    assert parts["local_score"].shape == (1, T) and parts["cum_score"].shape == (1, T) and parts["backlink"].shape == (1, T)
    _against(name, ref, tempo, beat, parts)
    if every and name != "B":
        assert ref["n_beats"] >= 3 and ((ref["beats"] - 7) % every == 0).all()      # the beats are on the clicks


def _batch():
    rows, refs = R.batch_rows()
    return refs, _dev(np.stack(rows))


def _same_run(a, b):
    _same(a[0], b[0])
    _same(a[1], b[1])
    for k in a[2]:
        _same(a[2][k], b[2][k])


def test_batch_of_three_with_a_silent_clip_and_two_periods():
    refs, O = _batch()
    run = MU.beat_track(O, return_parts=True)
    tempo, beat, parts = run
    assert tempo.shape == (3,) and beat.shape == (3, 600)
    assert parts["period"].tolist() == [30, 0, 27] and tempo.tolist() == [120.0, 0.0, 3600.0 / 27]
    for b in (0, 2):
        _against(f"batch{b}", refs[b], tempo, beat, parts, b)
    assert not beat[1].any() and int(parts["n_beats"][1]) == 0 and not parts["cum_score"][1].any() and not parts["local_score"][1].any()
    assert (parts["backlink"][1] == -1).all()
    for b in range(3):                                    # each row: the bits of the same clip run alone
        t1, b1, p1 = MU.beat_track(O[b], return_parts=True)
        _same(t1[0], tempo[b])
        _same(b1[0], beat[b])
        for k in parts:
            _same(p1[k][0], parts[k][b])
    _same_run(MU.beat_track(O, return_parts=True), run)   # a second run: the same bits
    t2, b2 = MU.beat_track(O)
    _same(t2, tempo)
    _same(b2, beat)


def test_wider_row_stride():
    refs, O = _batch()
    wide = torch.full((3, 600 + 37), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :600] = O
    view = wide[:, :600]
    assert not view.is_contiguous()
    _same_run(MU.beat_track(view, return_parts=True), MU.beat_track(O, return_parts=True))
    _same_run(MU.beat_track(view, bpm=[120.0, 100.0, 3600.0 / 27], return_parts=True),
              MU.beat_track(O, bpm=[120.0, 100.0, 3600.0 / 27], return_parts=True))


@pytest.mark.parametrize("name", ["C", "D"])
def test_untrimmed_beats(name):
    T, every, bpm, seed = R.CASES[name]
    o, ref = R.case(name, trim=False)
    tempo, beat, parts = MU.beat_track(_dev(o), bpm=bpm, trim=False, return_parts=True)
    _against(name + " untrimmed", ref, tempo, beat, parts)
    trimmed = R.case(name)[1]
    assert ref["n_beats"] > trimmed["n_beats"] and int(parts["n_beats"][0]) > trimmed["n_beats"]
    assert set(trimmed["beats"]) < set(np.nonzero(beat[0].cpu().numpy())[0])


def test_a_given_bpm_makes_one_launch_fewer(monkeypatch):
    """each of the two wrappers is one launcher call and each launcher one kernel launch (include/tcdiff_hip.h)"""
    calls = []
    for name in ("beat_tempo", "beat_track"):
        def wrap(*a, _inner=getattr(K, name), _name=name, **kw):
            calls.append(_name)
            return _inner(*a, **kw)
        monkeypatch.setattr(K, name, wrap)
    refs, O = _batch()
    est = MU.beat_track(O, return_parts=True)
    assert calls == ["beat_tempo", "beat_track"]
    del calls[:]
    given = MU.beat_track(O, bpm=[120.0, 77.0, 3600.0 / 27], return_parts=True)
    assert calls == ["beat_track"]
    assert given[2]["period"].tolist() == [30, 47, 27] and given[0].tolist() == [120.0, 0.0, 3600.0 / 27]      # (the silent row: tempo 0)
    for b in (0, 2):                                      # the estimated periods given: the same beats, scores and links, bit for bit
        _same(given[1][b], est[1][b])
        for k in ("local_score", "cum_score", "backlink", "n_beats"):
            _same(given[2][k][b], est[2][k][b])
    assert not given[1][1].any()


def test_music_cond_chains_the_three_calls():
    y = torch.from_numpy(music_ref.make_signal(40 * 512 + 137, seed=3)).to(DEV)
    chroma = torch.rand(1, 41, 12, generator=torch.Generator().manual_seed(0)).to(DEV)
    cond = MU.music_cond(y, chroma)
    assert cond.shape == (1, 41, 438) and cond.dtype == torch.float32 and cond.is_cuda
    feats, parts = MU.music_features(y, return_parts=True)
    tempo, onset_beat = MU.beat_track(parts["onset_env"])
    _same(cond, MU.assemble_cond(feats, chroma, onset_beat))
    _same(cond[..., MU.ONSET_BEAT], onset_beat)
    assert torch.equal(cond[..., 40:52], chroma) and set(onset_beat.unique().tolist()) <= {0.0, 1.0}
