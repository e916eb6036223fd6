"""csrc/music.hip and tcdiff_amd/music.py on an MI355X against the float64 run of the restatement tests/music_ref.py, on every
output, the ``return_parts`` ones included, no element left out.

Bound.  The kernels compute in fp32, as librosa does, so the yardstick is the restatement's own float32 run: per output and case,
with d32 = max |ref_f32 - ref_f64|,

    max |kernel - ref_f64| <= 32 max(d32, 2^-23 max |ref_f64|).

The factor 32 is a margin for a different FFT factorisation (eleven radix-2 stages against pocketfft's mixed radix) and different
summation orders in the mel, DCT, overlap-add and autocorrelation sums; it is not measured.  The observed error / max(d32, floor)
of every output and case is printed before it is asserted (recorded in profiles/music.txt).

Cases: the smallest clips at which each kernel can still go wrong -- A 2048 samples (5 frames: the smallest legal clip, the time
median reflects several times, the tempogram sees only padding), B 13 frames (length no multiple of the hop), C 42 frames (time
axis longer than the 31-tap median), D 451 frames (longer than the tempogram window; its lag-30 peak), E three clips of C's
length at once, one of them silent, F the same through a wider row stride."""
import numpy as np
import pytest
import torch

import music_ref as R
from tcdiff_amd import metrics as M
from tcdiff_amd import music as MU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 32.0
CASES = {"A": 2048, "B": 12 * 512 + 137, "C": 41 * 512 + 137, "D": 450 * 512 + 137}
SEED = {"A": 1, "B": 2, "C": 3, "D": 4}
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _ref(n, seed):
    """(signal, float64 features, float32 features), computed once and left unchanged"""
    def make():
        y = R.make_signal(n, seed=seed)
        return y, R.features(y, dtype=np.float64), R.features(y, dtype=np.float32)
    return _once(("ref", n, seed), make)


def _run(y):
    feats, parts = MU.music_features(torch.from_numpy(y).to(DEV), return_parts=True)
    torch.cuda.synchronize()
    return feats, parts


def _outputs(feats, parts):
    """name -> numpy array of one clip, under the names of music_ref.features"""
    f = feats.cpu().numpy()
    out = dict(mfcc=f[:, :20], delta=f[:, 20:40], onset_col=f[:, 40], tempogram=f[:, 41:])
    out.update({k: v.cpu().numpy() for k, v in parts.items()})
    return out


_REF_NAME = dict(onset_col="onset_env")


def _check(case, out, r64, r32):
    worst = {}
    failed = []
    for name, got in out.items():
        want, want32 = r64[_REF_NAME.get(name, name)], r32[_REF_NAME.get(name, name)]
        assert got.dtype == np.float32 and got.shape == want.shape, (case, name, got.shape, want.shape)
        assert np.isfinite(got).all(), (case, name)
        d32 = float(np.abs(want32.astype(np.float64) - want).max())
        unit = max(d32, 2.0 ** -23 * float(np.abs(want).max()))
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst[name] = err / unit if unit > 0 else (0.0 if err == 0 else float("inf"))
        print(f"music case {case} {name:11s} err {err:.3e} d32 {d32:.3e} unit {unit:.3e} ratio {worst[name]:.2f}")
        if not err <= FACTOR * unit:
            failed.append((name, err, unit))
    assert not failed, (case, failed)
    return worst


@pytest.mark.parametrize("case", list(CASES))
def test_against_float64(case):
    y, r64, r32 = _ref(CASES[case], SEED[case])
    feats, parts = _once(("run", case), lambda: _run(y))
    T = 1 + len(y) // 512
    assert feats.shape == (1, T, 425) and feats.dtype == torch.float32 and feats.is_cuda
    assert parts["mel_db"].shape == (1, T, 128) and parts["onset_env"].shape == (1, T)
    assert parts["harmonic"].shape == (1, len(y)) and parts["percussive"].shape == (1, len(y))
    _check(case, _outputs(feats[0], {k: v[0] for k, v in parts.items()}), r64, r32)
    assert (feats[0, :3, 40] == 0).all() and torch.equal(feats[0, :, 40], parts["onset_env"][0])


def test_tempogram_peak_of_the_120_bpm_signal():
    """bursts every sr / 2 samples are 30 frames apart: the middle frame's largest value at lags >= 10 is at lag 30, and lag 0 is 1"""
    y, r64, _ = _ref(CASES["D"], SEED["D"])
    feats, _ = _once(("run", "D"), lambda: _run(y))
    tg = feats[0, :, 41:].cpu().numpy()
    assert 10 + int(np.argmax(r64["tempogram"][225, 10:])) == 30
    assert 10 + int(np.argmax(tg[225, 10:])) == 30
    loud = np.abs(tg).max(axis=1) > 0
    assert loud[225] and (tg[loud, 0] == 1.0).all()


def _batch():
    n = CASES["C"]
    ys = [_ref(n, SEED["C"])[0], np.zeros(n, np.float32), _ref(n, 5)[0]]
    return n, ys, torch.from_numpy(np.stack(ys)).to(DEV)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_batch_of_three_with_a_silent_clip():
    n, ys, Y = _batch()
    feats, parts = MU.music_features(Y, return_parts=True)
    assert feats.shape == (3, 42, 425)
    for b, seed in ((0, SEED["C"]), (2, 5)):
        _, r64, r32 = _ref(n, seed)
        _check(f"E{b}", _outputs(feats[b], {k: v[b] for k, v in parts.items()}), r64, r32)
    for b in range(3):                                    # each clip: the bits of its single-clip call
        f1, p1 = MU.music_features(Y[b], return_parts=True)
        _same(f1[0], feats[b])
        for k in parts:
            _same(p1[k][0], parts[k][b])
    assert not torch.isnan(feats).any()
    assert (feats[1] == 0).all() and all((v[1] == 0).all() for v in parts.values())      # silence: exact zeros
    # a second call: the same bits; without the parts: the same features
    f2, p2 = MU.music_features(Y, return_parts=True)
    _same(f2, feats)
    for k in parts:
        _same(p2[k], parts[k])
    _same(MU.music_features(Y), feats)


def test_wider_row_stride():
    n, ys, Y = _batch()
    wide = torch.full((3, n + 37), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :n] = Y
    view = wide[:, :n]
    assert not view.is_contiguous()
    f0, p0 = MU.music_features(Y, return_parts=True)
    f1, p1 = MU.music_features(view, return_parts=True)
    _same(f1, f0)
    for k in p0:
        _same(p1[k], p0[k])


def test_assemble_cond_places_every_column():
    n, ys, Y = _batch()
    feats = MU.music_features(Y)
    B, T = feats.shape[:2]
    g = torch.Generator().manual_seed(0)
    chroma = torch.rand(B, T, 12, generator=g).to(DEV)
    beats = (torch.rand(B, T // 2, generator=g) > 0.7)
    onset_beat = beats.repeat_interleave(2, dim=1).float().to(DEV)
    cond = MU.assemble_cond(feats, chroma, onset_beat)
    assert cond.shape == (B, T, 438) and cond.dtype == torch.float32 and cond.is_cuda
    assert torch.equal(cond[..., :40], feats[..., :40]) and torch.equal(cond[..., 40:52], chroma)
    assert torch.equal(cond[..., 52], feats[..., 40]) and torch.equal(cond[..., 53], onset_beat)
    assert torch.equal(cond[..., 54:], feats[..., 41:])
    assert torch.equal(M.beats_from_cond(cond, T // 2).cpu(), beats.to(torch.uint8))
