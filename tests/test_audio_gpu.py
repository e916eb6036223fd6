"""csrc/audio.hip and tcdiff_amd.audio on an MI355X against the numpy restatement tests/audio_ref.py.

Decode and downmix: bit for bit.  Every sample format x 1, 2, 3 channels at 1, 255, 257 and 1000 frames (one frame; one short of
a block; one into the second block; several blocks with 3-, 6-, 9-byte frames that straddle dwords), the inputs holding the
extremes of each integer type, the s32 values that must round with their ties, f64 values that round, and -0.0.

Resample: the rule of tests/test_music_gpu.py, margin included.  The kernel computes weights, products and sums in fp32, as
resampy does on float32 input, so the yardstick is the restatement's own float32 run; per clip, with
d32 = max |ref_f32 - ref_f64|,

    max |kernel - ref_f64| <= 32 max(d32, 2^-23 max |ref_f64|)

over every output sample, and the trailing fix_length samples exactly 0.  The observed error / max(d32, floor) of every clip is
printed before it is asserted (recorded in profiles/audio.txt).

Cases (inputs: seeded noise plus two sines, |x| <= 1):
  R1  44100 -> 30720, n 50        every wing cut by both ends of the signal; one trailing zero
  R2  44100 -> 30720, n 735       511 + 1 outputs, two blocks
  R3  48000 -> 30720, n 1203      three blocks, the full 199-tap interior
  R4  22050 -> 30720, n 700       up-sampling, step 512
  R5   8000 -> 30720, n 300       the input span smaller than a block's outputs
  R6 192000 -> 30720, n 4000      808 taps
  R7 245760 -> 30720, n 4096      the ratio limit, step 64
  R8  44100 -> 30720, 3 x 1500    through a row stride of 1537 with NaN between the rows, the middle clip silent
  R9  44100 -> 30720              a 6000-sample signal sliced with window 2205, step 441: overlapping rows"""
import numpy as np
import pytest
import torch

import audio_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import audio as A
from tcdiff_amd import music as MU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 32.0
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- decode ----------------------------------------------------------------------------------------------------------------------
def _wav(fmt, channels, frames, seed, sr=44100):
    return A.WavData(sr, channels, frames, fmt, R.decode_case(fmt, channels, frames, seed))


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32", "f32", "f64"])
def test_decode_bits(fmt, channels):
    for seed, frames in enumerate((1, 255, 257, 1000)):
        wav = _wav(fmt, channels, frames, seed)
        want = R.to_mono(R.decode(wav.data, fmt, channels))
        assert not np.isnan(want).any()
        got = A.decode(wav, DEV)
        assert got.shape == (1, frames) and got.dtype == torch.float32 and got.device == torch.device(DEV)
        got = got[0].cpu().numpy()
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert len(bad) == 0, (fmt, channels, frames, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("fmt,channels,frames", [("s24", 3, 257), ("s16", 2, 1000), ("f64", 1, 255), ("u8", 3, 1001)])
def test_decode_batch_has_each_files_bits(fmt, channels, frames):
    wavs = [_wav(fmt, channels, frames, seed) for seed in (3, 4, 5)]
    got = A.decode(wavs, DEV)
    assert got.shape == (3, frames)
    for b, wav in enumerate(wavs):
        assert _same_bits(got[b], A.decode(wav, DEV)[0])
        want = R.to_mono(R.decode(wav.data, fmt, channels))
        assert np.array_equal(got[b].cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(L.TcdiffError, match="file 1 .* differs"):
        A.decode([wavs[0], _wav(fmt, channels, frames + 1, 0)], DEV)


# ---- resample --------------------------------------------------------------------------------------------------------------------
def _ref(x, sr):
    """(float64 run, float32 run) of the restatement on the float32 signal x, computed once and left unchanged"""
    key = ("ref", sr, x.tobytes())
    return _once(key, lambda: (R.resample(x, sr), R.resample(x, sr, dtype=np.float32)))


def _check(case, got, x, sr):
    r64, r32 = _ref(x, sr)
    p = R.plan(len(x), sr)
    assert got.dtype == np.float32 and got.shape == r64.shape == (p["size"],), (case, got.shape, r64.shape)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    assert np.isfinite(got).all(), case
    assert (got[p["n_out"]:] == 0).all() and not np.signbit(got[p["n_out"]:]).any(), case
    d32 = float(np.abs(r32.astype(np.float64) - r64).max())
    unit = max(d32, 2.0 ** -23 * float(np.abs(r64).max()))
    err = float(np.abs(got.astype(np.float64) - r64).max())
    ratio = err / unit if unit > 0 else (0.0 if err == 0 else float("inf"))
    print(f"audio case {case} {sr} -> {R.SR} n {len(x)} outputs {p['n_out']} + {p['size'] - p['n_out']}: err {err:.3e} d32 {d32:.3e} "
          f"unit {unit:.3e} ratio {ratio:.2f}")
    assert err <= FACTOR * unit, (case, err, unit)


def _run(y, sr):
    out = A.resample(y, sr)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case,sr,n", [("R1", 44100, 50), ("R2", 44100, 735), ("R3", 48000, 1203), ("R4", 22050, 700), ("R5", 8000, 300),
                                       ("R6", 192000, 4000), ("R7", 245760, 4096)])
def test_resample_single(case, sr, n):
    x = R.signal(n, sr, seed=int(case[1]))
    p = R.plan(n, sr)
    out = _run(torch.from_numpy(x).to(DEV), sr)
    assert out.shape == (1, p["size"])
    if case in ("R1", "R2"):
        assert p["size"] == p["n_out"] + 1                # the trailing zero
    if case == "R2":
        assert (p["n_out"], p["size"]) == (511, 512)
    _check(case, out[0].cpu().numpy(), x, sr)
    assert _same_bits(out, _run(torch.from_numpy(x).to(DEV)[None], sr))


def test_resample_batch_through_a_row_stride():
    sr, n, ld = 44100, 1500, 1537
    clips = [R.signal(n, sr, seed=81), np.zeros(n, np.float32), R.signal(n, sr, seed=83)]
    buf = torch.full((3, ld), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :n] = torch.from_numpy(np.stack(clips)).to(DEV)
    y = buf[:, :n]
    assert y.stride() == (ld, 1)
    out = _run(y, sr)
    assert out.shape == (3, R.plan(n, sr)["size"])
    for b, x in enumerate(clips):
        _check(f"R8.{b}", out[b].cpu().numpy(), x, sr)
        assert _same_bits(out[b], _run(torch.from_numpy(x).to(DEV), sr)[0])
    assert (_bits(out[1]) == 0).all()                     # the silent row: exact zeros
    assert _same_bits(out, _run(y, sr))


def test_resample_overlapping_rows():
    sr = 44100
    x = R.signal(6000, sr, seed=9)
    y = torch.from_numpy(x).to(DEV)
    rows = A.slice_audio(y, sr, stride=0.01, length=0.05)
    assert rows.shape == (9, 2205) and rows.stride() == (441, 1) and rows.data_ptr() == y.data_ptr()
    out = _run(rows, sr)
    for s in range(rows.shape[0]):
        _check(f"R9.{s}", out[s].cpu().numpy(), x[441 * s:441 * s + 2205], sr)
        assert _same_bits(out[s], _run(rows[s].clone(), sr)[0])


def test_resample_refusals_and_identity():
    y = torch.zeros(2, 4000, device=DEV)
    with pytest.raises(L.TcdiffError, match="too short"):
        A.resample(y[:, :1], 44100)
    with pytest.raises(L.TcdiffError, match="at most 8"):
        A.resample(y, 245761)
    with pytest.raises(L.TcdiffError, match="at most 8"):
        A.resample(y, 30720 * 9)
    assert A.resample(y, 30720) is y and A.resample(y, 44100, 44100) is y
    assert A.resample(y, 30720 * 8).shape == (2, 500)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _song():
    def make():
        frames, sr = 9000, 44100
        left, right = R.signal(frames, sr, seed=21), R.signal(frames, sr, seed=22)
        pcm = np.round(np.stack([left, right], 1) * 32767.0).astype(np.int64)
        return R.wav_file(R.pack(pcm, "s16"), "s16", 2, sr, before=[R.chunk(b"LIST", b"INFOabc")])
    return _once("song", make)


def test_load_audio_is_its_parts():
    raw = _song()
    wav = A.read_wav(raw)
    assert (wav.sr, wav.channels, wav.frames, wav.fmt) == (44100, 2, 9000, "s16")
    mono = A.decode(wav, DEV)
    want = R.to_mono(R.decode(wav.data, "s16", 2))
    assert np.array_equal(mono[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    parts = A.resample(mono, wav.sr)
    got = A.load_audio(raw, device=DEV)
    assert got.shape == (1, 6270) and _same_bits(got, parts)
    assert _same_bits(A.load_audio([raw, wav], device=DEV), torch.cat([parts, parts]))
    _check("load_audio", got[0].cpu().numpy(), want, wav.sr)
    assert A.load_audio(raw, sr=44100, device=DEV).shape == (1, 9000)


def test_load_audio_slices_are_resampled_slices():
    raw = _song()
    wav = A.read_wav(raw)
    rows = A.slice_audio(A.decode(wav, DEV)[0], wav.sr, 0.02, 0.1)
    assert rows.shape == (6, 4410) and rows.stride() == (882, 1)
    got = A.load_audio(raw, slices=(0.02, 0.1), device=DEV)
    assert got.shape == (6, R.plan(4410, wav.sr)["size"]) and _same_bits(got, A.resample(rows, wav.sr))
    for s in range(6):                                    # each slice has its own edges: it is the slice resampled alone
        assert _same_bits(got[s], A.resample(rows[s].clone(), wav.sr)[0])
    with pytest.raises(L.TcdiffError, match="shorter than one slice"):
        A.load_audio(raw, slices=(0.5, 5.0), device=DEV)


def test_wav_cond_is_music_cond_of_load_audio():
    raw = _song()
    cond = MU.wav_cond(raw)
    assert cond.shape == (1, 13, 438) and cond.dtype == torch.float32
    assert _same_bits(cond, MU.music_cond(A.load_audio(raw, device=DEV)))
    assert torch.isfinite(cond).all()
