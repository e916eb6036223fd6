"""tcdiff_amd.audio without a GPU: the WAV parser on files made with the standard library's ``wave`` and by hand with ``struct``,
and the numpy restatement tests/audio_ref.py held to things it was not written from -- resampy's output lengths, an analytic
sine, the DC gain that resampy's truncated table step leaves, the number of taps per output -- plus the host side of the
package's functions (plan, table, slicing, argument checks, no CPU fallback).  Measured figures: profiles/audio.txt."""
import io
import os
import struct
import wave

import numpy as np
import pytest
import torch

import audio_ref as R
import tcdiff_amd
from tcdiff_amd import _lib as L
from tcdiff_amd import audio as A
from tcdiff_amd import music as MU

# max |resampled - analytic| over the middle fifth of the output of a 1 kHz unit sine, measured with the float64 restatement
# (profiles/audio.txt); asserted at 4x, a margin that covers only another phase or length of the test signal
SINE_MEASURED = {22050: 6.2e-8, 8000: 2.8e-7}


# ---- the parser ------------------------------------------------------------------------------------------------------------------
def _wave_module(width, channels, sr, frames, seed):
    data = np.random.default_rng(seed).integers(0, 256, frames * channels * width, dtype=np.uint8).tobytes()
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(data)
    return buf.getvalue(), data


@pytest.mark.parametrize("width,fmt", [(1, "u8"), (2, "s16"), (3, "s24"), (4, "s32")])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_read_wav_wave_module(width, fmt, channels):
    raw, data = _wave_module(width, channels, 44100, 37, seed=width * 10 + channels)
    w = A.read_wav(raw)
    assert isinstance(w, A.WavData)
    assert (w.sr, w.channels, w.frames, w.fmt) == (44100, channels, 37, fmt) and w.data == data


def test_read_wav_from_a_path(tmp_path):
    raw, data = _wave_module(2, 2, 48000, 11, seed=1)
    p = tmp_path / "a.wav"
    p.write_bytes(raw)
    for path in (p, str(p)):
        w = A.read_wav(path)
        assert (w.sr, w.channels, w.frames, w.fmt, w.data) == (48000, 2, 11, "s16", data)
    assert A.read_wav(bytearray(raw)) == A.read_wav(raw) == A.read_wav(memoryview(raw))
    with pytest.raises(L.TcdiffError, match="cannot read"):
        A.read_wav(tmp_path / "missing.wav")
    with pytest.raises(L.TcdiffError, match="path or bytes"):
        A.read_wav(5)


def test_read_wav_hand_made():
    f32 = R.pack(np.linspace(-1, 1, 10), "f32")
    w = A.read_wav(R.wav_file(f32, "f32", 2, 22050))
    assert (w.sr, w.channels, w.frames, w.fmt, w.data) == (22050, 2, 5, "f32", f32)
    f64 = R.pack(np.linspace(-1, 1, 9), "f64")
    w = A.read_wav(R.wav_file(f64, "f64", 3, 8000))
    assert (w.sr, w.channels, w.frames, w.fmt, w.data) == (8000, 3, 3, "f64", f64)
    # extensible: the sub-format gives the tag, PCM and float
    s24 = R.pack(np.arange(-6, 6) * 70001, "s24")
    w = A.read_wav(R.wav_file(s24, "s24", 2, 96000, extensible=True))
    assert (w.sr, w.channels, w.frames, w.fmt, w.data) == (96000, 2, 6, "s24", s24)
    w = A.read_wav(R.wav_file(f32, "f32", 1, 44100, extensible=True))
    assert (w.frames, w.fmt, w.data) == (10, "f32", f32)
    # a LIST chunk and an odd-sized chunk (with its pad byte) before the data
    s16 = R.pack(np.arange(-8, 8) * 1000, "s16")
    w = A.read_wav(R.wav_file(s16, "s16", 1, 44100, before=[R.chunk(b"LIST", b"INFOISFT\x05\0\0\0abcd\0\0"), R.chunk(b"odd ", b"abc")]))
    assert (w.frames, w.fmt, w.data) == (16, "s16", s16)
    # a chunk after the data is not read; an odd-sized data chunk keeps its bytes
    u8 = R.pack(np.arange(7), "u8")
    body = R.wav_file(u8, "u8", 1, 8000) + b"\0" + R.chunk(b"LIST", b"xx")
    w = A.read_wav(body)
    assert (w.frames, w.data) == (7, u8)
    # data size 0 and 0xFFFFFFFF: to the end of the file
    for size in (0, 0xFFFFFFFF):
        w = A.read_wav(R.wav_file(s16, "s16", 2, 44100, data_size=size))
        assert (w.frames, w.data) == (8, s16)
    # a truncated last frame is dropped: by the declared size, and by the end of the file
    w = A.read_wav(R.wav_file(s16, "s16", 3, 44100))
    assert (w.frames, w.data) == (5, s16[:30])
    w = A.read_wav(R.wav_file(s16[:-1], "s16", 2, 44100, data_size=32))
    assert (w.frames, w.data) == (7, s16[:28])
    # no frame at all is a file, too (decode refuses it)
    w = A.read_wav(R.wav_file(b"", "s16", 2, 44100))
    assert (w.frames, w.data) == (0, b"")


def _riff(body):
    return b"RIFF" + struct.pack("<I", len(body)) + body


@pytest.mark.parametrize("raw,match", [
    (b"RF64" + b"\xff" * 4 + b"WAVE" + b"\0" * 40, "RF64"),
    (b"FORM" + b"\0\0\0\x20" + b"AIFF" + b"\0" * 40, "AIFF"),
    (b"RIFX" + b"\0" * 4 + b"WAVE" + b"\0" * 40, "RIFX"),
    (b"RIFF" + b"\0" * 4 + b"AVI " + b"\0" * 40, "AVI"),
    (b"RIFF\0\0", "6 bytes"),
    (R.wav_file(b"\0" * 8, "s16", 2, 44100, tag=0x55), "0x0055"),                  # MPEG layer 3
    (R.wav_file(b"\0" * 8, "s16", 2, 44100, tag=2), "0x0002"),                     # ADPCM
    (R.wav_file(b"\0" * 8, "s16", 2, 44100, tag=7, extensible=True), "0x0007"),    # mu-law behind an extensible header
    (R.wav_file(b"\0" * 8, "s16", 2, 44100, tag=3), "16 bits"),                    # no 16-bit float
    (R.wav_file(b"\0" * 8, "f64", 1, 44100, tag=1), "64 bits"),                    # no 64-bit PCM
    (R.wav_file(b"\0" * 8, "s16", 2, 44100, block_align=6), "block_align 6"),
    (R.wav_file(b"\0" * 8, "s16", 0, 44100), "0 channels"),
    (_riff(b"WAVE" + R.chunk(b"data", b"\0" * 8)), "before any fmt"),
    (_riff(b"WAVE" + R.chunk(b"LIST", b"abcd")), "no fmt chunk"),
    (_riff(b"WAVE" + R.fmt_chunk("s16", 2, 44100) + R.chunk(b"LIST", b"abcd")), "no data chunk"),
    (_riff(b"WAVE" + b"fmt " + struct.pack("<I", 14) + b"\0" * 14), "fmt chunk of 14"),
])
def test_read_wav_malformed(raw, match):
    with pytest.raises(L.TcdiffError, match=match):
        A.read_wav(raw)


# ---- the restatement, held to what it was not written from ----------------------------------------------------------------
def test_resample_lengths():
    for (n, sr), want in {(220500, 44100): (153600, 153600), (240000, 48000): (153600, 153600), (735, 44100): (511, 512),
                          (2, 44100): (1, 2)}.items():
        p, q = R.plan(n, sr), A.resample_plan(n, sr)
        assert (p["n_out"], p["size"]) == want and (q["n_out"], q["size"]) == want
        assert all(p[k] == q[k] for k in ("ratio", "inc", "scale", "step"))
    with pytest.raises(ValueError):
        R.plan(1, 44100)
    with pytest.raises(L.TcdiffError, match="too short"):
        A.resample_plan(1, 44100)
    y = R.resample(R.signal(735, 44100, 0), 44100)
    assert y.shape == (512,) and y[510] != 0 and y[511] == 0
    assert [R.plan(1000, sr)["step"] for sr in (44100, 48000, 192000, 245760, 22050, 8000)] == [356, 327, 81, 64, 512, 512]


@pytest.mark.parametrize("sr,n", [(22050, 4410), (8000, 1600)])
def test_upsampled_sine_is_the_analytic_sine(sr, n):
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)
    y = R.resample(x, sr)
    m = len(y)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(m) / R.SR)
    err = float(np.abs(y - want)[2 * m // 5:3 * m // 5].max())
    print(f"audio sine {sr} -> {R.SR}: n {n}, {m} outputs, middle fifth max error {err:.3e} (measured {SINE_MEASURED[sr]:.1e})")
    assert err <= 4 * SINE_MEASURED[sr]


@pytest.mark.parametrize("sr,n,bound,band", [(22050, 2000, 1e-7, None), (8000, 1000, 1e-7, None), (44100, 2000, 2e-3, (1.00055, 1.00078)),
                                             (48000, 2000, 2e-3, (1.00075, 1.00095)), (192000, 6000, 2e-2, (1.00963, 1.00965))])
def test_dc_gain_keeps_resampys_truncated_step(sr, n, bound, band):
    y = R.resample(np.ones(n), sr)
    m = R.plan(n, sr)["n_out"]
    g = y[m // 3:2 * m // 3]
    print(f"audio dc gain {sr} -> {R.SR}: {g.min():.7f} .. {g.max():.7f}")
    assert np.abs(g - 1).max() < bound
    if band is not None:                                  # a "corrected" filter would give 1
        assert band[0] - 1e-5 <= g.min() and g.max() <= band[1] + 1e-5 and g.min() > 1.0004


def test_taps_per_output():
    assert R.max_taps(2000, 44100) == 183 and R.max_taps(2000, 48000) == 199 and R.max_taps(6000, 192000) == 808
    assert R.max_taps(2000, 22050) == 127 and R.max_taps(1000, 8000) == 127
    ix = R.indices(50, 44100)                             # a short clip: every wing cut by an end of the signal
    assert (ix["left"][2] == ix["n"] + 1).all() and (ix["right"][2] == 50 - ix["n"] - 1).all()
    for n, sr in ((735, 44100), (4096, 245760), (300, 8000)):      # every table index and every sample index stays inside
        ix = R.indices(n, sr)
        for off, eta, cnt in (ix["left"], ix["right"]):
            assert (off >= 0).all() and (off + (np.maximum(cnt, 1) - 1) * ix["step"] <= R.N).all() and (0 <= eta).all() and (eta < 1).all()
        assert (ix["n"] - (ix["left"][2] - 1) >= 0).all() and (ix["n"] + ix["right"][2] <= n - 1).all()


def test_float32_run_is_close_to_the_float64_run():
    x = R.signal(1203, 48000, 3)
    y64, y32 = R.resample(x, 48000), R.resample(x, 48000, dtype=np.float32)
    assert y32.dtype == np.float32 and y64.dtype == np.float64
    assert 0 < np.abs(y32 - y64).max() < 2e-6


def test_decode_restatement():
    assert np.array_equal(R.decode(R.pack([0, 128, 255], "u8"), "u8", 1)[:, 0], np.float32([-1, 0, 127 / 128]))
    assert np.array_equal(R.decode(R.pack([-32768, 32767, -1], "s16"), "s16", 1)[:, 0], np.float32([-1, 32767 / 32768, -1 / 32768]))
    assert np.array_equal(R.decode(R.pack([-(1 << 23), (1 << 23) - 1, -1], "s24"), "s24", 1)[:, 0],
                          np.float32([-1, 1 - 2.0 ** -23, -2.0 ** -23]))
    # 2^24 + 1 is a tie and goes to the even 2^24; 2^24 + 3 is a tie and goes to the even 2^24 + 4
    got = R.decode(R.pack([(1 << 24) + 1, (1 << 24) + 3, -(1 << 31), (1 << 31) - 1], "s32"), "s32", 1)[:, 0]
    assert np.array_equal(got, np.float32([2.0 ** -7, (2.0 ** 24 + 4) * 2.0 ** -31, -1, 1]))
    got = R.decode(R.pack([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -0.0], "f64"), "f64", 1)[:, 0]
    assert np.array_equal(got, np.float32([1, 1 + 2.0 ** -22, 0])) and np.signbit(got[2])
    x = R.decode(R.pack([1, 2, 4, -3, -3, -3], "s16"), "s16", 3)
    assert x.shape == (2, 3) and np.array_equal(R.to_mono(x), np.float32([np.float32(7 / 32768) / np.float32(3), -3 / 32768]))
    one = R.decode(R.decode_case("f32", 1, 9, 0), "f32", 1)
    assert np.array_equal(R.to_mono(one).view(np.uint32), one[:, 0].view(np.uint32))      # C = 1 passes through, -0.0 included


# ---- the package's host side ---------------------------------------------------------------------------------------------------
def test_table_and_constants():
    for ratio in (30720 / 44100, 30720 / 22050):
        tab = A.resample_table(ratio)
        win, delta = R.table(ratio)
        assert tab.shape == (L.AUDIO_TABLE, 2) and tab.dtype == np.float64
        assert np.abs(tab[:, 0] - win).max() <= 1e-16 and np.abs(tab[:, 1] - delta).max() <= 1e-16 and tab[-1, 1] == 0
    assert abs(A.resample_table(2.0)[0, 0] - R.ROLLOFF) < 1e-15
    assert (A.ROLLOFF, A.BETA, A.PRECISION, A.N_TABLE, A.SR) == (R.ROLLOFF, R.BETA, R.PRECISION, R.NWIN, R.SR)
    assert L.AUDIO_FMT == {"u8": 0, "s16": 1, "s24": 2, "s32": 3, "f32": 4, "f64": 5}
    header = open(os.path.join(os.path.dirname(L.HERE), "include", "tcdiff_hip.h")).read()
    for name, v in (("TC_AUDIO_U8", 0), ("TC_AUDIO_F64", 5), ("TC_AUDIO_MIN_STEP", L.AUDIO_MIN_STEP), ("TC_AUDIO_PRECISION", L.AUDIO_PRECISION)):
        assert f"#define {name} {v}" in header
    assert "#define TC_AUDIO_TABLE (512 * 64 + 1)" in header and L.AUDIO_TABLE == 512 * 64 + 1
    lib = L.load()
    for sym in ("tcdiff_audio_decode", "tcdiff_audio_resample"):
        assert sym in L.EXPORTS and hasattr(lib, sym)
    for name in ("WavData", "read_wav", "decode", "resample", "slice_audio", "load_audio"):
        assert name in tcdiff_amd.__all__ and getattr(tcdiff_amd, name) is getattr(A, name)
    assert "wav_cond" in tcdiff_amd.__all__ and tcdiff_amd.wav_cond is MU.wav_cond


@pytest.mark.parametrize("n", [0, 100, 219, 220, 221, 263, 264, 265, 1000, 1011, 1012])
def test_slice_audio_is_the_reference_loop(n):
    sr, stride, length = 441, 0.1, 0.5                    # window 220, step 44
    y = torch.arange(n, dtype=torch.float32)
    window, step, starts = R.slice_starts(n, sr, stride, length)
    assert (window, step) == (220, 44)
    rows = A.slice_audio(y, sr, stride, length)
    assert rows.shape == (len(starts), window)
    if n >= window:
        assert rows.data_ptr() == y.data_ptr() and rows.stride() == (step, 1)
    for r, s in zip(rows, starts):
        assert torch.equal(r, y[s:s + window])
    assert list(A.slice_starts(n, sr, stride, length)[2]) == starts


def test_slice_audio_at_the_reference_arguments():
    window, step, starts = R.slice_starts(48000 * 180, 48000, 0.5, 5)
    assert (window, step, len(starts)) == (240000, 24000, 351)
    assert A.slice_audio(torch.zeros(44100 * 6), 44100).shape == (3, 220500)
    with pytest.raises(L.TcdiffError, match="window"):
        A.slice_audio(torch.zeros(100), 44100, stride=0.0)
    with pytest.raises(L.TcdiffError, match=r"\(n,\)"):
        A.slice_audio(torch.zeros(2, 100), 10)


def test_argument_checks_and_no_cpu_fallback():
    wav = A.read_wav(R.wav_file(R.pack(np.arange(40), "s16"), "s16", 2, 44100))
    with pytest.raises(L.TcdiffError, match="MI355X"):
        A.decode(wav, "cpu")
    with pytest.raises(L.TcdiffError, match="MI355X"):
        A.load_audio(wav, device="cpu")
    with pytest.raises(L.TcdiffError, match="MI355X"):
        MU.wav_cond(wav, device="cpu")
    with pytest.raises(L.TcdiffError, match="MI355X"):
        A.resample(torch.zeros(2, 100), 44100)
    with pytest.raises(L.TcdiffError, match="no frame"):
        A.decode(A.read_wav(R.wav_file(b"", "s16", 2, 44100)), "cpu")
    with pytest.raises(L.TcdiffError, match="no file"):
        A.decode([], "cpu")
    others = [wav._replace(sr=48000), wav._replace(fmt="u8", data=wav.data[:40]), wav._replace(channels=1, data=wav.data[:40]),
              A.read_wav(R.wav_file(R.pack(np.arange(38), "s16"), "s16", 2, 44100))]
    for other in others:
        with pytest.raises(L.TcdiffError, match="file 2 .* differs from file 0"):
            A.decode([wav, wav, other, other], "cpu")
    with pytest.raises(L.TcdiffError, match="file 1 holds"):
        A.decode([wav, wav._replace(frames=19)], "cpu")
    with pytest.raises(L.TcdiffError, match="exactly one file"):
        A.load_audio([wav, wav], slices=(0.5, 5.0), device="cpu")
    with pytest.raises(L.TcdiffError, match="slices must be"):
        A.load_audio(wav, slices=5.0, device="cpu")
    y = torch.zeros(2, 100)
    assert A.resample(y, 30720) is y and A.resample(y[0], 44100, 44100).data_ptr() == y.data_ptr()
    with pytest.raises(L.TcdiffError, match="too short"):
        A.resample(torch.zeros(1), 44100)
    with pytest.raises(L.TcdiffError, match="at most 8"):
        A.resample(torch.zeros(4000), 245761)
    A.resample_plan(4096, 245760)                         # the limit itself is inside
    with pytest.raises(L.TcdiffError, match="float32"):
        A.resample(torch.zeros(100, dtype=torch.float64), 44100)
    with pytest.raises(L.TcdiffError, match="contiguous"):
        A.resample(torch.zeros(2, 200)[:, ::2], 44100)
    with pytest.raises(L.TcdiffError, match=r"\(n,\) or \(B, n\)"):
        A.resample(torch.zeros(1, 2, 100), 44100)
    for bad in (0, -1, "x", float("nan"), None, True):
        with pytest.raises(L.TcdiffError, match="positive number"):
            A.resample(y, bad)
