"""``librosa.load(wav_path, sr=30720)`` restated from the definitions in include/tcdiff_hip.h with numpy: soundfile's decode to
float32, librosa.to_mono, and ``librosa.resample(res_type="kaiser_best", fix=True, scale=False)`` over resampy's interpolating
resampler (its ``tr = t * inc`` form).  ``resample`` takes ``dtype``: float64 is the yardstick of tests/test_audio_gpu.py,
float32 (float32 tables, weights and a sequential sum, left wing then right wing) its error scale.  The byte builders below make
data chunks and whole RIFF/WAVE files with ``struct`` and numpy alone; nothing here imports tcdiff_amd.

Neither librosa, resampy nor soundfile is installed where this project is built: the definitions are written from knowledge of
those versions, and parity with their own output is NOT pinned by anything here."""
import math
import struct

import numpy as np

SR = 30720
ROLLOFF, BETA, PRECISION, N_ZEROS = 0.9475937167399596, 14.769656459379492, 512, 64      # resampy's kaiser_best
N = PRECISION * N_ZEROS
NWIN = N + 1
SAMPLE_BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}
FORMAT_TAG = {"u8": 1, "s16": 1, "s24": 1, "s32": 1, "f32": 3, "f64": 3}


# ---- bytes ---------------------------------------------------------------------------------------------------------------------
def pack(values, fmt) -> bytes:
    """samples in file order (frames x channels, flattened) -> little-endian bytes: integers for the PCM formats (u8: 0 .. 255,
    the others two's complement), floats for f32 / f64"""
    v = np.asarray(values).ravel()
    if fmt == "u8":
        return v.astype(np.uint8).tobytes()
    if fmt == "s16":
        return v.astype("<i2").tobytes()
    if fmt == "s24":
        u = v.astype(np.int64) & 0xFFFFFF
        return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], 1).astype(np.uint8).tobytes()
    if fmt == "s32":
        return v.astype("<i4").tobytes()
    return v.astype("<f4" if fmt == "f32" else "<f8").tobytes()


def fmt_chunk(fmt, channels, sr, *, extensible=False, block_align=None, tag=None) -> bytes:
    bits = 8 * SAMPLE_BYTES[fmt]
    align = channels * SAMPLE_BYTES[fmt] if block_align is None else block_align
    tag = FORMAT_TAG[fmt] if tag is None else tag
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, sr, sr * align, align, bits)
    if extensible:                                        # cbSize, valid bits, channel mask, the sub-format GUID (tag first)
        body += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    return b"fmt " + struct.pack("<I", len(body)) + body


def chunk(cid, body) -> bytes:
    """a chunk with its pad byte after an odd size"""
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def wav_file(data, fmt, channels, sr, *, before=(), data_size=None, **kw) -> bytes:
    """a RIFF/WAVE file: the fmt chunk, the chunks of ``before``, then ``data`` (declared as ``data_size`` bytes when given)"""
    body = b"WAVE" + fmt_chunk(fmt, channels, sr, **kw) + b"".join(before)
    body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


# ---- decode and downmix --------------------------------------------------------------------------------------------------------
def decode(data, fmt, channels) -> np.ndarray:
    """the data chunk's bytes -> (frames, channels) float32, per sample as the header's table"""
    raw = np.frombuffer(data, np.uint8)
    if fmt == "u8":
        x = (raw.astype(np.int32) - 128).astype(np.float32) / np.float32(128)
    elif fmt == "s16":
        x = np.frombuffer(data, "<i2").astype(np.float32) / np.float32(2.0 ** 15)
    elif fmt == "s24":
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / np.float32(2.0 ** 23)
    elif fmt == "s32":
        x = np.frombuffer(data, "<i4").astype(np.float32) * np.float32(2.0 ** -31)     # int -> float32: nearest even
    elif fmt == "f32":
        x = np.frombuffer(data, "<f4").astype(np.float32)
    else:
        x = np.frombuffer(data, "<f8").astype(np.float32)                              # nearest even
    return x.reshape(-1, channels)


def to_mono(x) -> np.ndarray:
    """(frames, C) float32 -> (frames,): numpy's float32 mean, s = x_0, s = fl32(s + x_c), fl32(s / C); C = 1 passes through"""
    assert x.dtype == np.float32
    if x.shape[1] == 1:
        return x[:, 0].copy()
    s = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        s = (s + x[:, c]).astype(np.float32)
    return (s / np.float32(x.shape[1])).astype(np.float32)


def decode_case(fmt, channels, frames, seed) -> bytes:
    """a data chunk for the decode tests: seeded samples over the format's whole range, with the format's special values first
    (the extremes of the integer types, the s32 values that must round with their ties, the f64 values that round, -0.0)"""
    rng = np.random.default_rng(seed)
    n = frames * channels
    if fmt in ("u8", "s16", "s24", "s32"):
        bits = 8 * SAMPLE_BYTES[fmt]
        lo, hi = (0, 255) if fmt == "u8" else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
        v = rng.integers(lo, hi + 1, size=n, dtype=np.int64)
        special = [lo, hi, 0 if fmt != "u8" else 128, -1 if fmt != "u8" else 127, 1 if fmt != "u8" else 129]
        if fmt == "s32":                                  # 25 significant bits: ties to even, up and down; and beyond a tie
            special += [(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, -(1 << 24) - 3, (1 << 25) + 3, (1 << 30) + 65, hi - 63, hi - 64]
        special = np.array(special, np.int64)
    else:
        v = rng.uniform(-1.0, 1.0, size=n)
        if fmt == "f32":
            v = v.astype(np.float32)
            special = np.array([-0.0, 1.0, -1.0, np.finfo(np.float32).tiny, 2.0 ** -149, 3.0e38], np.float32)
        else:                                             # halfway between two floats (even below, even above), and off a tie
            special = np.array([-0.0, 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, -1.0 - 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 0.1,
                                1.0 / 3.0, 2.0 ** -150, 1.0e-310])
    # rotate the special values by the seed so that a one-frame case does not always hold the same one
    k = min(n, len(special))
    v[:k] = np.roll(special, -seed)[:k]
    return pack(v, fmt)


# ---- resample ------------------------------------------------------------------------------------------------------------------
def plan(n, sr_orig, sr_new=SR) -> dict:
    """the host side, Python's own float64 expressions; raises ValueError where resampy does (n_out < 1)"""
    ratio = float(sr_new) / sr_orig
    n_out = int(n * ratio)
    if n_out < 1:
        raise ValueError(f"{n} samples at {sr_orig} Hz are too short to be resampled to {sr_new} Hz")
    scale = min(1.0, ratio)
    return dict(ratio=ratio, n_out=n_out, size=int(math.ceil(n * ratio)), inc=1.0 / ratio, scale=scale, step=int(scale * PRECISION))


def table(ratio):
    """(win, delta), float64, m = 0 .. N"""
    win = ROLLOFF * np.sinc(ROLLOFF * np.arange(NWIN) / PRECISION) * np.kaiser(2 * N + 1, BETA)[N:]
    if ratio < 1:
        win = win * ratio
    delta = np.zeros(NWIN)
    delta[:-1] = win[1:] - win[:-1]
    return win, delta


def indices(n, sr_orig, sr_new=SR) -> dict:
    """per output t < n_out, in float64: n, and (off, eta, count) of the left and of the right wing"""
    p = plan(n, sr_orig, sr_new)
    t = np.arange(p["n_out"], dtype=np.float64)
    tr = t * p["inc"]
    nn = tr.astype(np.int64)
    frac = p["scale"] * (tr - nn)
    f = frac * PRECISION
    off_l = f.astype(np.int64)
    eta_l = f - off_l
    cnt_l = np.minimum(nn + 1, (NWIN - off_l) // p["step"])
    f = (p["scale"] - frac) * PRECISION
    off_r = f.astype(np.int64)
    eta_r = f - off_r
    cnt_r = np.maximum(np.minimum(n - nn - 1, (NWIN - off_r) // p["step"]), 0)
    return dict(p, n=nn, left=(off_l, eta_l, cnt_l), right=(off_r, eta_r, cnt_r))


def max_taps(n, sr_orig, sr_new=SR) -> int:
    ix = indices(n, sr_orig, sr_new)
    return int((ix["left"][2] + ix["right"][2]).max())


def resample(x, sr_orig, sr_new=SR, dtype=np.float64) -> np.ndarray:
    """x (n,) -> (size,) of ``dtype``; every weight, product and sum in ``dtype``, one rounding each, in the order the header
    writes them; samples n_out .. size - 1 are 0"""
    x = np.asarray(x).astype(dtype)
    n = len(x)
    ix = indices(n, sr_orig, sr_new)
    win, delta = (a.astype(dtype) for a in table(ix["ratio"]))
    step, nn = ix["step"], ix["n"]
    y = np.zeros(ix["size"], dtype)
    acc = np.zeros(ix["n_out"], dtype)
    for (off, eta, cnt), sign, first in ((ix["left"], -1, 0), (ix["right"], 1, 1)):
        eta = eta.astype(dtype)
        for i in range(int(cnt.max()) if len(cnt) else 0):
            live = np.nonzero(i < cnt)[0]
            at = off[live] + i * step
            w = (win[at] + (eta[live] * delta[at]).astype(dtype)).astype(dtype)
            acc[live] = (acc[live] + (w * x[nn[live] + sign * i + first]).astype(dtype)).astype(dtype)
    y[:ix["n_out"]] = acc
    return y


def signal(n, sr, seed) -> np.ndarray:
    """n float32 samples, |x| <= 1: seeded uniform noise plus two sines"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = 0.35 * np.sin(2 * np.pi * 440.0 * t + rng.uniform(0, 2 * np.pi)) + 0.3 * np.sin(2 * np.pi * 0.11 * sr * t + rng.uniform(0, 2 * np.pi))
    return (x + 0.35 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)


def slice_starts(n, sr, stride, length):
    """the loop of data/slice.py:16-23 -> (window, step, starts)"""
    window, step, start, starts = int(length * sr), int(stride * sr), 0, []
    while start <= n - window:
        starts.append(start)
        start += step
    return window, step, starts
