"""The Motion-JPEG encoder of include/tcdiff_mjpeg.h restated in numpy integers (colour -> subsampling -> DCT -> quantiser ->
Huffman symbols -> bytes), written from the header: the GPU tests hold ``encode_jpeg`` to these bytes and the CPU tests hold these
bytes to libjpeg through Pillow.  Also a walker for AVI 1.0 files written from the RIFF layout, and the seeded frames that
tests/test_mjpeg_cpu.py and tests/test_mjpeg_gpu.py share."""
import functools
import io
import math
import struct
import wave
from collections import Counter
from fractions import Fraction

import numpy as np
from PIL import Image

HEADER_BYTES = 625
DCT_BITS, COEF_BITS, DCT_BOUND = 14, 20, 0.2
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
BASE = np.array([[16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                  100, 103, 99],
                 [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66] + [99] * 38])
# Annex K.3: the counts per code length, then the values in code order; [0] luminance, [1] chrominance
DC_BITS = [bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])]
DC_VALS = bytes(range(12))
AC_BITS = [bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]), bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])]
AC_VALS = [bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")]


def dct_matrix_real():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    return np.where(k == 0, math.sqrt(1 / 8), 0.5) * np.cos((2 * n + 1) * k * math.pi / 16)


M = np.floor(np.abs(dct_matrix_real()) * 2 ** DCT_BITS + 0.5).astype(np.int64) * np.sign(dct_matrix_real()).astype(np.int64)


def quant_tables(quality):
    """the two tables in natural order, (2, 64) int"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE * scale + 50) // 100, 1, 255)


@functools.lru_cache(None)
def codes(kind, chroma):
    """symbol -> (code, length), Annex C"""
    bits, vals = (DC_BITS[chroma], DC_VALS) if kind == "dc" else (AC_BITS[chroma], AC_VALS[chroma])
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def ycc(rgb):
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32768) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32768) >> 16
    assert min(y.min(), cb.min(), cr.min()) >= 0
    return np.minimum(y, 255), np.minimum(cb, 255), np.minimum(cr, 255)


def planes(frame, sub):
    """the padded Y, Cb, Cr planes of one (H, W, 3) frame, chroma subsampled for "420" """
    H, W = frame.shape[:2]
    side = 16 if sub == "420" else 8
    yy = np.minimum(np.arange(-(-H // side) * side), H - 1)
    xx = np.minimum(np.arange(-(-W // side) * side), W - 1)
    y, cb, cr = ycc(frame[yy][:, xx])
    if sub == "420":
        cb, cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (cb, cr))
    return y, cb, cr


def blocks_of(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128          # (rows, cols, y, x), level shifted


def dct_int(s):
    """(..., 8, 8) level-shifted samples -> the coefficients with COEF_BITS fractional bits; every intermediate is checked to fit int32"""
    a = s.astype(np.int64) @ M.T
    t = (a + 128) >> 8
    c = M @ t
    assert max(np.abs(a).max(), np.abs(c).max()) < 2 ** 31 - 255 * 2 ** 19
    return c


def dct_float(s):
    A = dct_matrix_real()
    return A @ s.astype(np.float64) @ A.T


def quantise(c, table):
    """table (64,) natural order -> (..., 64) values in zigzag order, AC clamped"""
    t = table.reshape(8, 8).astype(np.int64)
    q = np.sign(c) * ((np.abs(c) + (t << (COEF_BITS - 1))) // (t << COEF_BITS))
    zz = q.reshape(q.shape[:-2] + (64,))[..., ZIGZAG]
    zz[..., 1:] = np.clip(zz[..., 1:], -1023, 1023)
    return zz


def coefficients(frame, quality, sub):
    qt = quant_tables(quality)
    return [quantise(dct_int(blocks_of(p)), qt[min(c, 1)]) for c, p in enumerate(planes(frame, sub))]


def header(W, H, sub, qt):
    out = bytes([0xFF, 0xD8, 0xFF, 0xE0, 0, 16]) + b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])
    out += bytes([0xFF, 0xDB, 0, 132, 0]) + bytes(qt[0][ZIGZAG].tolist()) + bytes([1]) + bytes(qt[1][ZIGZAG].tolist())
    out += bytes([0xFF, 0xC0, 0, 17, 8]) + struct.pack(">HH", H, W) + bytes([3, 1, 0x22 if sub == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for c in range(2):
        out += bytes([0xFF, 0xC4, 0, 31, c]) + DC_BITS[c] + DC_VALS + bytes([0xFF, 0xC4, 0, 181, 0x10 | c]) + AC_BITS[c] + AC_VALS[c]
    side = 16 if sub == "420" else 8
    out += bytes([0xFF, 0xDD, 0, 4]) + struct.pack(">H", -(-W // side)) + bytes([0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return out


def category(v):
    return int(abs(int(v))).bit_length()


def block_symbols(zz, d, chroma, stats=None):
    """[(bits, length)] of one block in stream order; ``stats`` counts what the block holds"""
    out = []
    s = category(d)
    code, n = codes("dc", chroma)[s]
    out.append((code << s | (d if d >= 0 else d + (1 << s) - 1), n + s))
    if stats is not None:
        stats[f"dc-category-{s}"] += 1
    ac, run = codes("ac", chroma), 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run >= 16:
            out.append(ac[0xF0])
            run -= 16
            if stats is not None:
                stats["zrl"] += 1
        s = category(v)
        code, n = ac[run << 4 | s]
        out.append((code << s | (v if v >= 0 else v + (1 << s) - 1), n + s))
        run = 0
    if run:
        out.append(ac[0])
    elif stats is not None:
        stats["no-eob"] += 1
    return out


def encode(frame, quality=90, sub="420", stats=None):
    """one (H, W, 3) uint8 frame -> the bytes of its JPEG stream"""
    frame = np.asarray(frame)
    H, W = frame.shape[:2]
    yq, cbq, crq = coefficients(frame, quality, sub)
    R, Mn = cbq.shape[:2] if sub == "420" else yq.shape[:2]
    out = [header(W, H, sub, quant_tables(quality))]
    for row in range(R):
        acc, nbits, pred = 0, 0, [0, 0, 0]
        for m in range(Mn):
            if sub == "420":
                mcu = [(0, yq[2 * row, 2 * m]), (0, yq[2 * row, 2 * m + 1]), (0, yq[2 * row + 1, 2 * m]), (0, yq[2 * row + 1, 2 * m + 1]),
                       (1, cbq[row, m]), (2, crq[row, m])]
            else:
                mcu = [(0, yq[row, m]), (1, cbq[row, m]), (2, crq[row, m])]
            for comp, zz in mcu:
                d = max(-2047, min(2047, int(zz[0]) - pred[comp]))
                pred[comp] = int(zz[0])
                for code, n in block_symbols(zz, d, int(comp > 0), stats):
                    acc, nbits = acc << n | code, nbits + n
        fill = -nbits % 8
        acc, nbits = acc << fill | ((1 << fill) - 1), nbits + fill
        data = acc.to_bytes(nbits // 8, "big")
        if stats is not None:
            stats["stuffed"] += data.count(b"\xff")
        out.append(data.replace(b"\xff", b"\xff\x00"))
        if row + 1 < R:
            out.append(bytes([0xFF, 0xD0 + row % 8]))
            if stats is not None:
                stats[f"rst{row % 8}"] += 1
                stats["rst-wrap"] += row >= 8
    out.append(b"\xff\xd9")
    return b"".join(out)


def encode_all(frames, quality=90, sub="420", stats=None):
    """(N, H, W, 3) -> (the concatenated streams, offsets (N + 1,) int64)"""
    streams = [encode(f, quality, sub, stats) for f in frames]
    return b"".join(streams), np.cumsum([0] + [len(s) for s in streams]).astype(np.int64)


# ---- the shared frames ---------------------------------------------------------------------------------------------------------------
def extreme_blocks():
    """the 64 sign-pattern blocks, one per basis function (v, u), each the extreme of its coefficient: (64, 8, 8) samples 0 / 255"""
    A = dct_matrix_real()
    return np.array([np.where(np.outer(A[v], A[u]) >= 0, 255, 0) for v in range(8) for u in range(8)], np.uint8)


@functools.lru_cache(None)
def case(name):
    """(N, H, W, 3) uint8, seeded"""
    rng = np.random.default_rng(sum(name.encode()))
    if name == "33x17":                                     # padding both ways: noise, a smooth ramp, flat white with a lone bright pixel
        f = np.empty((3, 17, 33, 3), np.uint8)
        f[0] = rng.integers(0, 256, (17, 33, 3))
        yy, xx = np.mgrid[0:17, 0:33]
        f[1] = np.stack([4 * xx + 3 * yy, 200 - 5 * xx + yy, 30 + 9 * yy], -1).clip(0, 255)
        f[2] = 255
        f[2, 3:5, 20:22] = 0
        f[2, 12, 2] = (255, 0, 0)
        return f
    if name == "16x80":                                     # 10 MCU rows at 4:4:4: every RSTm and the wrap
        return rng.integers(0, 256, (1, 80, 16, 3), dtype=np.uint8)
    if name == "8x8":
        return rng.integers(0, 256, (1, 8, 8, 3), dtype=np.uint8)
    if name == "1x1":
        return np.array([[[[200, 30, 90]]]], np.uint8)
    if name == "extreme":                                   # grey: Y is the sample; 8 x 8 blocks of 8 x 8 pixels
        b = extreme_blocks().reshape(8, 8, 8, 8).transpose(0, 2, 1, 3).reshape(64, 64)
        return np.repeat(b[None, :, :, None], 3, -1)
    if name == "checker":                                   # black / white alternation between blocks, and a dark sparse frame
        yy, xx = np.mgrid[0:32, 0:48]
        f = np.zeros((2, 32, 48, 3), np.uint8)
        f[0] = (((yy // 8 + xx // 8) % 2) * 255)[..., None]
        f[1, ::7, ::5] = rng.integers(0, 256, f[1, ::7, ::5].shape)
        return f
    if name == "seven":                                     # 7 frames of different content
        f = rng.integers(0, 256, (7, 24, 40, 3), dtype=np.uint8)
        for t in range(7):
            f[t, :, : 5 * t] = 30 * t
        return f
    raise KeyError(name)


CASES = ("33x17", "16x80", "8x8", "1x1", "extreme", "checker")
QUALITIES = (10, 90, 100)
SUBS = ("420", "444")


@functools.lru_cache(None)
def expected(name, quality, sub):
    """(bytes, offsets, Counter of what the symbol stream holds) of a shared case; computed once"""
    stats = Counter()
    data, offsets = encode_all(case(name), quality, sub, stats)
    return data, offsets, stats


def wide_frame(threads):
    """one frame, 8 rows high and 8 (threads + 3) wide: at 4:4:4 one interval holds 3 (threads + 3) blocks"""
    return np.random.default_rng(99).integers(0, 256, (1, 8, 8 * (threads + 3), 3), dtype=np.uint8)


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


# ---- AVI 1.0 ---------------------------------------------------------------------------------------------------------------------------
def _chunks(buf, start, end):
    """[(fourcc, payload offset, size)] of the chunks in buf[start:end]; every chunk starts on an even offset from `start`"""
    out, p = [], start
    while p < end:
        assert p + 8 <= end, "a chunk header runs past its list"
        fourcc, size = buf[p:p + 4], struct.unpack("<I", buf[p + 4:p + 8])[0]
        assert p + 8 + size <= end, (fourcc, size)
        out.append((fourcc, p + 8, size))
        p += 8 + size + (size & 1)
    assert p == end or p == end + 1, "padding to even sizes"
    return out


def walk_avi(buf):
    """an AVI 1.0 file -> dict: avih (the 14 dwords), streams [(strh fields, strf bytes)], movi [(fourcc, offset from the 'movi'
    fourcc, size, payload)], idx1 [(fourcc, flags, offset, size)], order (the top-level fourccs)"""
    assert buf[:4] == b"RIFF" and buf[8:12] == b"AVI " and struct.unpack("<I", buf[4:8])[0] == len(buf) - 8
    out = {"order": [], "streams": [], "movi": [], "idx1": []}
    for fourcc, p, size in _chunks(buf, 12, len(buf)):
        kind = buf[p:p + 4] if fourcc == b"LIST" else fourcc
        out["order"].append(kind)
        if kind == b"hdrl":
            inner = _chunks(buf, p + 4, p + size)
            assert inner[0][0] == b"avih" and inner[0][2] == 56
            out["avih"] = struct.unpack("<14I", buf[inner[0][1]:inner[0][1] + 56])
            for f2, p2, s2 in inner[1:]:
                assert f2 == b"LIST" and buf[p2:p2 + 4] == b"strl"
                (h, hp, hs), (f, fp, fs) = _chunks(buf, p2 + 4, p2 + s2)
                assert (h, hs, f) == (b"strh", 56, b"strf")
                names = ("fccType", "fccHandler", "dwFlags", "wPriority", "wLanguage", "dwInitialFrames", "dwScale", "dwRate", "dwStart",
                         "dwLength", "dwSuggestedBufferSize", "dwQuality", "dwSampleSize", "left", "top", "right", "bottom")
                out["streams"].append((dict(zip(names, struct.unpack("<4s4sIHHIIIIIIII4h", buf[hp:hp + 56]))), buf[fp:fp + fs]))
        elif kind == b"movi":
            out["movi_at"] = p
            for f2, p2, s2 in _chunks(buf, p + 4, p + size):
                out["movi"].append((f2, p2 - 8 - p, s2, buf[p2:p2 + s2]))
        elif kind == b"idx1":
            assert size % 16 == 0
            out["idx1"] = [struct.unpack("<4sIII", buf[p + 16 * k:p + 16 * k + 16]) for k in range(size // 16)]
    return out


# ---- what both test files ask of Pillow and of an AVI file --------------------------------------------------------------------------
PIL_SUB = {"444": 0, "420": 2}
# The decode's PSNR may fall below Pillow's own encoder's, at the same tables and the same box downsample, by the gap measured on
# the CPU plus 0.1 dB.  That gap (profiles/mjpeg.txt) is 0.46 dB, on one frame: the smooth ramp at 4:2:0, where the header's
# (a + b + c + d + 2) >> 2 rounds every chroma sample up and libjpeg alternates its bias between 1 and 2; at 4:4:4 the same frame is
# within 0.11 dB, and over all 84 frames the mean gap is -0.01 dB.  PSNRs are compared up to PSNR_CAP, the PSNR of rounding to 8 bits
# itself (a uniform error of variance 1 / 12): above it a difference measures the decoder's rounding.
PSNR_MARGIN = 0.46 + 0.1
PSNR_CAP = 10 * np.log10(255.0 ** 2 * 12)


def segments(stream):
    """[(marker, payload)] of a JPEG stream up to and including SOS"""
    assert stream[:2] == b"\xff\xd8"
    out, p = [], 2
    while True:
        assert stream[p] == 0xFF
        marker, n = stream[p + 1], struct.unpack(">H", stream[p + 2:p + 4])[0]
        out.append((marker, stream[p + 4:p + 2 + n]))
        p += 2 + n
        if marker == 0xDA:
            return out


def pillow_jpeg(frame, quality, sub):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=quality, subsampling=PIL_SUB[sub], optimize=False)
    return buf.getvalue()


def decode(stream):
    im = Image.open(io.BytesIO(stream))
    im.load()
    return im


def psnr_pair(frame, stream, quality, sub):
    """(the stream's decode, Pillow's own encode's decode) against the frame, both capped"""
    ours = psnr(np.asarray(decode(stream).convert("RGB")), frame)
    theirs = psnr(np.asarray(decode(pillow_jpeg(frame, quality, sub)).convert("RGB")), frame)
    return min(ours, PSNR_CAP), min(theirs, PSNR_CAP)


def tone(n, channels=1, seed=0):
    t = np.arange(n) / 8000.0
    a = 0.6 * np.sin(2 * np.pi * 440 * t + seed)
    return a if channels == 1 else np.stack([a, 0.5 * np.cos(2 * np.pi * 330 * t)], -1)


def check_avi(path, frames, width, height, rate, pcm=None, sr=None):
    """every claim of write_avi's docstring, walked back from the bytes"""
    with open(path, "rb") as f:
        buf = f.read()
    avi = walk_avi(buf)
    T = len(frames)
    assert avi["order"] == [b"hdrl", b"movi", b"idx1"] and len(buf) % 2 == 0
    usec, _, _, flags, total, _, n_streams, _, w, h = avi["avih"][:10]
    assert (usec, flags, total, w, h) == (int(round(1e6 / rate)), 0x110, T, width, height) and n_streams == len(avi["streams"]) == (1 if pcm is None else 2)
    vh, vf = avi["streams"][0]
    assert (vh["fccType"], vh["fccHandler"], vh["dwLength"]) == (b"vids", b"MJPG", T) and Fraction(vh["dwRate"], vh["dwScale"]) == rate
    assert len(vf) == 40 and struct.unpack("<IiiHH4sI", vf[:24]) == (40, width, height, 1, 24, b"MJPG", width * height * 3)
    video = [c for c in avi["movi"] if c[0] == b"00dc"]
    assert [c[3] for c in video] == [bytes(f) for f in frames]
    assert len(avi["idx1"]) == len(avi["movi"])
    for (fourcc, flags, offset, size), (tag, at, n, payload) in zip(avi["idx1"], avi["movi"]):
        assert (fourcc, offset, size) == (tag, at, n) and at % 2 == 0 and flags == (0x10 if tag == b"00dc" else 0)
        start = avi["movi_at"] + offset
        assert buf[start:start + 4] == tag and struct.unpack("<I", buf[start + 4:start + 8])[0] == size and buf[start + 8:start + 8 + size] == payload
    if pcm is None:
        assert all(c[0] == b"00dc" for c in avi["movi"])
        return avi
    ah, af = avi["streams"][1]
    channels = pcm.shape[1]
    keep = min(len(pcm), int(T * sr / rate))
    assert ah["fccType"] == b"auds" and Fraction(ah["dwRate"], ah["dwScale"]) == sr and ah["dwLength"] == keep and ah["dwSampleSize"] == 2 * channels
    assert struct.unpack("<HHIIHH", af) == (1, channels, sr, sr * 2 * channels, 2 * channels, 16)
    sound = np.frombuffer(b"".join(c[3] for c in avi["movi"] if c[0] == b"01wb"), "<i2").reshape(-1, channels)
    assert np.array_equal(sound, pcm[:keep])
    t = -1
    for tag, _, n, _ in avi["movi"]:                                       # a frame, then the samples of its own span
        if tag == b"00dc":
            t += 1
        else:
            assert n == 2 * channels * (min(int((t + 1) * sr / rate), len(pcm)) - min(int(t * sr / rate), len(pcm))) > 0
    return avi


def write_wav(path, samples, sr=8000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(sr)
        w.writeframes(np.rint(np.clip(samples, -1, 1) * 32767).astype(np.int16).astype("<i2").tobytes())
