"""CPU checks of the Motion-JPEG path (no GPU): the numpy restatement tests/mjpeg_ref.py of include/tcdiff_mjpeg.h against libjpeg
through Pillow (tables, decoding, quality), its DCT against the header's derived bound, the rare symbols of the shared frames, the
AVI container walked back, the refusals, the sixth header and its binding, and csrc/mjpeg_math.h built for the host as a
stand-alone program with the address and undefined-behaviour sanitizers against the restatement's bytes."""
import ctypes as C
import inspect
import os
import shutil
import struct
import subprocess
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest
import torch

import mjpeg_ref as R
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd import video as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcj_mjpeg_workspace", "tcj_mjpeg_plan", "tcj_mjpeg_write"]


# ---- tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 95, 100])
def test_quantisation_tables_equal_libjpeg_s(quality):
    frame = R.case("8x8")[0]
    theirs = R.decode(R.pillow_jpeg(frame, quality, "444")).quantization
    stream = R.encode(frame, quality, "444")
    assert R.decode(stream).quantization == theirs                          # the DQT bytes, read by the same reader
    dqt = [p for m, p in R.segments(stream) if m == 0xDB]
    assert len(dqt) == 1 and len(dqt[0]) == 130 and dqt[0][0] == 0 and dqt[0][65] == 1
    tables = V.jpeg_tables(quality)
    assert tables.shape == (2, 64) and tables.dtype == np.uint8 and np.array_equal(tables, R.quant_tables(quality))
    their_dqt = {p[0]: p[1:65] for m, p in R.segments(R.pillow_jpeg(frame, quality, "444")) if m == 0xDB for p in [p[i:i + 65] for i in range(0, len(p), 65)]}
    for c in range(2):
        assert bytes(tables[c][R.ZIGZAG].tolist()) == dqt[0][65 * c + 1:65 * c + 65] == their_dqt[c]
        natural = list(theirs[c]) if list(theirs[c]) == tables[c].tolist() else [theirs[c][i] for i in np.argsort(R.ZIGZAG)]
        assert natural == tables[c].tolist()


def test_huffman_tables_equal_libjpeg_s_byte_for_byte():
    frame = R.case("33x17")[0]
    for sub in R.SUBS:
        ours = [p for m, p in R.segments(R.encode(frame, 90, sub)) if m == 0xC4]
        theirs = [p for m, p in R.segments(R.pillow_jpeg(frame, 90, sub)) if m == 0xC4]
        assert len(ours) == 4 and [p[0] for p in ours] == [0x00, 0x10, 0x01, 0x11]
        assert sorted(ours) == sorted(theirs)
    for kind, chroma, n in (("dc", 0, 12), ("dc", 1, 12), ("ac", 0, 162), ("ac", 1, 162)):
        table = R.codes(kind, chroma)
        assert len(table) == n and max(length for _, length in table.values()) <= 16
        assert sum(2.0 ** -length for _, length in table.values()) < 1          # a prefix code with the all-ones code left free


# ---- DCT --------------------------------------------------------------------------------------------------------------------------------
def shared_blocks():
    blocks = [R.extreme_blocks().astype(np.int64) - 128]
    for name in R.CASES:
        for frame in R.case(name):
            for sub in R.SUBS:
                blocks += [R.blocks_of(p).reshape(-1, 8, 8) for p in R.planes(frame, sub)]
    return np.concatenate(blocks)


def test_the_integer_dct_stays_within_the_header_s_derived_bound():
    assert L.MJPEG.constants["TC_MJPEG_DCT_BOUND_MILLI"] == 1000 * R.DCT_BOUND and L.MJPEG.constants["TC_MJPEG_COEF_BITS"] == R.COEF_BITS
    assert L.MJPEG.constants["TC_MJPEG_DCT_BITS"] == R.DCT_BITS
    with open(_abi.HEADER_MJPEG) as f:
        text = f.read()
    for k, row in enumerate(R.M.tolist()):                                 # the matrix the header prints is the formula's
        assert f"row {k}:" + "".join(f"{v:7d}" for v in row) in text, k
    s = shared_blocks()
    err = np.abs(R.dct_int(s) / 2.0 ** R.COEF_BITS - R.dct_float(s)).max()
    print(f"[mjpeg] integer DCT against float64 over {len(s)} blocks: {err:.4f} of one coefficient (bound {R.DCT_BOUND})")
    assert err <= R.DCT_BOUND
    ext = R.dct_float(R.extreme_blocks().astype(np.int64) - 128).reshape(64, 64)
    assert abs(abs(ext[4, 4]) - 1020) < 1e-9 and abs(ext[0, 0] - 1016) < 1e-9          # block 4 is (v, u) = (0, 4): the AC value that reaches 1020


def test_the_clamp_keeps_every_category_in_the_standard_tables():
    data, offsets, stats = R.expected("extreme", 100, "444")
    coef = R.coefficients(R.case("extreme")[0], 100, "444")[0]
    assert np.abs(coef[..., 1:]).max() <= 1023 and np.abs(coef[..., 1:]).max() >= 1016
    ones = R.quantise(R.dct_int(R.extreme_blocks().astype(np.int64) - 128) * 2, np.ones(64, np.int64))          # what a wilder input would give
    assert np.abs(ones[..., 1:]).max() == 1023
    im = R.decode(data)
    assert im.size == (64, 64) and R.psnr(np.asarray(im.convert("RGB")), R.case("extreme")[0]) > 45


# ---- decoding and quality -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", R.SUBS)
@pytest.mark.parametrize("name", ["33x17", "16x80", "8x8"])
def test_pillow_decodes_every_restated_stream_to_the_right_size(name, sub):
    frames = R.case(name)
    for quality in R.QUALITIES:
        data, offsets, _ = R.expected(name, quality, sub)
        for i, frame in enumerate(frames):
            stream = data[offsets[i]:offsets[i + 1]]
            im = R.decode(stream)
            assert im.size == (frame.shape[1], frame.shape[0]) and im.mode == "RGB" and im.format == "JPEG"
            assert stream[:2] == b"\xff\xd8" and stream[-2:] == b"\xff\xd9" and len(stream) > R.HEADER_BYTES
            sof = [p for m, p in R.segments(stream) if m == 0xC0][0]
            assert struct.unpack(">BHHB", sof[:6]) == (8, frame.shape[0], frame.shape[1], 3)
            assert sof[7] == (0x22 if sub == "420" else 0x11) and sof[10] == sof[13] == 0x11
            dri = [p for m, p in R.segments(stream) if m == 0xDD][0]
            assert struct.unpack(">H", dri)[0] == -(-frame.shape[1] // (16 if sub == "420" else 8))


def test_the_decode_is_as_close_to_the_source_as_libjpeg_s_own_encode():
    worst = 0.0
    for name in ("33x17", "16x80", "checker", "seven", "extreme"):
        for quality in R.QUALITIES:
            for sub in R.SUBS:
                data, offsets = R.encode_all(R.case(name), quality, sub)
                for i, frame in enumerate(R.case(name)):
                    ours, theirs = R.psnr_pair(frame, data[offsets[i]:offsets[i + 1]], quality, sub)
                    worst = max(worst, theirs - ours)
                    assert ours >= theirs - R.PSNR_MARGIN, (name, quality, sub, i, ours, theirs)
    print(f"[mjpeg] the largest PSNR gap to Pillow's own encoder: {worst:.3f} dB (margin {R.PSNR_MARGIN:.2f})")


def test_grey_frames_have_neutral_chroma_exactly():
    v = np.arange(256, dtype=np.uint8)
    y, cb, cr = R.ycc(np.stack([v, v, v], -1))
    assert np.array_equal(y, v) and (cb == 128).all() and (cr == 128).all()
    grey = np.repeat(np.random.default_rng(3).integers(0, 256, (19, 21, 1), dtype=np.uint8), 3, -1)
    for sub in R.SUBS:
        _, cbq, crq = R.coefficients(grey, 90, sub)
        assert not cbq.any() and not crq.any()
        dec = np.asarray(R.decode(R.encode(grey, 90, sub)).convert("YCbCr"))
        assert (dec[..., 1:] == 128).all()


def test_the_shared_frames_hold_every_rare_symbol():
    total = Counter()
    for name in R.CASES:
        for quality in R.QUALITIES:
            for sub in R.SUBS:
                total.update(R.expected(name, quality, sub)[2])
    print("[mjpeg] the shared set's symbols:", sorted(total.items()))
    for key in ["zrl", "no-eob", "stuffed", "dc-category-0", "dc-category-11", "rst-wrap"] + [f"rst{m}" for m in range(8)]:
        assert total[key] >= 1, key
    assert R.expected("16x80", 90, "444")[2]["rst0"] == 2                  # ten MCU rows: RST0 .. RST7, then RST0 again


# ---- the container -------------------------------------------------------------------------------------------------------------------------
def test_write_avi_walked_back(tmp_path):
    frames = [R.encode(f, 90, "420") for f in R.case("33x17")] + [b"\xff\xd8odd\xff\xd9"]          # an odd-sized chunk is padded
    sr = 8000
    long_audio = R.tone(sr)                                                  # a second of sound on 4 frames: cut at T / fps
    pcm = V.pcm16(long_audio).reshape(-1, 1)
    p = V.write_avi(tmp_path / "a.avi", frames, fps=30, audio=long_audio, sample_rate=sr, width=33, height=17)
    assert p == str(tmp_path / "a.avi")
    avi = R.check_avi(p, frames, 33, 17, Fraction(30), pcm, sr)
    assert [c[0] for c in avi["movi"]] == [b"00dc", b"01wb"] * 4 and avi["streams"][1][0]["dwLength"] == 4 * sr // 30
    R.check_avi(V.write_avi(tmp_path / "b.avi", frames, fps=29.97, audio=long_audio, sample_rate=sr, width=33, height=17), frames, 33, 17,
              Fraction(2997, 100), pcm, sr)
    R.check_avi(V.write_avi(tmp_path / "c.avi", frames, fps=Fraction(30000, 1001), width=33, height=17), frames, 33, 17, Fraction(30000, 1001))
    stereo = R.tone(150, 2)                                                  # shorter than the video: kept as it is
    avi = R.check_avi(V.write_avi(tmp_path / "d.avi", frames, fps=25, audio=torch.from_numpy(stereo), sample_rate=sr, width=33, height=17),
                    frames, 33, 17, Fraction(25), V.pcm16(stereo), sr)
    assert avi["streams"][1][0]["dwLength"] == 150 and [c[0] for c in avi["movi"]][-3:] == [b"00dc", b"00dc", b"00dc"]
    host = V.JpegFrames(torch.frombuffer(bytearray(b"".join(frames[:3])), dtype=torch.uint8),
                        torch.tensor(np.cumsum([0] + [len(f) for f in frames[:3]])), 33, 17)
    assert len(host) == 3 and host.cpu() is host and host.frames() == frames[:3] and host.frame(-1) == frames[2]
    R.check_avi(V.write_avi(tmp_path / "e.avi", host, fps=30), frames[:3], 33, 17, Fraction(30))


def test_pcm16_rounds_to_even_and_clips():
    x = np.array([0.0, 1.0, -1.0, 2.0, -3.0, 0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767, 0.25])
    want = [0, 32767, -32767, 32767, -32767, 0, 2, 2, 0, 8192]
    assert V.pcm16(x).tolist() == want and V.pcm16(x).dtype == np.int16
    assert V.pcm16(torch.from_numpy(x).float()[:5]).tolist() == want[:5] and V.pcm16(np.stack([x, x], -1)).shape == (10, 2)
    i16 = np.array([-32768, 5, 32767], np.int16)
    assert np.array_equal(V.pcm16(i16), i16) and np.array_equal(V.pcm16(torch.from_numpy(i16)), i16)
    for bad in (np.zeros((2, 2, 2)), np.array([1, 2]), np.array([0.0, np.nan]), np.zeros((3, 0))):
        with pytest.raises(L.TcdiffError, match="pcm16"):
            V.pcm16(bad)


def test_refusals(tmp_path, monkeypatch):
    import tcdiff_amd
    for name in ("JpegFrames", "encode_jpeg", "jpeg_tables", "pcm16", "write_avi", "clip_audio"):
        assert getattr(tcdiff_amd, name) is getattr(V, name)
    good = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        V.encode_jpeg(good)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        V.encode_jpeg(good[None])
    for bad, what in ((good.float(), "uint8"), (good[0], "must be"), (torch.zeros(2, 8, 8, 4, dtype=torch.uint8), "must be"), (good.numpy(), "must be"),
                      (torch.zeros(2, 0, 8, 3, dtype=torch.uint8), "empty"), (torch.zeros(2, 3, 8, 8, dtype=torch.uint8).permute(0, 2, 3, 1), "contiguous")):
        with pytest.raises(L.TcdiffError, match=what):
            V.encode_jpeg(bad)
    for q in (0, 101, 90.0, True, None):
        with pytest.raises(L.TcdiffError, match="quality"):
            V.encode_jpeg(good, quality=q)
        with pytest.raises(L.TcdiffError, match="quality"):
            V.jpeg_tables(q)
    for s in ("422", 420, None):
        with pytest.raises(L.TcdiffError, match="subsampling"):
            V.encode_jpeg(good, subsampling=s)
    frames = [R.encode(R.case("8x8")[0])]
    out = tmp_path / "x.avi"
    for kw, what in ((dict(), "width"), (dict(width=8, height=0), "width"), (dict(width=8, height=8, fps=0), "fps"), (dict(width=8, height=8, fps="x"), "fps"),
                     (dict(width=8, height=8, fps=float("nan")), "fps"), (dict(width=8, height=8, audio=R.tone(10)), "sample_rate"),
                     (dict(width=8, height=8, sample_rate=8000), "sample_rate"), (dict(width=8, height=8, audio=R.tone(10), sample_rate=0), "sample_rate")):
        with pytest.raises(L.TcdiffError, match=what):
            V.write_avi(out, frames, **kw)
    for bad in ([], ["text"], 5):
        with pytest.raises(L.TcdiffError, match="write_avi"):
            V.write_avi(out, bad, width=8, height=8)
    assert not out.exists()
    size = os.path.getsize(V.write_avi(out, frames, width=8, height=8))
    assert V.MAX_AVI_BYTES == 2 ** 31 - 1
    monkeypatch.setattr(V, "MAX_AVI_BYTES", size - 1)                      # the 2 GiB limit, through a stubbed size
    os.remove(out)
    with pytest.raises(L.TcdiffError, match="OpenDML"):
        V.write_avi(out, frames, width=8, height=8)
    assert not out.exists()
    monkeypatch.setattr(V, "MAX_AVI_BYTES", size)
    assert os.path.getsize(V.write_avi(out, frames, width=8, height=8)) == size


def test_clip_audio_finds_the_files_the_reference_would(tmp_path):
    """the lookup; the R.decode and the stitch run on the device (tests/test_mjpeg_gpu.py), for audio.decode has no CPU path"""
    other = tmp_path / "elsewhere"
    other.mkdir()
    names = [str(tmp_path / f"song_slice{k}.npy") for k in range(3)]
    for k in range(3):
        R.write_wav(tmp_path / f"song_slice{k}.wav", R.tone(40, seed=k))
        R.write_wav(other / f"song_slice{k}.wav", R.tone(40, seed=k))
    wavs = [str(tmp_path / f"song_slice{k}.wav") for k in range(3)]
    assert V.clip_audio_paths(names, "normal") == [[w] for w in wavs] and V.clip_audio_paths(names, "long") == [wavs]
    moved = ["/nowhere/" + os.path.basename(n) for n in names]
    assert V.clip_audio_paths(moved, "long", folder=other) == [[str(other / os.path.basename(w)) for w in wavs]]
    os.remove(wavs[1])
    for mode in ("normal", "long"):
        with pytest.raises(L.TcdiffError, match="song_slice1.wav does not exist"):
            V.clip_audio_paths(names, mode)
        with pytest.raises(L.TcdiffError, match="song_slice1.wav does not exist"):
            V.clip_audio(names, mode)                                      # before anything touches a device
    for bad in (None, [], "name.wav"):
        with pytest.raises(L.TcdiffError, match="names"):
            V.clip_audio_paths(bad, "normal")


# ---- the sixth header ------------------------------------------------------------------------------------------------------------------
def test_the_sixth_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_mjpeg()
    assert list(abi.functions) == NAMES and L.MJPEG.functions == abi.functions and L.MJPEG.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_MJPEG_444=0, TC_MJPEG_420=1, TC_MJPEG_THREADS=256, TC_MJPEG_WINDOW=8192, TC_MJPEG_LAUNCHES=4,
                                 TC_MJPEG_HEADER_BYTES=625, TC_MJPEG_MAX_SIDE=65535, TC_MJPEG_DCT_BITS=14, TC_MJPEG_COEF_BITS=20,
                                 TC_MJPEG_DCT_BOUND_MILLI=200)
    assert abi.constants["TC_MJPEG_LAUNCHES"] <= 5 and V.THREADS == 256 and R.HEADER_BYTES == 625
    I, VP, LONG = C.c_int, C.c_void_p, C.c_long
    assert abi.functions["tcj_mjpeg_plan"][:2] == (I, [VP, VP, I, I, I, I, I, VP, LONG, VP, VP])
    assert abi.functions["tcj_mjpeg_write"][:2] == (I, [I, I, I, I, I, VP, LONG, VP, LONG, VP])
    with open(_abi.HEADER_MJPEG) as f:
        text = f.read()
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_mjpeg.h", prefix=prefix)
    for names in (L.ABI.functions, L.EXT.functions, L.GLTF.functions, L.SKIN.functions, L.SHADE.functions, L.EXPORTS):
        assert not any(n.startswith("tcj_") for n in names)
    frozen = {**L.ABI.constants, **L.EXT.constants, **L.GLTF.constants, **L.SKIN.constants, **L.SHADE.constants}
    assert not any(k.startswith("TC_MJPEG") for k in frozen) and len(L.ABI.functions) == 79


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    syms = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    assert sorted(s for s in syms if s.startswith("tcj_")) == sorted(NAMES)
    assert not [s for s in syms if "mjpeg" in s.lower() and s.split("_")[0] in ("tcdiff", "tcx", "tcs", "tcr")]
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    strides = (C.c_long * 3)(3 * 8 * 8, 3 * 8, 3)
    n = C.c_long(-1)
    assert lib.tcj_mjpeg_workspace(2, 17, 33, 1, C.addressof(n)) == 0 and n.value == 16 * 2 * 2 + 132 * 2 * 2 * 3 * 6
    assert lib.tcj_mjpeg_workspace(2, 17, 33, 0, C.addressof(n)) == 0 and n.value == 16 * 2 * 3 + 132 * 2 * 3 * 5 * 3
    assert lib.tcj_mjpeg_workspace(1, 8, 8, 0, None) == -1 and lib.tcj_mjpeg_workspace(1, 8, 8, 2, C.addressof(n)) == -1
    assert lib.tcj_mjpeg_workspace(1, 65536, 8, 0, C.addressof(n)) == -4 and lib.tcj_mjpeg_workspace(2 ** 31 - 1, 65535, 65535, 0, C.addressof(n)) == -4

    def plan(frames=p, strides=strides, N=1, H=8, W=8, quality=90, sub=0, ws=p, ws_bytes=16 + 132 * 3 - 1, offsets=p):
        return lib.tcj_mjpeg_plan(frames, strides, N, H, W, quality, sub, ws, ws_bytes, offsets, None)
    assert plan() == -1                                                    # good arguments but for one byte of workspace
    assert plan(ws=p + 4, ws_bytes=16 + 132 * 3) == -2
    for kw in (dict(frames=None), dict(strides=None), dict(ws=None), dict(offsets=None), dict(N=0), dict(H=0), dict(W=-1), dict(quality=0),
               dict(quality=101), dict(sub=2), dict(sub=-1), dict(strides=(C.c_long * 3)(192, -24, 3))):
        assert plan(ws_bytes=1 << 40, **kw) == -1, kw
    assert plan(W=65536, ws_bytes=1 << 40) == -4 and plan(N=2 ** 31 - 1, H=65535, W=65535, ws_bytes=1 << 40) == -4

    def write(N=1, H=8, W=8, quality=90, sub=0, ws=p, ws_bytes=16 + 132 * 3 - 1, data=p, data_bytes=1000):
        return lib.tcj_mjpeg_write(N, H, W, quality, sub, ws, ws_bytes, data, data_bytes, None)
    assert write() == -1 and write(ws=p + 4, ws_bytes=16 + 132 * 3) == -2 and write(ws_bytes=1 << 40, data_bytes=-1) == -1
    for kw in (dict(ws=None), dict(data=None), dict(N=0), dict(H=0), dict(W=0), dict(quality=0), dict(sub=3)):
        assert write(ws_bytes=1 << 40, **kw) == -1, kw
    assert write(H=65536, ws_bytes=1 << 40) == -4


def test_the_sixth_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.MJPEG.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_mjpeg.h"', '#include "tcdiff_mjpeg.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "mjpeg.c", tmp_path / "mjpeg"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.MJPEG.constants[n] for n in names]
    calls = ['#include "tcdiff_mjpeg.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.MJPEG.functions.items():
        assert restype is C.c_int and argtypes == [C.c_void_p if c.endswith("*") else _abi.SCALARS[c] for c in ctexts], fname
        calls.append(f"  {{ int (*f)({', '.join(ctexts)}) = {fname}; (void)f; }}")
        zeros = [f"({c})0" if c.endswith("*") or c == "hipStream_t" else f"({c})z" for c in ctexts]
        calls.append(f"  (void){fname}({', '.join(zeros)});")
    calls.append("}")
    tu = tmp_path / "calls.c"
    tu.write_text("\n".join(calls))
    r = subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-c", str(tu), "-o", str(tmp_path / "calls.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_defaults_leave_the_png_path_as_it_was():
    from tcdiff_amd import GaussianDiffusion
    from tcdiff_amd.draw import write_draw_out
    assert GaussianDiffusion.draw_format == "png" and GaussianDiffusion.draw_audio_folder is None
    params = list(inspect.signature(GaussianDiffusion.render_sample).parameters)
    assert params == ["self", "shape", "cond", "normalizer", "epoch", "render_out", "fk_out", "name", "sound", "mode", "noise", "constraint",
                      "sound_folder", "start_point", "render", "required_dancer_num", "x_0", "render_len", "glb_out", "draw_out"]
    sig = inspect.signature(write_draw_out).parameters
    assert sig["format"].default == "png" and sig["quality"].default == 90 and sig["subsampling"].default == "420" and sig["audio"].default is None
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("format", "quality", "subsampling", "audio"))
    poses = torch.zeros(1, 1, 2, 24, 3)
    with pytest.raises(L.TcdiffError, match="format"):
        write_draw_out("unused", "normal", 0, ["a.wav"], poses, None, format="gif")
    with pytest.raises(L.TcdiffError, match="no audio"):
        write_draw_out("unused", "normal", 0, ["a.wav"], poses, None, audio=[(R.tone(4), 8000)])
    assert not os.path.exists("unused")


# ---- csrc/mjpeg_math.h on the host, under the sanitizers ---------------------------------------------------------------------------------
def test_mjpeg_math_on_the_host_under_the_sanitizers_gives_the_restatement_s_bytes(tmp_path):
    """the SAME arithmetic the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "mjpeg_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "mjpeg_host.cpp")])
    for name in R.CASES:
        frames = R.case(name)
        for quality in R.QUALITIES:
            for sub in R.SUBS:
                data, offsets, _ = R.expected(name, quality, sub)
                with open(tmp_path / "in.bin", "wb") as f:
                    f.write(np.array([*frames.shape[:3], quality, V.SUBSAMPLING[sub]], np.int32).tobytes() + frames.tobytes())
                r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
                assert r.returncode == 0, (name, quality, sub, r.returncode, r.stderr)
                raw = (tmp_path / "out.bin").read_bytes()
                n = 8 * (len(frames) + 1)
                assert np.array_equal(np.frombuffer(raw[:n], np.int64), offsets) and raw[n:] == data, (name, quality, sub)
