"""From a WAV file to mono samples at 30720 Hz: the reference's ``librosa.load(wav_path, sr=30720)`` (data/data_preprocess/
dataset_utils.py:62) and the slicing of data/slice.py:10-26, with the decode, the downmix and the resampler on the device
(csrc/audio.hip; the definitions in include/tcdiff_hip.h).

    y = load_audio("song.wav", slices=(0.5, 5.0))          # (S, 153600): every 5-second window, resampled on its own
    cond = music.music_cond(y)                             # or music.wav_cond("song.wav", slices=(0.5, 5.0))

The parts, each callable alone:

    wav = read_wav(path_or_bytes)                          # host: the RIFF/WAVE container; sr, channels, frames, fmt, data
    y = decode([wav, ...], "cuda:0")                       # (B, frames) float32 mono at the file's rate: one launch
    rows = slice_audio(y[0], wav.sr, 0.5, 5.0)             # (S, window): an overlapping view, no copy
    z = resample(rows, wav.sr, 30720)                      # (S, size): resampy's kaiser_best resampler, one launch

The definitions restate soundfile, librosa 0.9.2 and resampy (its ``tr = t * inc`` form, resampy >= 0.3; 0.2.2 accumulates
``tr += inc``); none is a dependency and parity with their own output is not pinned.  Not built: containers other
than little-endian RIFF/WAVE, writing the slices back as files (``sf.write``), ``mono=False``."""
from __future__ import annotations

import math
import os
import struct
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import kernels as K

SR = 30720                                                # 60 frames per second x hop 512
ROLLOFF, BETA, N_ZEROS, PRECISION = 0.9475937167399596, 14.769656459379492, 64, L.AUDIO_PRECISION      # resampy's kaiser_best
N_TABLE = L.AUDIO_TABLE                                   # 32769 entries: m = 0 .. 512 * 64
MAX_DOWN = PRECISION // L.AUDIO_MIN_STEP                  # sr_orig / sr_new <= 8
_SAMPLE_BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}
_PCM = {8: "u8", 16: "s16", 24: "s24", 32: "s32"}
_FLOAT = {32: "f32", 64: "f64"}
_ROW_ALIGN = 16                                           # a file's bytes start on a 16-byte boundary of the upload

_TABLES = {}


class WavData(NamedTuple):
    """what ``read_wav`` returns: ``data`` holds the data chunk's bytes, ``frames`` whole frames of ``channels`` samples"""
    sr: int
    channels: int
    frames: int
    fmt: str
    data: bytes


def read_wav(path_or_bytes) -> WavData:
    """A little-endian RIFF/WAVE file, from a path or from its bytes -> WavData(sr, channels, frames, fmt, data).  Host only.

    ``fmt`` is "u8", "s16", "s24", "s32" (format tag 1, PCM), "f32" or "f64" (tag 3, IEEE float); tag 0xFFFE
    (WAVE_FORMAT_EXTENSIBLE) is resolved through its sub-format.  Unknown chunks are skipped, with the pad byte after an odd-sized
    one; a ``data`` size of 0 or 0xFFFFFFFF, or one that passes the end of the file, means "to the end of the file"; a truncated
    last frame is dropped.  Everything else raises a TcdiffError that names what was found."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        raw, name = bytes(path_or_bytes), "<bytes>"
    elif isinstance(path_or_bytes, (str, os.PathLike)):
        name = os.fspath(path_or_bytes)
        try:
            with open(path_or_bytes, "rb") as f:
                raw = f.read()
        except OSError as e:
            raise L.TcdiffError(f"read_wav: cannot read {name}: {e}") from None
    else:
        raise L.TcdiffError(f"read_wav: expected a path or bytes, got {type(path_or_bytes)}")
    if len(raw) < 12:
        raise L.TcdiffError(f"read_wav: {name}: {len(raw)} bytes are no RIFF/WAVE file")
    magic, form = raw[:4], raw[8:12]
    if magic != b"RIFF" or form != b"WAVE":
        what = {b"RF64": "an RF64 file", b"BW64": "a BW64 file", b"RIFX": "a big-endian RIFX file", b"FORM": "an AIFF / IFF file",
                b"fLaC": "a FLAC file", b"OggS": "an Ogg file"}.get(magic, f"magic {magic!r}, form {form!r}")
        raise L.TcdiffError(f"read_wav: {name}: not a little-endian RIFF/WAVE file ({what})")
    pos, spec = 12, None
    while pos + 8 <= len(raw):
        cid, size = struct.unpack_from("<4sI", raw, pos)
        pos += 8
        if cid == b"fmt ":
            if size < 16 or pos + 16 > len(raw):
                raise L.TcdiffError(f"read_wav: {name}: a fmt chunk of {size} bytes (at least 16)")
            tag, channels, sr, _, block_align, bits = struct.unpack_from("<HHIIHH", raw, pos)
            if tag == 0xFFFE:
                if size < 40 or pos + 40 > len(raw):
                    raise L.TcdiffError(f"read_wav: {name}: an extensible fmt chunk of {size} bytes (at least 40)")
                tag = struct.unpack_from("<H", raw, pos + 24)[0]
            kinds = _PCM if tag == 1 else _FLOAT if tag == 3 else None
            if kinds is None:
                raise L.TcdiffError(f"read_wav: {name}: format tag 0x{tag:04X} (only 1, PCM, and 3, IEEE float, are decoded)")
            if bits not in kinds:
                raise L.TcdiffError(f"read_wav: {name}: {bits} bits per sample with format tag {tag} (decoded: {sorted(kinds)})")
            if channels < 1 or sr < 1:
                raise L.TcdiffError(f"read_wav: {name}: {channels} channels at {sr} Hz")
            if block_align != channels * (bits // 8):
                raise L.TcdiffError(f"read_wav: {name}: block_align {block_align} with {channels} channels of {bits // 8} bytes")
            spec = (sr, channels, kinds[bits], block_align)
        elif cid == b"data":
            if spec is None:
                raise L.TcdiffError(f"read_wav: {name}: the data chunk comes before any fmt chunk")
            end = len(raw) if size in (0, 0xFFFFFFFF) else min(pos + size, len(raw))
            sr, channels, fmt, block_align = spec
            frames = (end - pos) // block_align
            return WavData(sr, channels, frames, fmt, raw[pos:pos + frames * block_align])
        pos += size + (size & 1)
    raise L.TcdiffError(f"read_wav: {name}: no {'data' if spec else 'fmt'} chunk")


def _wavs(name, files):
    """a WavData, a path, a file's bytes, or a list of them -> a list of WavData"""
    if isinstance(files, (WavData, str, os.PathLike, bytes, bytearray, memoryview)):
        files = [files]
    try:
        files = list(files)
    except TypeError:
        raise L.TcdiffError(f"{name}: expected a file or a list of files, got {type(files)}") from None
    if not files:
        raise L.TcdiffError(f"{name}: no file")
    return [f if isinstance(f, WavData) else read_wav(f) for f in files]


def _cuda(name, device):
    try:
        device = torch.device(device)
    except (RuntimeError, TypeError):
        raise L.TcdiffError(f"{name}: {device!r} is no device") from None
    if device.type != "cuda" or not torch.cuda.is_available():
        raise L.TcdiffError(f"{name} runs on MI355X only (no CPU fallback)")
    return device


def decode(wav_or_list, device="cuda:0") -> torch.Tensor:
    """WavData of ``read_wav``, or a list of them that agree in sr, channels, fmt and frames -> (B, frames) float32 on the device,
    mono at the file's rate: soundfile's conversion to float32 and librosa.to_mono's float32 mean over the channels, in one
    launch.  Only the data chunks' bytes are uploaded, as one uint8 tensor, each file's on a 16-byte boundary."""
    wavs = _wavs("decode", wav_or_list)
    first = wavs[0]
    for i, w in enumerate(wavs):
        if not isinstance(w.data, (bytes, bytearray)) or w.fmt not in _SAMPLE_BYTES or w.channels < 1 or \
                len(w.data) != w.frames * w.channels * _SAMPLE_BYTES[w.fmt]:
            raise L.TcdiffError(f"decode: file {i} holds {len(w.data)} bytes for {w.frames} frames of {w.channels} {w.fmt} samples")
        if (w.sr, w.channels, w.fmt, w.frames) != (first.sr, first.channels, first.fmt, first.frames):
            raise L.TcdiffError(f"decode: file {i} ({w.sr} Hz, {w.channels} channels, {w.fmt}, {w.frames} frames) differs from file 0 "
                                f"({first.sr} Hz, {first.channels} channels, {first.fmt}, {first.frames} frames)")
    if first.frames < 1:
        raise L.TcdiffError("decode: the files hold no frame")
    device = _cuda("decode", device)
    row = len(first.data)
    stride = -(-row // _ROW_ALIGN) * _ROW_ALIGN
    host = np.zeros((len(wavs), stride), np.uint8)
    for i, w in enumerate(wavs):
        host[i, :row] = np.frombuffer(w.data, np.uint8)
    with torch.cuda.device(device):
        data = torch.from_numpy(host).to(device)
        out = torch.empty(len(wavs), first.frames, dtype=torch.float32, device=device)
        K.audio_decode(data, first.frames, first.channels, first.fmt, out)
    return out


def resample_plan(n, sr_orig, sr_new=SR) -> dict:
    """the host's float64 side of ``resample`` (include/tcdiff_hip.h), Python's own expressions: ratio, n_out = int(n ratio),
    size = int(ceil(n ratio)), inc, scale and step = int(scale 512).  Raises where resampy does (n_out < 1) and where the ratio
    leaves the kernel's range (sr_orig / sr_new > 8)."""
    for what, v in (("sr_orig", sr_orig), ("sr_new", sr_new)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (v > 0 and math.isfinite(v)):
            raise L.TcdiffError(f"resample: {what} must be a positive number, got {v!r}")
    ratio = float(sr_new) / sr_orig
    n_out = int(n * ratio)
    if n_out < 1:
        raise L.TcdiffError(f"resample: {n} samples at {sr_orig} Hz are too short to be resampled to {sr_new} Hz")
    scale = min(1.0, ratio)
    step = int(scale * PRECISION)
    if step < L.AUDIO_MIN_STEP:
        raise L.TcdiffError(f"resample: {sr_orig} -> {sr_new} Hz is a ratio of {sr_orig / sr_new:.3f} to 1 (at most {MAX_DOWN})")
    return dict(ratio=ratio, n_out=n_out, size=int(math.ceil(n * ratio)), inc=1.0 / ratio, scale=scale, step=step)


def resample_table(ratio) -> np.ndarray:
    """(32769, 2) float64: win[m] = r sinc(r m / 512) kaiser(2 N + 1, beta)[N + m], N = 512 * 64, resampy's kaiser_best filter
    from its closed formula, times ``ratio`` when it is below 1, and delta[m] = win[m + 1] - win[m], delta[N] = 0"""
    n = N_TABLE - 1
    win = ROLLOFF * np.sinc(ROLLOFF * np.arange(N_TABLE) / PRECISION) * np.kaiser(2 * n + 1, BETA)[n:]
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    return np.stack([win, delta], 1)


def _table(sr_orig, sr_new, ratio, device):
    """rounded once to float32 and uploaded once per (sr_orig, sr_new, device)"""
    key = (float(sr_orig), float(sr_new), str(device))
    tab = _TABLES.get(key)
    if tab is None:
        tab = _TABLES[key] = torch.from_numpy(resample_table(ratio).astype(np.float32)).to(device)
    return tab


def resample(y, sr_orig, sr_new=SR) -> torch.Tensor:
    """y (n,) or (B, n) float32 on the device, samples at ``sr_orig`` Hz, read through its row stride (rows may overlap; only the
    last dimension must be contiguous) -> (B, size) float32 at ``sr_new`` Hz, size = ceil(n sr_new / sr_orig):
    ``librosa.resample(y, res_type="kaiser_best", fix=True, scale=False)``, in one launch.  ``sr_orig == sr_new`` returns ``y``
    itself, as librosa does.  Rates up to sr_orig / sr_new = 8; any ratio upwards."""
    if not isinstance(y, torch.Tensor) or y.dim() not in (1, 2):
        raise L.TcdiffError(f"resample: y must be (n,) or (B, n), got {tuple(y.shape) if isinstance(y, torch.Tensor) else type(y)}")
    if y.dtype != torch.float32:
        raise L.TcdiffError(f"resample: y must be float32, got {y.dtype}")
    rows = y if y.dim() == 2 else y[None]
    B, n = rows.shape
    plan = resample_plan(n, sr_orig, sr_new)
    if sr_orig == sr_new:
        return y
    if B < 1:
        raise L.TcdiffError("resample: y has no clip")
    if rows.stride(1) != 1:
        raise L.TcdiffError(f"resample: the last dimension of y must be contiguous (strides {tuple(y.stride())})")
    if B > 1 and rows.stride(0) < 0:
        raise L.TcdiffError(f"resample: the row stride of y must not be negative (strides {tuple(y.stride())})")
    if not y.is_cuda:
        raise L.TcdiffError("resample runs on MI355X only (no CPU fallback)")
    dev = y.device
    with torch.cuda.device(dev):
        table = _table(sr_orig, sr_new, plan["ratio"], dev)
        out = torch.empty(B, plan["size"], dtype=torch.float32, device=dev)
        K.audio_resample(rows, table, plan["inc"], plan["scale"], plan["step"], plan["n_out"], out)
    return out


def slice_starts(n, sr, stride=0.5, length=5.0):
    """(window, step, starts) of data/slice.py:16-23: window = int(length sr), step = int(stride sr), starts 0, step, ... while
    start <= n - window"""
    window, step = int(length * sr), int(stride * sr)
    if window < 1 or step < 1:
        raise L.TcdiffError(f"slice_audio: length {length!r} and stride {stride!r} at {sr!r} Hz give a window of {window} and a step "
                            f"of {step} samples")
    return window, step, range(0, n - window + 1, step)


def slice_audio(y, sr, stride=0.5, length=5.0) -> torch.Tensor:
    """y (n,) -> (S, window), the overlapping windows of data/slice.py as a view of ``y`` (no copy): window = int(length sr)
    samples every int(stride sr).  S is 0 where the signal is shorter than one window."""
    if not isinstance(y, torch.Tensor) or y.dim() != 1:
        raise L.TcdiffError(f"slice_audio: y must be (n,), got {tuple(y.shape) if isinstance(y, torch.Tensor) else type(y)}")
    window, step, starts = slice_starts(y.shape[0], sr, stride, length)
    return y.as_strided((len(starts), window), (step * y.stride(0), y.stride(0)))


def load_audio(files, *, sr=SR, slices=None, device="cuda:0") -> torch.Tensor:
    """A WAV file (a path, its bytes or a WavData) or a list of files that agree in rate, channels, format and length ->
    (B, size) float32 mono at ``sr`` Hz on the device: ``read_wav``, ``decode`` and ``resample``, two launches.
    ``slices=(stride, length)`` in seconds, with exactly one file, cuts it into the windows of ``slice_audio`` first, as the
    reference does, so the rows are the file's slices and each is resampled with its own edges."""
    wavs = _wavs("load_audio", files)
    if slices is not None:
        try:
            stride, length = slices
        except (TypeError, ValueError):
            raise L.TcdiffError(f"load_audio: slices must be (stride, length) in seconds, got {slices!r}") from None
        if len(wavs) != 1:
            raise L.TcdiffError(f"load_audio: slices are cut from exactly one file, got {len(wavs)}")
    y = decode(wavs, device)
    if slices is not None:
        y = slice_audio(y[0], wavs[0].sr, stride, length)
        if y.shape[0] < 1:
            raise L.TcdiffError(f"load_audio: {wavs[0].frames} frames at {wavs[0].sr} Hz are shorter than one slice of {length} s")
    return resample(y, wavs[0].sr, sr)
