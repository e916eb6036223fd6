"""The drawn clip as a video with its music: a baseline JPEG encoder on the device (``tcj_mjpeg_plan`` + ``tcj_mjpeg_write``,
csrc/mjpeg.hip; the bytes are defined in include/tcdiff_mjpeg.h) on the frames where ``draw_dance`` left them, and a Motion-JPEG
AVI 1.0 container with a 16-bit PCM audio stream, packed on the host with ``struct`` alone.  Only compressed bytes cross to the
host.  The counterpart of the reference's ``skeleton_render`` with ``sound`` (vis.py:292-320: a GIF, the clip's .wav, ffmpeg).

    frames = draw_dance(poses, contacts)                                         # (b, T, 480, 480, 3) uint8, on the device
    jpeg = encode_jpeg(frames[0], quality=90)                                    # JpegFrames: data + offsets, on the device
    samples, sr = clip_audio(["clip0.wav"], "normal")[0]
    write_avi("clip0.avi", jpeg, fps=30, audio=samples, sample_rate=sr)

mpv, VLC, ffmpeg and Windows play Motion-JPEG in AVI as it is; parity with them is unpinned (none is installed): the JPEG frames
are held to libjpeg through Pillow by the tests.  Not built: OpenDML (files above 2 GiB), compressed audio, resampling, MP4.
"""
from __future__ import annotations

import os
import struct
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L
from . import kernels as K

THREADS = L.MJPEG.constants["TC_MJPEG_THREADS"]
MAX_SIDE = L.MJPEG.constants["TC_MJPEG_MAX_SIDE"]
SUBSAMPLING = {"444": L.MJPEG.constants["TC_MJPEG_444"], "420": L.MJPEG.constants["TC_MJPEG_420"]}
MAX_AVI_BYTES = 2 ** 31 - 1          # AVI 1.0: one RIFF chunk
_AVIF_HASINDEX, _AVIF_ISINTERLEAVED, _AVIIF_KEYFRAME = 0x10, 0x100, 0x10

# Annex K.1 / K.2, natural order (csrc/mjpeg_math.h TCJ_BASE)
_BASE = np.array([[16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                   100, 103, 99],
                  [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66] + [99] * 38])


def _quality(quality) -> int:
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise L.TcdiffError(f"encode_jpeg: quality must be an integer in 1..100, got {quality!r}")
    return int(quality)


def _subsampling(subsampling) -> int:
    if subsampling not in SUBSAMPLING:
        raise L.TcdiffError(f'encode_jpeg: subsampling must be "420" or "444", got {subsampling!r}')
    return SUBSAMPLING[subsampling]


def jpeg_tables(quality) -> np.ndarray:
    """The two quantisation tables ``encode_jpeg`` uses at ``quality``, (2, 64) uint8 in natural (row-major) order, luminance then
    chrominance: Annex K's tables scaled by the IJG rule (include/tcdiff_mjpeg.h)."""
    q = _quality(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((_BASE * scale + 50) // 100, 1, 255).astype(np.uint8)


class JpegFrames:
    """N JPEG streams back to back: ``data`` uint8, ``offsets`` int64 (N + 1,) -- frame i is data[offsets[i]:offsets[i + 1]] --
    both on one side, and the frames' ``width`` and ``height``."""

    def __init__(self, data, offsets, width, height):
        self.data, self.offsets, self.width, self.height = data, offsets, int(width), int(height)
        self._host = self._bytes = None          # the host copy of device frames; the host data as numpy and the offsets as a list

    def __len__(self):
        return self.offsets.numel() - 1

    @property
    def is_cuda(self):
        return self.data.is_cuda

    def cpu(self) -> "JpegFrames":
        """the same frames on the host: one copy of the data, one of the offsets"""
        if not self.is_cuda:
            return self
        if self._host is None:
            self._host = JpegFrames(self.data.cpu(), self.offsets.cpu(), self.width, self.height)
        return self._host

    def frame(self, i) -> bytes:
        host = self.cpu()
        n = len(host)
        if not -n <= i < n:
            raise L.TcdiffError(f"JpegFrames.frame: {i} of {n} frames")
        i %= n
        if host._bytes is None:
            host._bytes = (host.data.numpy(), host.offsets.tolist())
        data, offsets = host._bytes
        return data[offsets[i]:offsets[i + 1]].tobytes()

    def frames(self) -> list:
        return [self.frame(i) for i in range(len(self))]


def _encode(frames, quality, sub) -> tuple:
    N, H, W, _ = frames.shape
    dev = frames.device
    workspace = torch.empty(K.mjpeg_workspace(N, H, W, sub), dtype=torch.uint8, device=dev)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=dev)
    K.mjpeg_plan(frames, quality, sub, workspace, offsets)
    data = torch.empty(int(offsets[N].item()), dtype=torch.uint8, device=dev)          # the one scalar that crosses to the host
    K.mjpeg_write(N, H, W, quality, sub, workspace, data)
    return data, offsets


def encode_jpeg(frames, quality=90, subsampling="420") -> JpegFrames:
    """frames (N, H, W, 3) or (b, T, H, W, 3) uint8 RGB on the device, read in place through its strides (only the trailing 3 must
    be contiguous: a view or a crop of ``draw_dance``'s frames is encoded where it lies) -> JpegFrames on the device, N (b T)
    baseline JFIF streams, clip after clip.  ``quality`` 1..100 scales Annex K's tables by the IJG rule; ``subsampling`` "420"
    or "444".  Every frame is a complete JPEG file: standard Huffman tables, one restart interval per MCU row.  The bytes are
    defined in include/tcdiff_mjpeg.h and are the same for the same input.  A (b, T, ...) batch whose two leading dimensions do
    not share one stride is encoded clip by clip."""
    q, sub = _quality(quality), _subsampling(subsampling)
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (4, 5) or frames.shape[-1] != 3:
        got = tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames)
        raise L.TcdiffError(f"encode_jpeg: frames must be (N, H, W, 3) or (b, T, H, W, 3), got {got}")
    if frames.dtype != torch.uint8:
        raise L.TcdiffError(f"encode_jpeg: frames must be uint8, got {frames.dtype}")
    if min(frames.shape) < 1 or max(frames.shape[-3:-1]) > MAX_SIDE:
        raise L.TcdiffError(f"encode_jpeg: frames {tuple(frames.shape)} has an empty dimension or a side above {MAX_SIDE}")
    if frames.stride(-1) != 1:
        raise L.TcdiffError(f"encode_jpeg: the trailing dimension of frames must be contiguous (strides {tuple(frames.stride())})")
    if not frames.is_cuda:
        raise L.TcdiffError("encode_jpeg runs on MI355X only (no CPU fallback)")
    H, W = frames.shape[-3:-1]
    with torch.cuda.device(frames.device):
        if frames.dim() == 5:
            b, T = frames.shape[:2]
            if b == 1 or T == 1 or frames.stride(0) == T * frames.stride(1):
                frames = frames.as_strided((b * T, H, W, 3), (frames.stride(1) if T > 1 else frames.stride(0),) + tuple(frames.stride()[2:]),
                                           frames.storage_offset())
            else:
                parts, base = [_encode(clip, q, sub) for clip in frames], 0
                offsets = []
                for data, off in parts:
                    offsets.append(off[:-1] + base)
                    base = base + off[-1]
                return JpegFrames(torch.cat([d for d, _ in parts]), torch.cat(offsets + [base.reshape(1)]), W, H)
        data, offsets = _encode(frames, q, sub)
    return JpegFrames(data, offsets, W, H)


def pcm16(audio) -> np.ndarray:
    """float samples in [-1, 1], (n,) or (n, channels), a tensor or an array on either side -> host int16 of the same shape,
    round(clip(x, -1, 1) * 32767), halves to even; int16 is passed through."""
    if isinstance(audio, torch.Tensor):
        audio = audio.detach().cpu().numpy()
    a = np.asarray(audio)
    if a.ndim not in (1, 2) or (a.ndim == 2 and not 1 <= a.shape[1] <= 65535):
        raise L.TcdiffError(f"pcm16: audio must be (n,) or (n, channels), got {a.shape}")
    if a.dtype == np.int16:
        return np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        raise L.TcdiffError(f"pcm16: audio must be float in [-1, 1] or int16, got {a.dtype}")
    if not np.isfinite(a).all():
        raise L.TcdiffError("pcm16: audio holds values that are not finite")
    return np.rint(np.clip(a.astype(np.float64), -1.0, 1.0) * 32767.0).astype(np.int16)


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _rate(fps) -> Fraction:
    try:
        rate = Fraction(str(fps)) if isinstance(fps, float) else Fraction(fps)
    except (ValueError, TypeError, ZeroDivisionError):
        rate = None
    if rate is None or rate <= 0 or rate.numerator >= 2 ** 32 or rate.denominator >= 2 ** 32:
        raise L.TcdiffError(f"write_avi: fps must be a positive rate that two 32-bit integers can hold, got {fps!r}")
    return rate


def write_avi(path, jpeg, fps=30, audio=None, sample_rate=None, *, width=None, height=None) -> str:
    """An AVI 1.0 file at ``path``: ``RIFF 'AVI '``; ``LIST hdrl`` with ``avih`` and one ``strl`` (``strh`` + ``strf``) per stream
    -- the video ``vids`` / ``MJPG`` with dwRate / dwScale = Fraction(fps) (a float goes through its decimal form: 29.97 is
    2997 / 100) and a 40-byte BITMAPINFOHEADER, the audio ``auds`` with a 16-byte PCM WAVEFORMAT, 16 bit; ``LIST movi`` with one
    ``00dc`` chunk per frame, each followed, with audio, by a ``01wb`` chunk of the samples floor(t sr / fps) .. floor((t + 1) sr /
    fps) (none when the audio has run out), chunks padded to even size; ``idx1`` with one entry per chunk, offsets from the
    ``movi`` fourcc, the key-frame flag on every video chunk.

    ``jpeg``: JpegFrames on either side, or a list of ``bytes`` with ``width=`` and ``height=``.  ``audio``: what ``pcm16`` takes,
    with its ``sample_rate`` in Hz; audio longer than T / fps seconds is cut there (ffmpeg's -shortest, vis.py:320), shorter audio
    is kept as it is.  A file that would pass 2^31 - 1 bytes is refused: OpenDML is not built.  ``struct`` only."""
    if isinstance(jpeg, JpegFrames):
        frames, width, height = jpeg.frames(), jpeg.width, jpeg.height
    else:
        try:
            frames = list(jpeg)
        except TypeError:
            raise L.TcdiffError(f"write_avi: jpeg must be JpegFrames or a list of bytes, got {type(jpeg)}") from None
        if any(not isinstance(f, (bytes, bytearray)) for f in frames):
            raise L.TcdiffError("write_avi: a list of frames must hold bytes")
        if width is None or height is None:
            raise L.TcdiffError("write_avi: a list of bytes needs width= and height=")
    if not frames:
        raise L.TcdiffError("write_avi: no frame")
    width, height = int(width), int(height)
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise L.TcdiffError(f"write_avi: width and height must be in 1..{MAX_SIDE}, got {width}, {height}")
    rate, T = _rate(fps), len(frames)
    pcm = None
    if audio is not None:
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or not 1 <= sample_rate < 2 ** 31:
            raise L.TcdiffError(f"write_avi: audio needs its sample_rate, a positive integer, got {sample_rate!r}")
        pcm = pcm16(audio)
        pcm = pcm.reshape(len(pcm), -1)
        sr, channels = int(sample_rate), pcm.shape[1]
        bounds = [min(int(t * sr / rate), len(pcm)) for t in range(T + 1)]          # Fraction arithmetic: exact floors
        pcm = pcm[:bounds[T]]
    elif sample_rate is not None:
        raise L.TcdiffError("write_avi: a sample_rate without audio")

    movi, index, pos, biggest = [b"movi"], [], 4, [0, 0]
    for t, frame in enumerate(frames):
        chunks = [(b"00dc", bytes(frame), _AVIIF_KEYFRAME, 0)]
        if pcm is not None and bounds[t + 1] > bounds[t]:
            chunks.append((b"01wb", pcm[bounds[t]:bounds[t + 1]].astype("<i2").tobytes(), 0, 1))
        for fourcc, payload, flags, stream in chunks:
            index.append(struct.pack("<4sIII", fourcc, flags, pos, len(payload)))
            packed = _chunk(fourcc, payload)
            movi.append(packed)
            pos += len(packed)
            biggest[stream] = max(biggest[stream], len(payload))
    usec = int(round(1_000_000 / rate))
    n_streams = 1 if pcm is None else 2
    per_second = int(sum(len(f) for f in frames) * rate / T) + (0 if pcm is None else sr * 2 * channels)
    avih = struct.pack("<14I", usec, min(per_second, 2 ** 32 - 1), 0, _AVIF_HASINDEX | _AVIF_ISINTERLEAVED, T, 0, n_streams, max(biggest),
                       width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, rate.denominator, rate.numerator, 0, T, biggest[0], 0xFFFFFFFF, 0,
                       0, 0, min(width, 32767), min(height, 32767))
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf))
    if pcm is not None:
        align = 2 * channels
        strh = struct.pack("<4s4sIHHIIIIIIII4h", b"auds", b"\0\0\0\0", 0, 0, 0, 0, align, sr * align, 0, len(pcm), biggest[1], 0xFFFFFFFF,
                           align, 0, 0, 0, 0)
        strf = struct.pack("<HHIIHH", 1, channels, sr, sr * align, align, 16)
        hdrl += _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf))
    body = [b"AVI ", _chunk(b"LIST", hdrl), _chunk(b"LIST", b"".join(movi)), _chunk(b"idx1", b"".join(index))]
    size = sum(len(p) for p in body)
    if size + 8 > MAX_AVI_BYTES:
        raise L.TcdiffError(f"write_avi: the file would hold {size + 8} bytes, above AVI 1.0's {MAX_AVI_BYTES} (OpenDML is not built)")
    path = os.fspath(path)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", size))
        for p in body:
            f.write(p)
    return path


def clip_audio_paths(names, mode, folder=None) -> list:
    """The .wav files behind each file ``render_sample`` writes, as the reference finds them: ``splitext(name)[0] + ".wav"`` per
    clip, or in "long" mode one list of every window's file (vis.py:299-317).  With ``folder``, the basenames are looked up
    there.  A file that does not exist raises a TcdiffError that names its path."""
    from .export import _is_long
    if names is None or isinstance(names, (str, os.PathLike)) or len(names) == 0:
        raise L.TcdiffError(f"clip_audio: names must be a list of the clips' names, got {names!r}")
    wavs = [os.path.splitext(os.fspath(n))[0] + ".wav" for n in names]
    if folder is not None:
        wavs = [os.path.join(os.fspath(folder), os.path.basename(w)) for w in wavs]
    for w in wavs:
        if not os.path.isfile(w):
            raise L.TcdiffError(f"clip_audio: {w} does not exist")
    return [wavs] if _is_long(mode) else [[w] for w in wavs]


def clip_audio(names, mode, folder=None, device="cuda:0") -> list:
    """[(samples, sample_rate)] per file ``render_sample`` writes: the clip's sound as the reference finds it -- its .wav in
    "normal" mode; in "long" mode the first window's file whole, then the second half of each following one, ``half`` being half
    of the FIRST file's length (vis.py:299-310).  Read through ``audio.read_wav`` and ``audio.decode`` at the file's own rate, mono
    (``librosa.load(..., sr=None)``); samples float32 (n,) on the host.  No resampling: the rate is that of the last file read,
    as in the reference."""
    from . import audio as A
    out = []
    for group in clip_audio_paths(names, mode, folder):
        wavs = [A.read_wav(w) for w in group]
        first = A.decode(wavs[0], device)[0]
        ll, half = first.numel(), first.numel() // 2
        total = torch.zeros(ll + half * (len(wavs) - 1), dtype=torch.float32, device=first.device)
        total[:ll] = first
        at = ll
        for w in wavs[1:]:
            tail = A.decode(w, device)[0][half:][:half]
            total[at:at + tail.numel()] = tail
            at += half
        out.append((total.cpu().numpy(), wavs[-1].sr))
    return out
