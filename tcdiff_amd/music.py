"""From a waveform to `cond`: the reference's librosa front end (data/data_preprocess/dataset_utils.py:45-86) on the device
(csrc/music.hip, csrc/beat.hip, csrc/chroma.hip; the definitions in include/tcdiff_hip.h).

    cond = music_cond(audio)                               # (B, T, 438), the layout every entry point of this package reads

    cond = wav_cond("song.wav", slices=(0.5, 5.0))         # the same from a WAV file on disk, one row per 5-second slice

``audio`` holds samples at ``sr``; ``tcdiff_amd.audio`` brings them from a WAV file (decode, downmix, the slicing of
data/slice.py, resampling to 30720 Hz: two more launches).  The parts, each callable alone:

    feats, parts = music_features(audio, return_parts=True)    # (B, T, 425): mfcc, delta, onset_env, tempogram; eleven launches
    tempo, onset_beat = beat_track(parts["onset_env"])     # (B,) float64 beats per minute, (B, T) one-hot: two more launches
    chroma = chroma_cqt(parts["harmonic"])                 # (B, T, 12), librosa's chroma_cqt with its tuning estimate: four more
    cond = assemble_cond(feats, chroma, onset_beat)

Eleven launches of ``music_features`` for any number of clips: STFT + mel power; clip maximum; dB + MFCC + delta; the two 31-tap
medians; masks + inverse FFT; overlap-add; STFT + mel power of the percussive signal; its clip maximum; onset envelope; tempogram.
``chroma_cqt``: the six-signal decimation pyramid; the STFT of the harmonic signal; the tuning estimate; the seven-octave
constant-Q response with the fold to 12 chroma.  The definitions restate librosa 0.9 (and resampy's kaiser_fast filter); neither
is a dependency and parity with their own output is not pinned."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import audio
from . import kernels as K

N_FFT, HOP, N_BINS, N_MELS, N_MFCC, TEMPO_WIN, N_COLS = L.MUSIC_N_FFT, L.MUSIC_HOP, L.MUSIC_N_FFT // 2 + 1, L.MUSIC_N_MELS, \
    L.MUSIC_N_MFCC, L.MUSIC_TEMPO_WIN, L.MUSIC_COLS
COND_COLS, CHROMA0, N_CHROMA, ONSET_BEAT = 438, 40, 12, 53      # the row of dataset_utils.py:75-82 (metrics.ONSET_BEAT)
BEAT_WIN = L.BEAT_WIN                                     # the tempo estimate's 8-second window; beat periods are 1 .. 479 frames
CQT_BPO, CQT_OCTAVES, CQT_BINS, CQT_N_FFT, CQT_BAND, N_TUNINGS = L.CHROMA_BPO, L.CHROMA_OCTAVES, L.CHROMA_BINS, L.CHROMA_N_FFT, \
    L.CHROMA_BAND, L.CHROMA_TUNINGS
CQT_FMIN = 32.70319566257483                              # C1
CQT_Q = 1.0 / (2.0 ** (1.0 / CQT_BPO) - 1.0)
TUNINGS = np.linspace(-0.5, 0.5, N_TUNINGS + 1)           # tuning k is TUNINGS[k], in fractions of a 1/36-octave bin; the histogram's edges

_TABLES = {}


def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), f * (3.0 / 200.0))


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)), m * (200.0 / 3.0))


def mel_filter_bank(sr) -> np.ndarray:
    """(128, 1025) float64: Slaney-scale triangles over [0, sr / 2] with Slaney's area normalisation"""
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), N_MELS + 2))
    bins = np.arange(N_BINS) * (sr / N_FFT)
    up = (bins[None, :] - edges[:-2, None]) / (edges[1:-1] - edges[:-2])[:, None]
    down = (edges[2:, None] - bins[None, :]) / (edges[2:] - edges[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(up, down)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def _hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def _tables(sr, device):
    """the constant tables of include/tcdiff_hip.h: float64 on the host, rounded once, uploaded once per (sr, device)"""
    key = (float(sr), str(device))
    tab = _TABLES.get(key)
    if tab is None:
        a = 2.0 * np.pi * np.arange(N_FFT // 2) / N_FFT
        W = mel_filter_bank(float(sr)).astype(np.float32)
        nz = W != 0
        lo = np.where(nz.any(1), nz.argmax(1), 0)
        hi = np.where(nz.any(1), N_BINS - nz[:, ::-1].argmax(1), 0)
        k, m = np.arange(N_MFCC)[:, None], np.arange(N_MELS)[None, :]
        dct = np.cos(np.pi * (2 * m + 1) * k / (2 * N_MELS)) * np.where(k == 0, np.sqrt(1.0 / N_MELS), np.sqrt(2.0 / N_MELS))
        up = lambda x, dt=np.float32: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(device)
        tab = dict(twiddle=up(np.stack([np.cos(a), -np.sin(a)], 1)), window=up(_hann(N_FFT)), tempo_window=up(_hann(TEMPO_WIN)),
                   mel_w=up(W), mel_range=up(np.stack([lo, hi], 1), np.int32), dct=up(dct))
        _TABLES[key] = tab
    return tab


def music_features(audio, *, sr=30720, return_parts=False):
    """audio (n,) or (B, n) float32 on the device, samples at ``sr`` Hz, n >= 2048, read through its row stride (only the last
    dimension must be contiguous) -> (B, T, 425) float32, T = 1 + n // 512 frames: columns 0-19 MFCC of the mel-dB spectrogram,
    20-39 their delta, 40 the onset envelope of the percussive part, 41-424 its tempogram.  ``sr`` (default 60 fps x 512) only
    enters the mel filter bank.

    ``return_parts=True`` -> (feats, parts): ``mel_db`` (B, T, 128), ``harmonic`` and ``percussive`` (B, n), ``onset_env`` (B, T).
    The harmonic signal is only computed when asked for."""
    if not isinstance(audio, torch.Tensor) or audio.dim() not in (1, 2):
        raise L.TcdiffError(f"music_features: audio must be (n,) or (B, n), got {tuple(audio.shape) if isinstance(audio, torch.Tensor) else type(audio)}")
    if audio.dtype != torch.float32:
        raise L.TcdiffError(f"music_features: audio must be float32, got {audio.dtype}")
    y = audio if audio.dim() == 2 else audio[None]
    B, n = y.shape
    if B < 1:
        raise L.TcdiffError("music_features: audio has no clip")
    if n < N_FFT:
        raise L.TcdiffError(f"music_features: a clip needs at least {N_FFT} samples, got {n}")
    if y.stride(1) != 1:
        raise L.TcdiffError(f"music_features: the last dimension of audio must be contiguous (strides {tuple(audio.stride())})")
    try:
        sr = float(sr)
    except (TypeError, ValueError):
        raise L.TcdiffError(f"music_features: sr must be a number, got {sr!r}") from None
    if not (sr > 0 and np.isfinite(sr)):
        raise L.TcdiffError(f"music_features: sr must be positive, got {sr!r}")
    if not y.is_cuda:
        raise L.TcdiffError("music_features runs on MI355X only (no CPU fallback)")
    dev = y.device
    T = 1 + n // HOP
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        tab = _tables(sr, dev)
        D, S, H, P, M = f32(B, T, N_BINS, 2), f32(B, T, N_BINS), f32(B, T, N_BINS), f32(B, T, N_BINS), f32(B, T, N_MELS)
        frames = f32(B, 2 if return_parts else 1, T, N_FFT)
        fmax, mx, mel_db, feats, onset_env = f32(B, T), f32(B), f32(B, T, N_MELS), f32(B, T, N_COLS), f32(B, T)
        percussive = f32(B, n)
        harmonic = f32(B, n) if return_parts else None
        K.music_stft(y, tab, D, S, M, fmax)
        K.music_mfcc(M, fmax, tab, mx, mel_db, feats)
        K.music_hpss(D, S, n, tab, H, P, frames, percussive, harmonic)
        K.music_stft(percussive, tab, None, None, M, fmax)
        K.music_onset(M, fmax, tab, mx, onset_env, feats)
    if return_parts:
        return feats, dict(mel_db=mel_db, harmonic=harmonic, percussive=percussive, onset_env=onset_env)
    return feats


def beat_tables(tightness) -> np.ndarray:
    """(2, 480^2 - 1) float64, the tracker's two tables for every period p = 1 .. 479, row p at offset p^2 - 1 (include/tcdiff_hip.h):
    the local score's window exp(-0.5 (32 j / p)^2), j = -p .. p, and the programme's transition score
    -tightness ln(-d / p)^2, d = -2 p .. -rint(p / 2) (numpy's round: half to even)"""
    tab = np.zeros((2, L.BEAT_TABLE), np.float64)
    with np.errstate(divide="ignore"):                    # p = 1: d = 0 scores -inf
        for p in range(1, BEAT_WIN):
            at = p * p - 1
            tab[0, at:at + 2 * p + 1] = np.exp(-0.5 * (np.arange(-p, p + 1) * 32.0 / p) ** 2)
            d = np.arange(-2 * p, -int(np.round(p / 2)) + 1)
            tab[1, at:at + len(d)] = -tightness * (np.log(-d / p) ** 2)
    return tab


def tempo_prior(start_bpm, std_bpm, max_tempo) -> np.ndarray:
    """(480,) float64: the log-normal prior over the lags' tempi 3600 / l; -inf for l = 0 and wherever 3600 / l >= max_tempo"""
    with np.errstate(divide="ignore"):
        bpms = 3600.0 / np.arange(BEAT_WIN)
    prior = -0.5 * ((np.log2(bpms) - np.log2(start_bpm)) / std_bpm) ** 2
    prior[bpms >= max_tempo] = -np.inf
    return prior


def _beat_tables(tightness, device):
    """uploaded once per (tightness, device), as ``_tables``"""
    key = ("beat", float(tightness), str(device))
    tab = _TABLES.get(key)
    if tab is None:
        tab = dict(tables=torch.from_numpy(beat_tables(float(tightness))).to(device),
                   window=torch.from_numpy(_hann(BEAT_WIN).astype(np.float32)).to(device))
        _TABLES[key] = tab
    return tab


def _beat_prior(start_bpm, std_bpm, max_tempo, device):
    key = ("prior", start_bpm, std_bpm, max_tempo, str(device))
    tab = _TABLES.get(key)
    if tab is None:
        tab = _TABLES[key] = torch.from_numpy(tempo_prior(start_bpm, std_bpm, max_tempo)).to(device)
    return tab


def _positive(name, v):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise L.TcdiffError(f"beat_track: {name} must be a number, got {v!r}") from None
    if not (v > 0 and np.isfinite(v)):
        raise L.TcdiffError(f"beat_track: {name} must be positive and finite, got {v!r}")
    return v


def beat_track(onset_env, *, bpm=None, start_bpm=120.0, std_bpm=1.0, max_tempo=320.0, tightness=100.0, trim=True, return_parts=False):
    """onset_env (T,) or (B, T) float32 on the device, T >= 5 frames at 60 per second (``parts["onset_env"]`` of
    ``music_features``; finite and non-negative), read through its row stride -> (tempo (B,) float64 in beats per minute, onset_beat (B, T) float32, 1 at
    the beat frames): librosa 0.9.2's ``beat.beat_track`` -- tempo from the mean 8-second autocorrelation under a log-normal
    prior, then the dynamic-programme tracker, with librosa's trimming of weak leading / trailing beats -- in two launches, or one
    when ``bpm`` (a number, or one per clip) is given.  A silent clip has tempo 0 and no beats.

    ``return_parts=True`` -> (tempo, onset_beat, parts): ``period`` (B,) int32 frames per beat, ``local_score`` and ``cum_score``
    (B, T) float64, ``backlink`` (B, T) int32, ``n_beats`` (B,) int32."""
    if not isinstance(onset_env, torch.Tensor) or onset_env.dim() not in (1, 2):
        raise L.TcdiffError(f"beat_track: onset_env must be (T,) or (B, T), got "
                            f"{tuple(onset_env.shape) if isinstance(onset_env, torch.Tensor) else type(onset_env)}")
    if onset_env.dtype != torch.float32:
        raise L.TcdiffError(f"beat_track: onset_env must be float32, got {onset_env.dtype}")
    o = onset_env if onset_env.dim() == 2 else onset_env[None]
    B, T = o.shape
    if B < 1:
        raise L.TcdiffError("beat_track: onset_env has no clip")
    if T < 5:
        raise L.TcdiffError(f"beat_track: a clip needs at least 5 frames, got {T}")
    if o.stride(1) != 1:
        raise L.TcdiffError(f"beat_track: the last dimension of onset_env must be contiguous (strides {tuple(onset_env.stride())})")
    tightness = _positive("tightness", tightness)
    periods = None
    if bpm is None:
        start_bpm, std_bpm, max_tempo = _positive("start_bpm", start_bpm), _positive("std_bpm", std_bpm), _positive("max_tempo", max_tempo)
        if not max_tempo > 3600.0 / (BEAT_WIN - 1):
            raise L.TcdiffError(f"beat_track: max_tempo {max_tempo} leaves no lag below {BEAT_WIN}")
    else:
        bpms = [bpm] * B if np.ndim(bpm) == 0 else list(bpm)
        if len(bpms) != B:
            raise L.TcdiffError(f"beat_track: bpm must be a number or one per clip ({B}), got {len(bpms)}")
        bpms = [_positive("bpm", v) for v in bpms]
        periods = [int(np.round(3600.0 / v)) for v in bpms]           # half to even, as librosa 0.9.2
        if not all(1 <= p < BEAT_WIN for p in periods):
            raise L.TcdiffError(f"beat_track: bpm {bpm!r} gives a period outside [1, {BEAT_WIN - 1}] frames")
    if not o.is_cuda:
        raise L.TcdiffError("beat_track runs on MI355X only (no CPU fallback)")
    dev = o.device
    new = lambda dt, *s: torch.empty(*s, dtype=dt, device=dev)
    with torch.cuda.device(dev):
        tab = _beat_tables(tightness, dev)
        local_score, cum_score = new(torch.float64, B, T), new(torch.float64, B, T)
        backlink, beats_ws, onset_beat = new(torch.int32, B, T), new(torch.int32, B, T), new(torch.float32, B, T)
        n_beats = new(torch.int32, B)
        if periods is None:
            tempo, period, prior = new(torch.float64, B), new(torch.int32, B), _beat_prior(start_bpm, std_bpm, max_tempo, dev)
            partial = new(torch.float64, B, -(-T // L.BEAT_CHUNK), BEAT_WIN)
            K.beat_tempo(o, tab["window"], partial)
        else:
            tempo, period = torch.tensor(bpms, dtype=torch.float64, device=dev), torch.tensor(periods, dtype=torch.int32, device=dev)
            prior = partial = None
        K.beat_track(o, partial, prior, tab["tables"], periods, trim, local_score, cum_score, backlink, beats_ws, onset_beat, period,
                     n_beats, tempo)
    if return_parts:
        return tempo, onset_beat, dict(period=period, local_score=local_score, cum_score=cum_score, backlink=backlink, n_beats=n_beats)
    return tempo, onset_beat


def resample_taps() -> np.ndarray:
    """(63,) float64, h[j + 31] for j = -31 .. 31: resampy's kaiser_fast filter as a decimation by exactly two reads it, every
    256th entry of win[m] = 0.85 sinc(0.85 m / 512) kaiser(2 * 8192 + 1, 8.555504641634386)[8192 + m], halved"""
    m = 256 * np.abs(np.arange(-31, 32))
    return 0.5 * 0.85 * np.sinc(0.85 * m / 512.0) * np.kaiser(2 * 8192 + 1, 8.555504641634386)[8192 + m]


def cqt_basis(sr=30720) -> dict:
    """The constant-Q tables of include/tcdiff_hip.h for all 100 tunings, float64 / complex128 on the host: ``basis``
    (100, 36, 24) complex, row r of tuning k holding bins ``band`` (100, 36, 2) = [lo, hi) of the top octave's 513-bin filter
    (octave i uses it times sqrt(2^i)); ``scale`` (100, 252), lowest bin first, sqrt(2^i) over the root of the bin's filter
    length at the original rate.  Raises where ``sr`` leaves librosa's path at 30720 Hz (a 1024-point basis, no early
    downsampling, no separate top octave) or a band wider than 24 bins."""
    sr = float(sr)
    r = np.arange(CQT_BPO)
    basis = np.zeros((N_TUNINGS, CQT_BPO, CQT_BAND), np.complex128)
    band = np.zeros((N_TUNINGS, CQT_BPO, 2), np.int64)
    scale = np.zeros((N_TUNINGS, CQT_BINS), np.float64)
    for k in range(N_TUNINGS):
        fmin = CQT_FMIN * 2.0 ** (TUNINGS[k] / CQT_BPO)
        freqs = fmin * 2.0 ** ((CQT_OCTAVES - 1) + r / CQT_BPO)
        lens = CQT_Q * sr / freqs
        cutoff = freqs[-1] * (1.0 + 0.5 * 1.50018310546875 / CQT_Q)
        early = max(0, int(np.ceil(np.log2(0.85 * (sr / 2.0) / cutoff)) - 1) - 1) if cutoff < 0.85 * sr / 2.0 else -1
        if not (CQT_N_FFT // 2 < np.ceil(lens.max()) <= CQT_N_FFT) or early != 0:
            raise L.TcdiffError(f"chroma_cqt: sr {sr} is not supported (the constant-Q path is built for a 1024-point basis without "
                                f"early downsampling, as at 30720 Hz)")
        rows = np.zeros((CQT_BPO, CQT_N_FFT // 2 + 1), np.complex128)
        for i, (f, ln) in enumerate(zip(freqs, lens)):
            a = np.arange(-ln // 2, ln // 2, dtype=float)
            w = np.zeros(len(a))
            nw = min(int(np.floor(ln)), len(a))
            w[:nw] = _hann(int(np.floor(ln)))[:nw]
            sig = np.exp(2j * np.pi * f * a / sr) * w
            sig /= np.abs(sig).sum()
            padded = np.zeros(CQT_N_FFT, np.complex128)
            lpad = (CQT_N_FFT - len(sig)) // 2
            padded[lpad:lpad + len(sig)] = sig * (ln / CQT_N_FFT)
            rows[i] = np.fft.fft(padded)[:CQT_N_FFT // 2 + 1]
        mags = np.abs(rows)
        srt = np.sort(mags, axis=1)
        cum = np.cumsum(srt / mags.sum(axis=1, keepdims=True), axis=1)
        cut = srt[r, np.argmin(cum < 0.01, axis=1)]
        rows = np.where(mags >= cut[:, None], rows, 0).astype(np.complex64)
        nz = rows != 0
        lo, hi = nz.argmax(1), rows.shape[1] - nz[:, ::-1].argmax(1)
        if (hi - lo).max() > CQT_BAND:
            raise L.TcdiffError(f"chroma_cqt: sr {sr} gives a filter band of {(hi - lo).max()} bins (at most {CQT_BAND})")
        for i in range(CQT_BPO):
            basis[k, i, :hi[i] - lo[i]] = rows[i, lo[i]:hi[i]]
        band[k, :, 0], band[k, :, 1] = lo, hi
        b = np.arange(CQT_BINS)
        scale[k] = np.sqrt(2.0 ** (CQT_OCTAVES - 1 - b // CQT_BPO)) / np.sqrt(CQT_Q * sr / (fmin * 2.0 ** (b / CQT_BPO)))
    return dict(basis=basis, band=band, scale=scale)


def _tuning_tables(sr, device):
    """what the tuning estimate reads: piptrack's band of interior STFT bins, the bin width and the histogram's edges"""
    key = ("tuning", float(sr), str(device))
    tab = _TABLES.get(key)
    if tab is None:
        freqs = np.arange(N_BINS) * (float(sr) / N_FFT)
        pitched = np.nonzero((150.0 <= freqs[1:N_BINS - 1]) & (freqs[1:N_BINS - 1] < 4000.0))[0] + 1
        if len(pitched) == 0:
            raise L.TcdiffError(f"estimate_tuning: sr {sr} leaves no STFT bin in [150, 4000) Hz")
        tab = dict(edges=torch.from_numpy(TUNINGS).to(device), f_lo=int(pitched[0]), f_hi=int(pitched[-1]),
                   bin_hz=float(np.float32(float(sr) / N_FFT)))
        _TABLES[key] = tab
    return tab


def _chroma_tables(sr, device):
    """the constant-Q tables, uploaded once per (sr, device), as ``_tables``"""
    key = ("chroma", float(sr), str(device))
    tab = _TABLES.get(key)
    if tab is None:
        cq = cqt_basis(sr)
        a = 2.0 * np.pi * np.arange(CQT_N_FFT // 2) / CQT_N_FFT
        up = lambda x, dt=np.float32: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(device)
        tab = dict(taps=up(resample_taps()), twiddle=up(np.stack([np.cos(a), -np.sin(a)], 1)),
                   basis=up(np.stack([cq["basis"].real, cq["basis"].imag], -1)), band=up(cq["band"], np.int32), scale=up(cq["scale"]))
        _TABLES[key] = tab
    return tab


def _clips(name, what, x, sr):
    """the checks of ``music_features`` on a (n,) or (B, n) signal -> ((B, n) view, sr)"""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise L.TcdiffError(f"{name}: {what} must be (n,) or (B, n), got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
    if x.dtype != torch.float32:
        raise L.TcdiffError(f"{name}: {what} must be float32, got {x.dtype}")
    y = x if x.dim() == 2 else x[None]
    B, n = y.shape
    if B < 1:
        raise L.TcdiffError(f"{name}: {what} has no clip")
    if n < N_FFT:
        raise L.TcdiffError(f"{name}: a clip needs at least {N_FFT} samples, got {n}")
    if y.stride(1) != 1:
        raise L.TcdiffError(f"{name}: the last dimension of {what} must be contiguous (strides {tuple(x.stride())})")
    try:
        sr = float(sr)
    except (TypeError, ValueError):
        raise L.TcdiffError(f"{name}: sr must be a number, got {sr!r}") from None
    if not (sr > 0 and np.isfinite(sr)):
        raise L.TcdiffError(f"{name}: sr must be positive, got {sr!r}")
    return y, sr


def _estimate_tuning(y, sr):
    """y (B, n) on the device, checked -> (tuning_index, parts), two launches"""
    dev = y.device
    B, n = y.shape
    T = 1 + n // HOP
    new = lambda dt, *s: torch.empty(*s, dtype=dt, device=dev)
    tab, ctab = _tables(sr, dev), _tuning_tables(sr, dev)
    W = ctab["f_hi"] - ctab["f_lo"] + 1
    D, S = new(torch.float32, B, T, N_BINS, 2), new(torch.float32, B, T, N_BINS)
    M, fmax = new(torch.float32, B, T, N_MELS), new(torch.float32, B, T)
    pitch_ws, mag_ws = new(torch.float32, B, T, W), new(torch.float32, B, T, W)
    tuning_index, n_pitches, counts = new(torch.int32, B), new(torch.int32, B), new(torch.int32, B, N_TUNINGS)
    threshold = new(torch.float32, B)
    K.music_stft(y, tab, D, S, M, fmax)                  # (hands out the magnitude, |D|)
    K.chroma_tuning(S, ctab["f_lo"], ctab["f_hi"], ctab["bin_hz"], ctab["edges"], pitch_ws, mag_ws, tuning_index, n_pitches, threshold,
                    counts)
    return tuning_index, dict(n_pitches=n_pitches, threshold=threshold, counts=counts)


def estimate_tuning(harmonic, *, sr=30720, return_parts=False):
    """harmonic (n,) or (B, n) float32 on the device, n >= 2048, read through its row stride -> (B,) int32, the tuning index k in
    0 .. 99: librosa 0.9.2's ``estimate_tuning`` (piptrack on the 2048-point STFT, the pitches at or above the median magnitude,
    the histogram of their residuals in 100 cells, first argmax) at 36 bins per octave; the tuning is ``TUNINGS[k]``, a fraction
    of a 1/36-octave bin.  A clip without a pitch gets 50 (tuning 0.0).  The residual is computed in float64 from the float32
    pitch where librosa stays in float32.

    ``return_parts=True`` -> (index, parts): ``n_pitches`` (B,) int32, ``threshold`` (B,) float32 the median magnitude,
    ``counts`` (B, 100) int32 the histogram."""
    y, sr = _clips("estimate_tuning", "harmonic", harmonic, sr)
    if not y.is_cuda:
        raise L.TcdiffError("estimate_tuning runs on MI355X only (no CPU fallback)")
    with torch.cuda.device(y.device):
        tuning_index, parts = _estimate_tuning(y, sr)
    return (tuning_index, parts) if return_parts else tuning_index


def _tuning_indices(tuning, B):
    """a given tuning, a number or one per clip (a tensor is copied to the host once), in [-0.5, 0.5) on the 0.01 grid -> B indices"""
    if isinstance(tuning, torch.Tensor):
        if tuning.dim() > 1:
            raise L.TcdiffError(f"chroma_cqt: tuning must be a number or one per clip ({B}), got shape {tuple(tuning.shape)}")
        tuning = tuning.detach().cpu().tolist()
    vals = [tuning] * B if np.ndim(tuning) == 0 else list(tuning)
    if len(vals) != B:
        raise L.TcdiffError(f"chroma_cqt: tuning must be a number or one per clip ({B}), got {len(vals)}")
    out = []
    for v in vals:
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise L.TcdiffError(f"chroma_cqt: tuning must be a number, got {v!r}") from None
        if not -0.5 <= v < 0.5:
            raise L.TcdiffError(f"chroma_cqt: tuning must lie in [-0.5, 0.5), got {v!r}")
        k = int(np.round((v + 0.5) * N_TUNINGS))
        if k >= N_TUNINGS or abs(v - TUNINGS[k]) > 1e-9:
            raise L.TcdiffError(f"chroma_cqt: tuning must be a multiple of 0.01 (the estimate's grid), got {v!r}")
        out.append(k)
    return out


def chroma_cqt(harmonic, *, sr=30720, tuning=None, return_parts=False):
    """harmonic (n,) or (B, n) float32 on the device (``parts["harmonic"]`` of ``music_features``), n >= 2048, read through its
    row stride -> (B, T, 12) float32, T = 1 + n // 512: librosa 0.9.2's ``chroma_cqt(y=harmonic, sr=sr, n_octaves=7)`` -- seven
    octaves of 36 constant-Q bins from C1 at hop 512, each octave on the signal decimated once more by resampy's kaiser_fast
    filter, magnitudes folded to 12 chroma and divided by the frame's maximum (a frame of zeros stays zeros).

    ``tuning=None`` estimates the tuning on the device (``estimate_tuning``); the response launch reads the clip's index there and
    picks that tuning's filters, so nothing comes back to the host.  A number, or one per clip, in [-0.5, 0.5) on the 0.01 grid
    skips the estimate.  Four launches, two with a given tuning.

    ``return_parts=True`` -> (chroma, parts): ``tuning_index`` (B,) int32, ``cqt_mag`` (B, T, 252) float32 the magnitudes after
    the length scaling, lowest bin first, ``pyramid`` the six decimated signals (B, ceil(n / 2^s)), s = 1 .. 6."""
    y, sr = _clips("chroma_cqt", "harmonic", harmonic, sr)
    B, n = y.shape
    given = None if tuning is None else _tuning_indices(tuning, B)
    if not y.is_cuda:
        raise L.TcdiffError("chroma_cqt runs on MI355X only (no CPU fallback)")
    dev = y.device
    T = 1 + n // HOP
    lens = [-(-n // (1 << s)) for s in range(1, CQT_OCTAVES)]
    with torch.cuda.device(dev):
        ctab = _chroma_tables(sr, dev)
        pyramid = torch.empty(B, sum(lens), dtype=torch.float32, device=dev)
        chroma = torch.empty(B, T, N_CHROMA, dtype=torch.float32, device=dev)
        cqt_mag = torch.empty(B, T, CQT_BINS, dtype=torch.float32, device=dev) if return_parts else None
        K.chroma_pyramid(y, ctab["taps"], pyramid)
        if given is None:
            tuning_index, _ = _estimate_tuning(y, sr)
        else:
            tuning_index = torch.tensor(given, dtype=torch.int32, device=dev)
        K.chroma_response(y, pyramid, tuning_index, ctab, chroma, cqt_mag)
    if return_parts:
        at = np.concatenate([[0], np.cumsum(lens)])
        return chroma, dict(tuning_index=tuning_index, cqt_mag=cqt_mag,
                            pyramid=[pyramid[:, at[s]:at[s + 1]] for s in range(CQT_OCTAVES - 1)])
    return chroma


def music_cond(audio, chroma=None, *, sr=30720) -> torch.Tensor:
    """audio (n,) or (B, n) float32 on the device -> cond (B, T, 438): ``music_features``, ``beat_track`` of its onset envelope,
    ``chroma_cqt`` of its harmonic signal and ``assemble_cond``.  A given ``chroma`` (B, T, 12) takes the place of the computed
    columns 40-51."""
    feats, parts = music_features(audio, sr=sr, return_parts=True)
    _, onset_beat = beat_track(parts["onset_env"])
    if chroma is None:
        chroma = chroma_cqt(parts["harmonic"], sr=sr)
    return assemble_cond(feats, chroma, onset_beat)


def wav_cond(files, *, slices=None, sr=30720, device="cuda:0") -> torch.Tensor:
    """WAV files (paths, bytes or ``audio.WavData``; see ``audio.load_audio``) -> cond (B, T, 438): ``music_cond`` of
    ``audio.load_audio(files, sr=sr, slices=slices)``, the reference's ``librosa.load(wav_path, sr=30720)`` in front of its feature
    extraction.  With ``slices=(stride, length)`` in seconds the rows are the slices of one file."""
    return music_cond(audio.load_audio(files, sr=sr, slices=slices, device=device), sr=sr)


def assemble_cond(stft_feats, chroma, onset_beat) -> torch.Tensor:
    """stft_feats (B, T, 425) of ``music_features``, chroma (B, T, 12), onset_beat (B, T) -> cond (B, T, 438) in the reference's
    column order: mfcc 0-19, delta 20-39, chroma 40-51, onset_env 52, onset_beat 53, tempogram 54-437.  Both missing parts are
    required: nothing is filled with zeros."""
    for name, t, last in (("stft_feats", stft_feats, N_COLS), ("chroma", chroma, N_CHROMA), ("onset_beat", onset_beat, None)):
        rank = 3 if last else 2
        if not isinstance(t, torch.Tensor) or t.dim() != rank or (last and t.shape[-1] != last):
            want = f"(B, T, {last})" if last else "(B, T)"
            raise L.TcdiffError(f"assemble_cond: {name} must be {want}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
        if t.dtype != torch.float32:
            raise L.TcdiffError(f"assemble_cond: {name} must be float32, got {t.dtype}")
        if t.shape[:2] != stft_feats.shape[:2]:
            raise L.TcdiffError(f"assemble_cond: {name} {tuple(t.shape)} does not match stft_feats {tuple(stft_feats.shape)}")
        if t.device != stft_feats.device:
            raise L.TcdiffError("assemble_cond: the three parts must be on one device")
    cond = torch.cat([stft_feats[..., :CHROMA0], chroma, stft_feats[..., CHROMA0:CHROMA0 + 1], onset_beat[..., None],
                      stft_feats[..., CHROMA0 + 1:]], dim=-1)
    assert cond.shape[-1] == COND_COLS
    return cond
