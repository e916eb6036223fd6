"""From a waveform to `cond`: the part of the reference's librosa front end (data/data_preprocess/dataset_utils.py:45-86) that
hangs off one STFT, on the device (csrc/music.hip, the definitions in include/tcdiff_hip.h).

    feats = music_features(audio)                          # (B, T, 425): mfcc, delta, onset_env, tempogram
    cond = assemble_cond(feats, chroma, onset_beat)        # (B, T, 438), the layout every entry point of this package reads

The caller brings samples at ``sr`` (decoding and resampling audio files is not part of this) and the two parts
``music_features`` does not compute: ``chroma`` (librosa's chroma_cqt of the harmonic signal, columns 40-51) and ``onset_beat``
(its beat tracker run on the onset envelope, column 53).  ``return_parts=True`` hands out their inputs, ``harmonic`` and
``onset_env``.  The second of the two is built as well (csrc/beat.hip):

    tempo, onset_beat = beat_track(parts["onset_env"])     # (B,) float64 beats per minute, (B, T) one-hot: two more launches
    cond = music_cond(audio, chroma)                       # the three calls chained

Eleven launches for any number of clips: STFT + mel power; clip maximum; dB + MFCC + delta; the two 31-tap medians; masks + inverse
FFT; overlap-add; STFT + mel power of the percussive signal; its clip maximum; onset envelope; tempogram.  The definitions restate
librosa 0.9; librosa is not a dependency and parity with its own output is not pinned."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import kernels as K

N_FFT, HOP, N_BINS, N_MELS, N_MFCC, TEMPO_WIN, N_COLS = L.MUSIC_N_FFT, L.MUSIC_HOP, L.MUSIC_N_FFT // 2 + 1, L.MUSIC_N_MELS, \
    L.MUSIC_N_MFCC, L.MUSIC_TEMPO_WIN, L.MUSIC_COLS
COND_COLS, CHROMA0, N_CHROMA, ONSET_BEAT = 438, 40, 12, 53      # the row of dataset_utils.py:75-82 (metrics.ONSET_BEAT)
BEAT_WIN = L.BEAT_WIN                                     # the tempo estimate's 8-second window; beat periods are 1 .. 479 frames

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


def music_cond(audio, chroma, *, sr=30720) -> torch.Tensor:
    """audio (n,) or (B, n) float32 on the device, chroma (B, T, 12) -> cond (B, T, 438): ``music_features``, ``beat_track`` of its
    onset envelope and ``assemble_cond``.  ``chroma`` (columns 40-51) stays the caller's."""
    feats, parts = music_features(audio, sr=sr, return_parts=True)
    _, onset_beat = beat_track(parts["onset_env"])
    return assemble_cond(feats, chroma, onset_beat)


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
