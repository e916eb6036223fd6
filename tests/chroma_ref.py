"""Columns 40-51 of `cond`, chroma_cqt of the harmonic signal, restated from the definitions in include/tcdiff_hip.h with numpy
and scipy: librosa 0.9.2's estimate_tuning (piptrack + pitch_tuning), resampy's kaiser_fast at ratio 1/2, the constant-Q
filter basis, the seven-octave response and the fold to 12 chroma, as the reference's data/data_preprocess/_preprocess_wav.py:45-47
calls them (sr 30720, hop 512, 36 bins per octave, 7 octaves from C1).  Every step takes ``dtype``: float64 is the yardstick of
tests/test_chroma_gpu.py, float32 (librosa's own precision) its error scale.  ``tuning_index`` also returns the margin of every
decision it takes, so a test can tell a wrong kernel from a decision no float32 arithmetic could be held to.

Neither librosa nor resampy is installed where this project is built: the definitions are written from knowledge of those
versions, and parity with their own output is NOT pinned by anything here."""
import numpy as np
import scipy.fft
import scipy.signal

import music_ref as MR

SR, HOP, BPO, N_OCT, N_CHROMA = 30720, 512, 36, 7, 12
N_BINS = BPO * N_OCT                                      # 252
N_FFT = 1024                                              # the constant-Q frames; the tuning estimate's STFT is music_ref's (2048)
FMIN0 = 32.70319566257483                                 # C1
ALPHA = 2.0 ** (1.0 / BPO) - 1.0
Q = 1.0 / ALPHA
TINY = float(np.finfo(np.float32).tiny)
N_TUNINGS = 100
EDGES = np.linspace(-0.5, 0.5, N_TUNINGS + 1)            # tuning k is EDGES[k], in fractions of a 1/36-octave bin
N_TAPS, KAISER_BETA, ROLLOFF = 63, 8.555504641634386, 0.85
GUARD_BINS, GUARD_REL = 1e-4, 1e-5                        # a decision closer than this is one float32 arithmetic may take either way


# ---- test signals ------------------------------------------------------------------------------------------------------------
def make_tones(n, seed, sr=SR):
    """n float32 samples: four harmonic tones, a base of 300 .. 495 Hz and its octaves 2, 4, 8, of amplitudes 0.7 .. 1, and with
    them none or two weaker tones (0.3 .. 0.45) elsewhere, plus white noise 40 dB below the loudest tone.  The base sits on a
    bin of the tuning estimate's 2048-point STFT, where piptrack's parabola has no bias, so the four loud tones are detuned
    from the A440 grid by one common fraction of a bin and fall into one histogram cell; their amplitudes are 0.1 apart, so
    the median threshold falls between two of them.  That is what keeps the reference's decision margins positive."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    base = int(rng.integers(20, 34)) * (sr / MR.N_FFT)
    y = np.zeros(n)
    for a, mult in zip(rng.permutation([0.7, 0.8, 0.9, 1.0]), (1, 2, 4, 8)):
        y += a * np.cos(2 * np.pi * base * mult * t + rng.uniform(0, 2 * np.pi))
    for _ in range(2 * int(rng.integers(0, 2))):
        f = rng.uniform(600.0, 3500.0)
        y += rng.uniform(0.3, 0.45) * np.cos(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    y += 0.01 * rng.standard_normal(n)
    return (0.2 * y).astype(np.float32)


def make_tone(n, freq, sr=SR, amp=0.5):
    """one cosine that grows by half over the clip (so no two frames' peaks have the same magnitude), float32"""
    t = np.arange(n) / sr
    return (amp * (1.0 + 0.5 * np.arange(n) / n) * np.cos(2 * np.pi * freq * t)).astype(np.float32)


# the clips of tests/test_chroma_gpu.py, (samples, seeds of make_tones; None: silence): tests/test_chroma_cpu.py asserts that the
# reference's decision margins are positive on every one of them
GPU_CASES = {"A": (2048, (7,)),                          # T = 5, every octave-6 frame mostly padding
             "B": (4095, (8,)),                          # the octaves disagree on the frame count
             "C": (512 * 40 + 137, (4, None, 9))}        # three clips, one of them silent


def case_clip(n, seed):
    return np.zeros(n, np.float32) if seed is None else make_tones(n, seed)


# ---- the resampler: kaiser_fast at ratio 1/2 -------------------------------------------------------------------------------------
def resample_table():
    """win[m], m = 0 .. 8192: the right half of the interpolation filter, 512 samples per zero crossing"""
    m = np.arange(8193)
    return ROLLOFF * np.sinc(ROLLOFF * m / 512.0) * scipy.signal.windows.kaiser(2 * 8192 + 1, KAISER_BETA)[8192 + m]


def resample_taps():
    """h[j + 31], j = -31 .. 31: a decimation by exactly two only ever reads every 256th table entry"""
    return 0.5 * resample_table()[256 * np.abs(np.arange(-31, 32))]


def resample_stage(x, dtype=np.float64):
    """y[t] = sqrt(2) sum_j h[j] x[2 t + j], terms outside the signal dropped, t < ceil(len / 2)"""
    x = np.asarray(x, dtype)
    m = (len(x) + 1) // 2
    xp = np.concatenate([np.zeros(31, dtype), x, np.zeros(32, dtype)])
    rows = np.lib.stride_tricks.sliding_window_view(xp, N_TAPS)[::2][:m]      # row t: x[2 t - 31 .. 2 t + 31]
    return (dtype(np.sqrt(2.0)) * (rows * resample_taps().astype(dtype)).sum(axis=-1, dtype=dtype)).astype(dtype)


def pyramid(y, dtype=np.float64):
    """the six decimated signals, each fed by the one before it"""
    out, x = [], np.asarray(y, dtype)
    for _ in range(N_OCT - 1):
        x = resample_stage(x, dtype)
        out.append(x)
    return out


# ---- the filter basis --------------------------------------------------------------------------------------------------------------
def octave_freqs(tuning, octave=0):
    """the 36 centre frequencies of an octave; 0 is the top one"""
    fmin = FMIN0 * 2.0 ** (tuning / BPO)
    return fmin * 2.0 ** ((N_OCT - 1 - octave) + np.arange(BPO) / BPO)


def cqt_lengths(tuning, sr=SR):
    """(252,) the filter lengths Q sr / f at the original rate, lowest bin first"""
    return Q * sr / (FMIN0 * 2.0 ** (tuning / BPO) * 2.0 ** (np.arange(N_BINS) / BPO))


def sparsify(rows, quantile=0.01):
    mags = np.abs(rows)
    srt = np.sort(mags, axis=1)
    cum = np.cumsum(srt / mags.sum(axis=1, keepdims=True), axis=1)
    idx = np.argmin(cum < quantile, axis=1)
    return np.where(mags >= srt[np.arange(len(rows)), idx][:, None], rows, 0)


def octave_basis_dense(freqs, sr, sparse=True):
    """(36, 513) complex128: the frequency-domain filters of one octave at its own rate, before any rescaling by octave"""
    out = np.zeros((len(freqs), N_FFT // 2 + 1), np.complex128)
    for k, f in enumerate(freqs):
        ln = Q * sr / f
        a = np.arange(-ln // 2, ln // 2, dtype=float)
        w = scipy.signal.get_window("hann", int(np.floor(ln)), fftbins=True)
        w = np.concatenate([w, np.zeros(len(a))])[:len(a)]                    # zero-extended where the filter is one longer
        sig = np.exp(2j * np.pi * f * a / sr) * w
        sig = sig / np.abs(sig).sum()
        lpad = (N_FFT - len(sig)) // 2
        padded = np.zeros(N_FFT, np.complex128)
        padded[lpad:lpad + len(sig)] = sig
        out[k] = scipy.fft.fft(padded * (ln / N_FFT))[:N_FFT // 2 + 1]
    return sparsify(out) if sparse else out


def basis(tuning_index, sr=SR):
    """(36, 513) complex64: the top octave's basis at tuning EDGES[tuning_index]; octave i uses it times sqrt(2^i)"""
    return octave_basis_dense(octave_freqs(EDGES[tuning_index]) * (sr / SR), sr).astype(np.complex64)


def early_downsample_count(tuning, sr=SR):
    """librosa's count of octaves it would decimate before the transform: 0 at these settings"""
    fmax_t = octave_freqs(tuning)[-1]
    nyquist = sr / 2.0
    filter_cutoff = fmax_t * (1 + 0.5 * 1.50018310546875 / Q)
    assert filter_cutoff < ROLLOFF * nyquist
    a = max(0, int(np.ceil(np.log2(ROLLOFF * nyquist / filter_cutoff)) - 1) - 1)
    b = max(0, int(np.log2(HOP)) - N_OCT + 1)            # the hop's factors of two less the octaves it must survive
    return min(a, b)


# ---- the response and the chroma -------------------------------------------------------------------------------------------------
def octave_frames(n_i, octave):
    return 1 + n_i // (HOP >> octave)


def cqt_mag(y, tuning_index, dtype=np.float64, return_pyramid=False):
    """y (n,) -> |C| (T, 252) after the length scaling, lowest bin first; T = the smallest frame count of the seven octaves"""
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    y = np.asarray(y, dtype)
    pyr = pyramid(y, dtype)
    fb = basis(tuning_index).astype(cdt)
    resp = []
    for i, x in enumerate([y] + pyr):
        xp = np.concatenate([np.zeros(N_FFT // 2, dtype), x, np.zeros(N_FFT // 2, dtype)])
        fr = np.lib.stride_tricks.sliding_window_view(xp, N_FFT)[::HOP >> i]
        assert fr.shape[0] == octave_frames(len(x), i)
        D = scipy.fft.fft(fr.astype(cdt), axis=-1)[:, :N_FFT // 2 + 1]
        resp.append(((D @ fb.T) * dtype(np.sqrt(2.0 ** i))).astype(cdt))
    T = min(r.shape[0] for r in resp)
    C = np.concatenate([r[:T] for r in resp[::-1]], axis=1)
    mag = (np.abs(C) / np.sqrt(cqt_lengths(EDGES[tuning_index])).astype(dtype)).astype(dtype)
    return (mag, pyr) if return_pyramid else mag


def fold(mag):
    """(T, 252) -> (T, 12): chroma c sums bins 3 c - 1, 3 c, 3 c + 1 (mod 36) of every octave; each frame over its maximum"""
    w = np.roll(np.repeat(np.eye(N_CHROMA), BPO // N_CHROMA, axis=1), -1, axis=1)
    raw = (mag @ np.tile(w, N_OCT).T.astype(mag.dtype)).astype(mag.dtype)
    mx = raw.max(axis=1, keepdims=True)
    return (raw / np.where(mx < TINY, 1, mx)).astype(mag.dtype)


# ---- the tuning estimate ---------------------------------------------------------------------------------------------------------
def piptrack(S, sr=SR):
    """S (1025, T) -> flag, pitch (float32 values), mag, and the number of flags within the guard of flipping"""
    dt = S.dtype.type
    avg = dt(0.5) * (S[2:] - S[:-2])
    den = dt(2) * S[1:-1] - S[2:] - S[:-2]
    shift = avg / (den + (np.abs(den) < TINY))
    avg, shift = np.pad(avg, ((1, 1), (0, 0))), np.pad(shift, ((1, 1), (0, 0)))
    dskew = dt(0.5) * avg * shift
    freqs = np.arange(S.shape[0]) * (sr / MR.N_FFT)
    band = ((150.0 <= freqs) & (freqs < 4000.0))[:, None]
    ref = dt(0.1) * S.max(axis=0)

    def localmax(Mc, Mn, e):
        lm = np.zeros(S.shape, bool)
        lm[1:-1] = (Mc[1:-1] > Mn[:-2] + e) & (Mc[1:-1] >= Mn[2:] + e) & (Mc[1:-1] > 0)
        return lm & band
    M = S * (S > ref)
    flag = localmax(M, M, 0)
    e = GUARD_REL * S.max(axis=0)
    Mlo, Mhi = S * (S > ref + e), S * (S > ref - e)
    unsure = int((localmax(Mhi, Mlo, -e) & ~localmax(Mlo, Mhi, e)).sum())
    pitch = ((np.arange(S.shape[0], dtype=S.dtype)[:, None] + shift) * dt(sr / MR.N_FFT)).astype(np.float32)
    return flag, pitch, S + dskew, unsure


def tuning_index(y, dtype=np.float64, sr=SR):
    """y (n,) -> (k, info): the tuning index 0 .. 99 and the margins of the decisions behind it.  ``margin`` is the gap between the
    best and second-best histogram counts less the pitches that could fall either way: mag within GUARD_REL of the median
    threshold, residual within GUARD_BINS of a histogram edge, or a piptrack flag within GUARD_REL of flipping.  The index is
    only binding on float32 arithmetic where it is positive (a clip with no pitch at all has margin 1)."""
    S = np.abs(MR.stft(y, dtype)).astype(dtype)
    flag, pitch, mag, unsure_flags = piptrack(S, sr)
    p, m = pitch[flag], mag[flag]
    info = dict(n_pitches=int(flag.sum()), unsure_flags=unsure_flags)
    if p.size == 0:
        info.update(margin=1 - unsure_flags, threshold=0.0, counts=np.zeros(N_TUNINGS, int))
        return 50, info
    thr = np.median(m)
    rel = np.abs(m - thr) / abs(thr)
    keep = m >= thr
    r = np.mod(BPO * np.log2(p[keep].astype(np.float64) / 27.5), 1.0)
    r[r >= 0.5] -= 1.0
    counts, _ = np.histogram(r, EDGES)
    edge_dist = np.abs(r[:, None] - EDGES[None, :]).min(axis=1)
    unsure = int((rel < GUARD_REL).sum()) + int((edge_dist < GUARD_BINS).sum()) + unsure_flags
    order = np.sort(counts)
    k = int(np.argmax(counts))
    info.update(threshold=float(thr), counts=counts, median_margin=float(rel.min()), edge_margin=float(edge_dist.min()),
                gap=int(order[-1] - order[-2]), unsure=unsure, margin=int(order[-1] - order[-2]) - unsure)
    return k, info


# ---- the whole path --------------------------------------------------------------------------------------------------------------
def chroma_cqt(y, tuning_idx=None, dtype=np.float64):
    """y (n,) float32 harmonic signal -> dict: chroma (T, 12), cqt_mag (T, 252), pyramid (six arrays), tuning_index, info"""
    info = None
    if tuning_idx is None:
        tuning_idx, info = tuning_index(y, dtype)
    mag, pyr = cqt_mag(y, tuning_idx, dtype, return_pyramid=True)
    return dict(chroma=fold(mag), cqt_mag=mag, pyramid=pyr, tuning_index=tuning_idx, info=info)
