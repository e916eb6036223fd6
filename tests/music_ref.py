"""The STFT-path music features, restated from the definitions in include/tcdiff_hip.h with numpy and the scipy primitives librosa
itself calls (scipy.fft.rfft / irfft / dct, scipy.ndimage.median_filter, scipy.signal.get_window / savgol_filter, numpy.pad):
librosa 0.9 as the reference's data/data_preprocess/dataset_utils.py:45-86 calls it.  Every function takes ``dtype``: float64 is
the yardstick of tests/test_music_gpu.py, float32 (librosa's own precision: float32 audio, complex64 STFT) its error scale.

librosa is not installed where this project is built, so parity with librosa's own output is NOT pinned by anything here."""
import numpy as np
import scipy.fft
import scipy.ndimage
import scipy.signal

N_FFT, HOP, N_BINS, N_MELS, N_MFCC, TEMPO_WIN, HPSS_TAPS = 2048, 512, 1025, 128, 20, 384, 31
N_COLS = 2 * N_MFCC + 1 + TEMPO_WIN                       # 425: mfcc, delta, onset_env, tempogram
TINY = float(np.finfo(np.float32).tiny)                   # FLT_MIN, whatever dtype the arithmetic runs in (librosa: float32 data)


# ---- test signals ------------------------------------------------------------------------------------------------------------
def make_signal(n, sr=30720, seed=0):
    """n float32 samples: two sinusoids (the second with a slow vibrato), low white noise and a decaying noise burst every sr / 2
    samples (120 BPM)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f1, f2 = 220.0 * (1 + 0.1 * rng.random()), 1320.0 * (1 + 0.1 * rng.random())
    y = 0.3 * np.sin(2 * np.pi * f1 * t + rng.random())
    y += 0.2 * np.sin(2 * np.pi * f2 * t + 6.0 * np.sin(2 * np.pi * 3.0 * t))          # +- 18 Hz at 3 Hz
    y += 0.003 * rng.standard_normal(n)
    period = sr // 2
    k = np.arange(n) % period
    y += 0.5 * rng.standard_normal(n) * np.exp(-k / (0.02 * sr))
    return y.astype(np.float32)


# ---- 1. STFT / 6. ISTFT ------------------------------------------------------------------------------------------------------
def window(n, dtype=np.float64):
    return scipy.signal.get_window("hann", n, fftbins=True).astype(dtype)


def n_frames(n):
    return 1 + n // HOP


def stft(y, dtype=np.float64):
    """y (n,) -> D (1025, T) complex: reflect padding by 1024, frames at hop 512, periodic Hann, real DFT"""
    y = np.asarray(y, dtype)
    yp = np.pad(y, N_FFT // 2, mode="reflect")
    frames = np.lib.stride_tricks.sliding_window_view(yp, N_FFT)[::HOP]
    assert frames.shape[0] == n_frames(len(y))
    return scipy.fft.rfft(frames * window(N_FFT, dtype), axis=-1).T          # complex64 for float32 frames


def istft(D, n, dtype=np.float64):
    """D (1025, T) -> (n,) : inverse real DFT, window, overlap-add in ascending frame order, division by the overlap-added squared
    window where that exceeds FLT_MIN, the first 1024 samples dropped, cut or zero-filled to n"""
    T = D.shape[1]
    w = window(N_FFT, dtype)
    fr = scipy.fft.irfft(D.T, n=N_FFT, axis=-1).astype(dtype) * w
    y = np.zeros(N_FFT + HOP * (T - 1), dtype)
    ws = np.zeros_like(y)
    w2 = w * w
    for t in range(T):
        y[HOP * t:HOP * t + N_FFT] += fr[t]
        ws[HOP * t:HOP * t + N_FFT] += w2
    nz = ws > TINY
    y[nz] /= ws[nz]
    y = y[N_FFT // 2:]
    out = np.zeros(n, dtype)
    m = min(n, len(y))
    out[:m] = y[:m]
    return out


# ---- 2. mel bank ---------------------------------------------------------------------------------------------------------------
def hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3.0))


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_points(sr):
    """the 130 band edges in Hz"""
    return mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), N_MELS + 2))


def mel_bank(sr, dtype=np.float64):
    """W (128, 1025): triangles between the band edges, Slaney area normalisation; built in float64 as librosa does"""
    fft_f = np.linspace(0.0, sr / 2.0, N_BINS)
    mel_f = mel_points(sr)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    W = np.zeros((N_MELS, N_BINS))
    for i in range(N_MELS):
        W[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    W *= (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    return W.astype(dtype)


def mel_power(y, sr, dtype=np.float64):
    """(128, T)"""
    return mel_bank(sr, dtype) @ (np.abs(stft(y, dtype)) ** 2)


# ---- 3. dB / 4. MFCC and delta ---------------------------------------------------------------------------------------------
def power_to_db(M, ref):
    """10 log10(max(1e-10, M)) - 10 log10(max(1e-10, ref)), floored 80 below its own maximum; in M's dtype"""
    amin = M.dtype.type(1e-10)
    db = 10 * np.log10(np.maximum(amin, M)) - 10 * np.log10(np.maximum(amin, M.dtype.type(ref)))
    return np.maximum(db, db.max() - 80)


def mfcc_delta(mel_db):
    """mel_db (128, T) -> mfcc, delta (20, T)"""
    mfcc = scipy.fft.dct(mel_db, axis=0, type=2, norm="ortho")[:N_MFCC]
    delta = scipy.signal.savgol_filter(mfcc, 3, deriv=1, polyorder=1, axis=-1, mode="interp")
    return mfcc, delta.astype(mel_db.dtype)


# ---- 5. HPSS -------------------------------------------------------------------------------------------------------------------
def median_time(S):
    return scipy.ndimage.median_filter(S, size=(1, HPSS_TAPS), mode="reflect")


def median_freq(S):
    return scipy.ndimage.median_filter(S, size=(HPSS_TAPS, 1), mode="reflect")


def softmask(X, R):
    """power 2: (X/Z)^2 / ((X/Z)^2 + (R/Z)^2) with Z = max(X, R); 0.5 where Z < FLT_MIN"""
    Z = np.maximum(X, R)
    bad = Z < TINY
    Zs = np.where(bad, 1, Z).astype(X.dtype)
    m, r = (X / Zs) ** 2, (R / Zs) ** 2
    return np.where(bad, 0.5, m / np.where(bad, 1, m + r)).astype(X.dtype)


def hpss(y, dtype=np.float64):
    """y (n,) -> harmonic, percussive (n,)"""
    D = stft(y, dtype)
    S = np.abs(D)
    H, P = median_time(S), median_freq(S)
    return istft(D * softmask(H, P), len(y), dtype), istft(D * softmask(P, H), len(y), dtype)


# ---- 7. onset envelope / 8. tempogram ------------------------------------------------------------------------------------------
def onset_envelope(percussive, sr, dtype=np.float64):
    """(T,): the median over the mel bins of the positive dB flux, three zeros in front"""
    db = power_to_db(mel_power(percussive, sr, dtype), 1.0)
    flux = np.maximum(0, db[:, 1:] - db[:, :-1])
    med = np.median(flux, axis=0).astype(dtype)
    return np.concatenate([np.zeros(3, dtype), med])[:db.shape[1]]


def tempogram(env):
    """env (T,) -> (384, T): linear autocorrelation of the Hann-windowed 384-frame neighbourhood of every frame (by FFT, as librosa),
    divided by its largest absolute value unless that is below FLT_MIN"""
    T = len(env)
    p = np.pad(env, TEMPO_WIN // 2, mode="linear_ramp", end_values=0)
    fr = np.lib.stride_tricks.sliding_window_view(p, TEMPO_WIN)[:T] * window(TEMPO_WIN, env.dtype)
    n_pad = 2 * TEMPO_WIN + 1
    spec = scipy.fft.rfft(fr, n=n_pad, axis=-1)
    ac = scipy.fft.irfft(np.abs(spec) ** 2, n=n_pad, axis=-1)[:, :TEMPO_WIN].astype(env.dtype)
    mx = np.abs(ac).max(axis=-1, keepdims=True)
    return (ac / np.where(mx < TINY, 1, mx)).astype(env.dtype).T


# ---- the whole front end ---------------------------------------------------------------------------------------------------------
def features(y, sr=30720, dtype=np.float64):
    """y (n,) float32 audio -> dict: feats (T, 425) in the order mfcc, delta, onset_env, tempogram; mel_db (T, 128); harmonic,
    percussive (n,); onset_env (T,); mfcc, delta (T, 20); tempogram (T, 384)"""
    y = np.asarray(y, dtype)
    M = mel_power(y, sr, dtype)
    mel_db = power_to_db(M, M.max())
    mfcc, delta = mfcc_delta(mel_db)
    harmonic, percussive = hpss(y, dtype)
    env = onset_envelope(percussive, sr, dtype)
    tg = tempogram(env)
    feats = np.concatenate([mfcc, delta, env[None], tg], axis=0).T
    assert feats.shape == (n_frames(len(y)), N_COLS)
    return dict(feats=np.ascontiguousarray(feats), mel_db=np.ascontiguousarray(mel_db.T), harmonic=harmonic, percussive=percussive,
                onset_env=env, mfcc=mfcc.T, delta=delta.T, tempogram=tg.T)
