"""CPU checks of the music front end (no GPU): the numpy / scipy restatement tests/music_ref.py -- the yardstick of
tests/test_music_gpu.py -- against things that can be checked by hand, and the host side of tcdiff_amd.music (tables, validation,
no CPU fallback, the column layout of ``assemble_cond``)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import music_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import metrics as M
from tcdiff_amd import music as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 30720
_cache = {}


def _long():
    """the 451-frame signal of the GPU test's case D and its float64 features, once"""
    if "long" not in _cache:
        y = R.make_signal(450 * 512 + 137, seed=4)
        _cache["long"] = (y, R.features(y))
    return _cache["long"]


# ---- STFT / ISTFT ------------------------------------------------------------------------------------------------------------
def test_stft_of_a_bin_centred_cosine():
    """cos(2 pi 64 i / 2048) under a periodic Hann window: 1024 / 2 in bin 64, half of that (negated) in its two neighbours, nothing
    elsewhere; in every frame the padding leaves periodic, i.e. away from the clip's ends"""
    n = 16 * 2048
    y = np.cos(2 * np.pi * 64 * np.arange(n) / 2048)
    D = R.stft(y)
    assert D.shape == (1025, 1 + n // 512) and D.dtype == np.complex128
    mid = np.abs(D[:, 2:-2])
    want = np.zeros(1025)
    want[64], want[63], want[65] = 512.0, 256.0, 256.0
    assert np.abs(mid - want[:, None]).max() < 1e-9
    # frame t starts 512 t - 1024 samples into the clip: the phase of bin 64 turns by 2 pi 64 / 4 per frame, a whole number of turns
    assert np.abs(D[64, 2:-2] - 512.0).max() < 1e-9
    # reflect padding: the cosine is even about sample 0, so even the first frame sees the same periodic signal
    assert np.abs(np.abs(D[:, 0]) - want).max() < 1e-9
    assert R.stft(y.astype(np.float32), np.float32).dtype == np.complex64


@pytest.mark.parametrize("n", [2048, 12 * 512 + 137, 41 * 512 + 137])
def test_istft_inverts_stft(n):
    y = np.random.default_rng(n).standard_normal(n)
    back = R.istft(R.stft(y), n)
    assert back.shape == (n,) and np.abs(back - y).max() < 1e-12
    assert R.n_frames(n) == 1 + n // 512


def test_istft_zero_fills_past_the_last_frame():
    D = R.stft(np.ones(2048))                             # 5 frames reach 4 * 512 + 1024 samples
    out = R.istft(D, 5000)
    assert out.shape == (5000,) and np.abs(out[:2048] - 1).max() < 1e-12 and (out[3072:] == 0).all()
    assert np.abs(out[2048:3072] - 1).max() < 1e-3        # the last frame's tail alone: divided by a vanishing squared window


# ---- mel bank ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [SR, 22050])
def test_mel_bank(sr):
    assert float(R.hz_to_mel(1000.0)) == 15.0 and float(R.hz_to_mel(200.0 / 3.0)) == pytest.approx(1.0, rel=1e-15)
    assert float(R.mel_to_hz(R.hz_to_mel(6400.0))) == pytest.approx(6400.0, rel=1e-14)
    assert float(R.hz_to_mel(6400.0)) == pytest.approx(15.0 + 27.0, rel=1e-14)          # 27 log steps from 1 kHz to 6.4 kHz
    W = R.mel_bank(sr)
    f = R.mel_points(sr)
    assert W.shape == (128, 1025) and f.shape == (130,) and f[0] == 0 and f[-1] == pytest.approx(sr / 2, rel=1e-14)
    assert np.allclose(np.diff(R.hz_to_mel(f)), R.hz_to_mel(sr / 2) / 129, rtol=1e-12, atol=0)
    assert (W >= 0).all()
    bins = np.arange(1025) * sr / 2048
    for i in range(128):                                  # 2 / (f[i+2] - f[i]) times the triangle 0 - 1 - 0 over f[i], f[i+1], f[i+2]
        tri = np.interp(bins, f[i:i + 3], [0.0, 1.0, 0.0], left=0.0, right=0.0)
        assert np.abs(W[i] - 2.0 / (f[i + 2] - f[i]) * tri).max() < 1e-12 * W[i].max() + 1e-18
    # the package builds the same bank without this file
    assert np.abs(MU.mel_filter_bank(sr) - W).max() < 1e-13


# ---- dB, MFCC, delta -----------------------------------------------------------------------------------------------------------
def test_power_to_db_floor_and_reference():
    Mx = np.array([[1.0, 1e-3], [1e-12, 1e-9]])
    db = R.power_to_db(Mx, Mx.max())
    assert np.allclose(db, [[0.0, -30.0], [-80.0, -80.0]], atol=1e-12)      # 1e-12 -> amin 1e-10 -> -100 -> floor; 1e-9 -> -90 -> floor
    assert np.allclose(R.power_to_db(Mx, 1.0), db, atol=1e-12)


def test_mfcc_is_the_orthonormal_dct_and_the_delta_of_a_ramp_is_one():
    x = np.random.default_rng(0).standard_normal((128, 9))
    mfcc, _ = R.mfcc_delta(x)
    k, m = np.arange(20)[:, None], np.arange(128)[None, :]
    basis = np.cos(np.pi * (2 * m + 1) * k / 256) * np.where(k == 0, np.sqrt(1 / 128), np.sqrt(2 / 128))
    assert np.abs(mfcc - basis @ x).max() < 1e-12
    for T in (5, 9):
        ramp = np.tile(np.arange(T, dtype=np.float64), (128, 1)) * np.arange(1, 129)[:, None]
        c, d = R.mfcc_delta(ramp)
        assert d.shape == (20, T)
        assert np.abs(d - (c[:, 1] - c[:, 0])[:, None]).max() < 1e-9        # slope of each coefficient, the edges included
    one = np.zeros((128, 6))
    one[:, :] = np.arange(6.0)[None, :] / np.sqrt(128.0)                    # every bin t / sqrt(128): coefficient 0 is t, the others 0
    c, d = R.mfcc_delta(one)
    assert np.abs(d[0] - 1.0).max() < 1e-12 and np.abs(d[1:]).max() < 1e-12    # the delta of a ramp is 1 everywhere, edges included
    x = np.random.default_rng(1).standard_normal((128, 7))
    c, d = R.mfcc_delta(x)
    assert np.abs(d[:, 1:-1] - (c[:, 2:] - c[:, :-2]) / 2).max() < 1e-12
    assert np.abs(d[:, 0] - (c[:, 2] - c[:, 0]) / 2).max() < 1e-12 and np.abs(d[:, -1] - (c[:, -1] - c[:, -3]) / 2).max() < 1e-12


# ---- medians and masks ---------------------------------------------------------------------------------------------------------
def _reflect(i, n):
    m = i % (2 * n)
    return m if m < n else 2 * n - 1 - m


@pytest.mark.parametrize("n", [5, 13, 42])
def test_median_filters_against_a_periodic_reflect_evaluation(n):
    S = np.random.default_rng(n).random((n, n))
    Ht, Pf = R.median_time(S), R.median_freq(S)
    for r in range(n):
        for c in range(n):
            assert Ht[r, c] == np.sort([S[r, _reflect(c + d, n)] for d in range(-15, 16)])[15]
            assert Pf[r, c] == np.sort([S[_reflect(r + d, n), c] for d in range(-15, 16)])[15]


def test_softmask():
    X = np.array([3.0, 0.0, 0.0, 1.0, 1e-39])
    Rr = np.array([4.0, 0.0, 2.0, 1.0, 0.0])
    m = R.softmask(X, Rr)
    assert np.allclose(m, [9 / 25, 0.5, 0.0, 0.5, 0.5], atol=1e-15)
    assert np.allclose(m + R.softmask(Rr, X), 1.0, atol=1e-15)


# ---- onset envelope and tempogram -----------------------------------------------------------------------------------------------
def test_onset_envelope_and_tempogram_of_the_120_bpm_signal():
    y, f = _long()
    T = 451
    assert f["feats"].shape == (T, 425) and f["onset_env"].shape == (T,) and (f["onset_env"][:3] == 0).all()
    assert np.array_equal(f["feats"][:, 40], f["onset_env"]) and (f["onset_env"] >= 0).all() and f["onset_env"].max() > 1
    tg = f["tempogram"]
    loud = np.abs(tg).max(axis=1) > 0
    assert loud.sum() > 400 and (tg[loud, 0] == 1.0).all() and np.abs(tg).max() == 1.0
    assert 10 + int(np.argmax(tg[225, 10:])) == 30        # bursts every sr / 2 samples = 30 frames
    assert not any(np.isnan(v).any() for v in f.values())


def test_tempogram_by_direct_autocorrelation():
    env = np.concatenate([np.zeros(3), np.random.default_rng(2).random(37)])
    tg = R.tempogram(env).T                               # (T, 384)
    assert tg.shape == (40, 384)
    left = np.zeros(192)
    right = env[-1] * np.arange(191, -1, -1) / 192
    p = np.concatenate([left, env, right])
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(384) / 384)
    for t in (0, 17, 39):
        x = p[t:t + 384] * w
        ac = np.array([np.dot(x[:384 - k], x[k:]) for k in range(384)])
        assert np.abs(tg[t] - ac / np.abs(ac).max()).max() < 1e-12


def test_digital_silence():
    for dtype in (np.float64, np.float32):
        f = R.features(np.zeros(41 * 512 + 137, np.float32), dtype=dtype)
        for k, v in f.items():
            assert v.dtype == dtype and not np.isnan(v).any() and (v == 0).all(), k


def test_float32_run_stays_float32():
    y = R.make_signal(12 * 512 + 137, seed=2)
    f32, f64 = R.features(y, dtype=np.float32), R.features(y)
    for k in f64:
        assert f32[k].dtype == np.float32 and f64[k].dtype == np.float64 and f32[k].shape == f64[k].shape
        assert np.abs(f32[k] - f64[k]).max() <= 1e-4 * max(1.0, np.abs(f64[k]).max())


# ---- the host side ---------------------------------------------------------------------------------------------------------------
def test_tables():
    tab = MU._tables(SR, "cpu")
    assert MU._tables(SR, "cpu") is tab and MU._tables(22050, "cpu") is not tab
    assert tab["twiddle"].shape == (1024, 2) and tab["window"].shape == (2048,) and tab["tempo_window"].shape == (384,)
    assert tab["mel_w"].shape == (128, 1025) and tab["dct"].shape == (20, 128) and tab["mel_range"].dtype == torch.int32
    half_ulp = 2.0 ** -24                                  # float64 values rounded once: two ways of writing them agree to that
    assert np.abs(tab["window"].numpy() - R.window(2048)).max() <= half_ulp and np.abs(tab["tempo_window"].numpy() - R.window(384)).max() <= half_ulp
    tw = np.exp(-2j * np.pi * np.arange(1024) / 2048)
    assert np.abs(tab["twiddle"].numpy() - np.stack([tw.real, tw.imag], 1)).max() <= half_ulp
    dct = tab["dct"].numpy().astype(np.float64)
    assert np.abs(dct @ dct.T - np.eye(20)).max() < 1e-6
    W = tab["mel_w"].numpy()
    W64 = R.mel_bank(SR)
    assert (np.abs(W - W64) <= half_ulp * W64 + 1e-13).all()
    for i, (lo, hi) in enumerate(tab["mel_range"].numpy()):
        assert 0 <= lo < hi <= 1025 and (W[i, :lo] == 0).all() and (W[i, hi:] == 0).all() and W[i, lo] > 0 and W[i, hi - 1] > 0


def test_argument_errors_and_no_cpu_fallback():
    ok = torch.zeros(2, 4096)
    for bad in (ok.double(), ok[0, :2047], torch.zeros(1, 2, 4096), torch.zeros(()), ok[:, ::2], np.zeros(4096, np.float32), ok[:0]):
        with pytest.raises(L.TcdiffError):
            MU.music_features(bad)
    for sr in (0, -1.0, float("nan"), "x"):
        with pytest.raises(L.TcdiffError):
            MU.music_features(ok, sr=sr)
    with pytest.raises(L.TcdiffError, match="no CPU fallback"):
        MU.music_features(ok)
    with pytest.raises(L.TcdiffError, match="no CPU fallback"):
        MU.music_features(ok[0], return_parts=True)


def test_launchers_validate_before_any_launch():
    from tcdiff_amd import build
    build.build(verbose=False)
    lib = L.load()
    for sym in ("tcdiff_music_stft", "tcdiff_music_mfcc", "tcdiff_music_hpss", "tcdiff_music_onset"):
        assert sym in L.EXPORTS and hasattr(lib, sym)
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert lib.tcdiff_music_stft(None, 4096, 1, 4096, p, p, p, p, p, p, p, p, None) == -1
    assert lib.tcdiff_music_stft(p, 4096, 1, 2047, p, p, p, p, p, p, p, p, None) == -1       # n < 2048
    assert lib.tcdiff_music_stft(p, 4096, 0, 4096, p, p, p, p, p, p, p, p, None) == -1
    assert lib.tcdiff_music_stft(p, 4096, 1, 4096, p, p, p, p, p, None, p, p, None) == -1    # D without S
    assert lib.tcdiff_music_stft(p, 4096, 1, 4096, p, p, p, p, None, None, p, None, None) == -1      # the frame maxima are not optional
    assert lib.tcdiff_music_stft(p, 4096, 65536, 4096, p, p, p, p, p, p, p, p, None) == -4
    assert lib.tcdiff_music_mfcc(p, p, 1, 4, p, p, p, p, None) == -1 and lib.tcdiff_music_mfcc(p, p, 1, 5, p, p, None, p, None) == -1
    assert lib.tcdiff_music_hpss(p, p, 1, 2047, p, p, p, p, p, p, p, None) == -1
    assert lib.tcdiff_music_hpss(p, p, 1, 4096, p, p, p, p, p, None, p, None) == -1          # percussive is not optional
    assert lib.tcdiff_music_onset(p, p, 1, 4, p, p, p, p, None) == -1 and lib.tcdiff_music_onset(p, None, 1, 5, p, p, p, p, None) == -1
    hdr = open(os.path.join(ROOT, "include", "tcdiff_hip.h")).read()
    for name, val in (("N_FFT", MU.N_FFT), ("HOP", MU.HOP), ("N_MELS", MU.N_MELS), ("N_MFCC", MU.N_MFCC), ("TEMPO_WIN", MU.TEMPO_WIN),
                      ("COLS", MU.N_COLS)):
        assert f"#define TC_MUSIC_{name} {val}" in hdr


def test_assemble_cond_layout():
    B, T = 2, 6
    feats = torch.arange(B * T * 425, dtype=torch.float32).reshape(B, T, 425)
    chroma = -torch.arange(1, B * T * 12 + 1, dtype=torch.float32).reshape(B, T, 12)
    beat = (torch.arange(B * T).reshape(B, T) % 4 < 2).float()
    cond = MU.assemble_cond(feats, chroma, beat)
    assert cond.shape == (B, T, 438) and MU.ONSET_BEAT == M.ONSET_BEAT == 53 and MU.COND_COLS == 438
    assert torch.equal(cond[..., :40], feats[..., :40]) and torch.equal(cond[..., 40:52], chroma)
    assert torch.equal(cond[..., 52], feats[..., 40]) and torch.equal(cond[..., M.ONSET_BEAT], beat)
    assert torch.equal(cond[..., 54:], feats[..., 41:])
    assert torch.equal(M.beats_from_cond(cond, T // 2), beat[:, ::2].to(torch.uint8))
    for args in ((feats[..., :424], chroma, beat), (feats, chroma[..., :11], beat), (feats, chroma, beat[:, :5]),
                 (feats.double(), chroma, beat), (feats, chroma, beat[..., None]), (feats, None, beat), (feats[0], chroma[0], beat[0])):
        with pytest.raises(L.TcdiffError):
            MU.assemble_cond(*args)
    with pytest.raises(TypeError):                        # both missing parts are required arguments
        MU.assemble_cond(feats)
