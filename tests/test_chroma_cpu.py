"""tests/chroma_ref.py pinned without a GPU: the resampler's taps, the shared filter basis, the properties of librosa's path the
kernels rely on (no early downsampling, seven octaves on one basis), what the restatement says about plain tones, the margins of
its tuning decisions on the clips of tests/test_chroma_gpu.py, and the host side of tcdiff_amd.music (tables, argument checks)."""
import numpy as np
import pytest
import scipy.signal
import torch

import chroma_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import music as MU


def test_taps_are_symmetric_with_unit_dc_gain():
    h = R.resample_taps()
    assert h.shape == (63,) and np.array_equal(h, h[::-1])
    # 0.85 sinc(0.85 x) integrates to 1; sampled every half unit and halved it sums to 1 up to the Kaiser window's ripple, so a
    # stage (which also restores the power lost to the decimation) has DC gain sqrt(2)
    assert abs(h.sum() * np.sqrt(2.0) - np.sqrt(2.0)) < 1e-4
    assert abs(R.resample_table()[0] - 0.85) < 1e-15 and len(R.resample_table()) == 8193


@pytest.mark.parametrize("n", [200, 201])
def test_one_stage_is_upfirdn(n):
    x = np.random.default_rng(n).standard_normal(n)
    # upfirdn's output m is sum_k h[k] x'[2 m - k]; with one zero in front of x and the taps symmetric that is y[m - 16] / sqrt(2)
    full = scipy.signal.upfirdn(R.resample_taps(), np.concatenate([[0.0], x]), down=2)
    want = np.sqrt(2.0) * full[16:16 + (n + 1) // 2]
    got = R.resample_stage(x)
    assert got.shape == ((n + 1) // 2,) and np.abs(got - want).max() < 1e-14


@pytest.mark.parametrize("k", [0, 37, 50, 99])
def test_every_octave_has_the_top_octaves_basis(k):
    tuning = R.EDGES[k]
    top = R.octave_basis_dense(R.octave_freqs(tuning, 0), R.SR)
    for i in range(1, R.N_OCT):
        own = R.octave_basis_dense(R.octave_freqs(tuning, i), R.SR / 2 ** i)
        assert np.abs(own - top).max() <= 1e-13 * np.abs(top).max(), i
    assert np.array_equal(R.basis(k), top.astype(np.complex64))
    # the longest filter needs the 1024-point frame, and one of half the length would not do
    lens = R.cqt_lengths(tuning)[-R.BPO:]
    assert 512 < np.ceil(lens.max()) <= 1024


@pytest.mark.parametrize("k", [0, 50, 99])
def test_sparsification_drops_less_than_a_hundredth(k):
    dense = R.octave_basis_dense(R.octave_freqs(R.EDGES[k]), R.SR, sparse=False)
    kept = R.octave_basis_dense(R.octave_freqs(R.EDGES[k]), R.SR)
    lost = (np.abs(dense) - np.abs(kept)).sum(axis=1) / np.abs(dense).sum(axis=1)
    assert (lost < 0.01).all() and (lost > 0).all()
    nz = kept != 0
    assert ((R.N_FFT // 2 + 1 - nz[:, ::-1].argmax(1)) - nz.argmax(1)).max() <= L.CHROMA_BAND


def test_no_early_downsampling_at_any_tuning():
    assert [R.early_downsample_count(t) for t in R.EDGES[:-1]] == [0] * R.N_TUNINGS


def test_a_pure_c_gives_chroma_zero():
    y = R.make_tone(512 * 20, R.FMIN0 * 8)
    for k in (None, 50):
        out = R.chroma_cqt(y, k)
        assert out["chroma"].shape == (21, 12) and (out["chroma"].argmax(axis=1) == 0).all()
        assert (out["chroma"].max(axis=1) == 1.0).all()


def test_a_detuned_tone_is_found():
    """A7 raised by 0.235 bin: cell 73 is [0.23, 0.24); piptrack's parabola on a Hann peak reads this tone some 0.007 bin sharp, so
    the restatement (as librosa would) lands one cell up"""
    y = R.make_tone(512 * 20, 3520.0 * 2.0 ** (0.235 / 36.0))
    k, info = R.tuning_index(y)
    assert k in (73, 74) and info["margin"] > 0, (k, info)
    k32, _ = R.tuning_index(y, np.float32)
    assert k32 == k


def test_frame_count_when_the_octaves_disagree():
    n = 4095
    assert R.octave_frames(n, 0) == 8 and R.octave_frames((n + 1) // 2, 1) == 9
    out = R.chroma_cqt(R.make_tone(n, 440.0), 50)
    assert out["chroma"].shape == (8, 12) and out["cqt_mag"].shape == (8, 252)
    assert [len(p) for p in out["pyramid"]] == [2048, 1024, 512, 256, 128, 64]


@pytest.mark.parametrize("case", list(R.GPU_CASES))
def test_margins_of_the_gpu_cases_are_positive(case):
    n, seeds = R.GPU_CASES[case]
    for seed in seeds:
        k, info = R.tuning_index(R.case_clip(n, seed))
        print(f"chroma case {case} seed {seed}: index {k} margin {info['margin']} pitches {info['n_pitches']}")
        assert info["margin"] > 0, (case, seed, info)
        assert (k == 50 and info["n_pitches"] == 0) if seed is None else info["n_pitches"] > 0


def test_host_tables_match_the_restatement():
    assert np.abs(MU.resample_taps() - R.resample_taps()).max() < 1e-15
    cq = MU.cqt_basis(R.SR)
    assert cq["basis"].shape == (100, 36, L.CHROMA_BAND) and cq["band"].shape == (100, 36, 2) and cq["scale"].shape == (100, 252)
    for k in range(R.N_TUNINGS):
        want = R.basis(k)
        dense = np.zeros(want.shape, np.complex128)
        for r in range(R.BPO):
            lo, hi = cq["band"][k, r]
            assert 0 <= lo < hi <= 513 and hi - lo <= L.CHROMA_BAND and want[r, lo] != 0 and want[r, hi - 1] != 0
            dense[r, lo:hi] = cq["basis"][k, r, :hi - lo]
            assert (cq["basis"][k, r, hi - lo:] == 0).all()
        assert np.abs(dense - want).max() <= 2.0 ** -23 * np.abs(want).max()          # both are rounded to complex64
        scale = np.sqrt(2.0 ** (R.N_OCT - 1 - np.arange(R.N_BINS) // R.BPO)) / np.sqrt(R.cqt_lengths(R.EDGES[k]))
        assert np.abs(cq["scale"][k] - scale).max() <= 1e-15
    assert np.array_equal(MU.TUNINGS, R.EDGES)


def test_unsupported_rate_raises():
    with pytest.raises(L.TcdiffError, match="not supported"):
        MU.cqt_basis(8000)


def test_given_tuning_is_validated():
    y = torch.zeros(2, 4096)
    for bad in (0.5, -0.51, 0.123, float("nan"), "x", [0.0], [0.0, 0.1, 0.2]):
        with pytest.raises(L.TcdiffError, match="tuning"):
            MU.chroma_cqt(y, tuning=bad)
    for bad in (torch.tensor([0.0, 0.123]), torch.zeros(2, 1), torch.zeros(3)):
        with pytest.raises(L.TcdiffError, match="tuning"):
            MU.chroma_cqt(y, tuning=bad)
    for good in (0.0, -0.5, 0.49, 0.12 + 1e-12, [0.1, -0.2], np.float32(0.25), torch.tensor([0.1, -0.2], dtype=torch.float64),
                 torch.tensor(0.25)):      # past the check: stopped for want of a GPU
        with pytest.raises(L.TcdiffError, match="MI355X"):
            MU.chroma_cqt(y, tuning=good)
    assert MU._tuning_indices(0.12 + 1e-12, 1) == [62] and MU._tuning_indices([-0.5, 0.49], 2) == [0, 99]
    assert MU._tuning_indices(torch.tensor([-0.5, 0.49], dtype=torch.float64), 2) == [0, 99]


def test_argument_checks_and_no_cpu_fallback():
    for fn in (MU.chroma_cqt, MU.estimate_tuning):
        with pytest.raises(L.TcdiffError, match="at least 2048"):
            fn(torch.zeros(2047))
        with pytest.raises(L.TcdiffError, match="float32"):
            fn(torch.zeros(4096, dtype=torch.float64))
        with pytest.raises(L.TcdiffError, match="contiguous"):
            fn(torch.zeros(2, 8192)[:, ::2])
        with pytest.raises(L.TcdiffError, match=r"\(n,\) or \(B, n\)"):
            fn(torch.zeros(1, 2, 4096))
        with pytest.raises(L.TcdiffError, match="MI355X"):
            fn(torch.zeros(4096))
    with pytest.raises(L.TcdiffError, match="MI355X"):
        MU.music_cond(torch.zeros(4096))
    with pytest.raises(L.TcdiffError, match="MI355X"):
        MU.music_cond(torch.zeros(4096), torch.zeros(1, 9, 12))
