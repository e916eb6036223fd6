"""csrc/chroma.hip and tcdiff_amd.music.chroma_cqt on an MI355X against the float64 run of the restatement tests/chroma_ref.py, on
every output, the ``return_parts`` ones included, no element left out.

Bound.  The rule of tests/test_music_gpu.py, margin included: the kernels compute in fp32, as librosa does, so the yardstick is the
restatement's own float32 run (at the float64 run's tuning); per output and clip, with d32 = max |ref_f32 - ref_f64|,

    max |kernel - ref_f64| <= 32 max(d32, 2^-23 max |ref_f64|).

The observed error / max(d32, floor) of every output and clip is printed before it is asserted (recorded in profiles/chroma.txt).

Tuning.  ``tuning_index`` is an integer decision: it must equal the restatement's wherever the restatement's margin is positive
(chroma_ref.tuning_index), which tests/test_chroma_cpu.py asserts for every clip used here, so it is asserted again and no clip is
let off.

Cases (chroma_ref.GPU_CASES): A 2048 samples (5 frames, every octave-6 frame mostly padding), B 4095 samples (the octaves disagree
on the frame count; odd lengths all the way down the pyramid), C three clips of 40 frames and 137 samples at once through a wider
row stride, the middle one silent."""
import numpy as np
import pytest
import torch

import chroma_ref as R
import music_ref as MR
from tcdiff_amd import music as MU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 32.0
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _ref(n, seed):
    """(signal, float64 outputs, float32 outputs at the same tuning), computed once and left unchanged"""
    def make():
        y = R.case_clip(n, seed)
        r64 = R.chroma_cqt(y)
        return y, r64, R.chroma_cqt(y, r64["tuning_index"], dtype=np.float32)
    return _once(("ref", n, seed), make)


def _run(Y, **kw):
    chroma, parts = MU.chroma_cqt(Y, return_parts=True, **kw)
    torch.cuda.synchronize()
    return chroma, parts


def _outputs(chroma, parts, b):
    out = dict(chroma=chroma[b].cpu().numpy(), cqt_mag=parts["cqt_mag"][b].cpu().numpy())
    out.update({f"pyramid{s + 1}": p[b].cpu().numpy() for s, p in enumerate(parts["pyramid"])})
    return out


def _want(r):
    out = dict(chroma=r["chroma"], cqt_mag=r["cqt_mag"])
    out.update({f"pyramid{s + 1}": p for s, p in enumerate(r["pyramid"])})
    return out


def _check(case, out, r64, r32):
    failed = []
    w64, w32 = _want(r64), _want(r32)
    assert set(out) == set(w64)
    for name, got in out.items():
        want, want32 = w64[name], w32[name]
        assert got.dtype == np.float32 and got.shape == want.shape, (case, name, got.shape, want.shape)
        assert want32.dtype == np.float32 and want.dtype == np.float64
        assert np.isfinite(got).all(), (case, name)
        d32 = float(np.abs(want32.astype(np.float64) - want).max())
        unit = max(d32, 2.0 ** -23 * float(np.abs(want).max()))
        err = float(np.abs(got.astype(np.float64) - want).max())
        ratio = err / unit if unit > 0 else (0.0 if err == 0 else float("inf"))
        print(f"chroma case {case} {name:9s} err {err:.3e} d32 {d32:.3e} unit {unit:.3e} ratio {ratio:.2f}")
        if not err <= FACTOR * unit:
            failed.append((name, err, unit))
    assert not failed, (case, failed)


def _check_tuning(case, got, r64):
    info = r64["info"]
    print(f"chroma case {case} tuning_index {got} reference {r64['tuning_index']} margin {info['margin']} pitches {info['n_pitches']}")
    assert info["margin"] > 0, (case, info)              # (tests/test_chroma_cpu.py asserts the same: no clip is let off)
    assert got == r64["tuning_index"], (case, got, r64["tuning_index"], info)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", ["A", "B"])
def test_single_clip_against_float64(case):
    n, (seed,) = R.GPU_CASES[case]
    y, r64, r32 = _ref(n, seed)
    chroma, parts = _once(("run", case), lambda: _run(torch.from_numpy(y).to(DEV)))
    T = 1 + n // 512
    assert chroma.shape == (1, T, 12) and chroma.dtype == torch.float32 and chroma.is_cuda
    assert parts["cqt_mag"].shape == (1, T, 252) and parts["tuning_index"].shape == (1,) and parts["tuning_index"].dtype == torch.int32
    assert [tuple(p.shape) for p in parts["pyramid"]] == [(1, -(-n // 2 ** s)) for s in range(1, 7)]
    _check_tuning(case, int(parts["tuning_index"][0]), r64)
    _check(case, _outputs(chroma, parts, 0), r64, r32)
    assert float(chroma.max()) == 1.0


def _batch():
    """the three clips of case C as a view into a wider buffer"""
    n, seeds = R.GPU_CASES["C"]
    ys = [R.case_clip(n, s) for s in seeds]
    wide = torch.full((3, n + 37), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :n] = torch.from_numpy(np.stack(ys)).to(DEV)
    view = wide[:, :n]
    assert not view.is_contiguous()
    return n, seeds, view


def _batch_run():
    return _once(("run", "C"), lambda: _run(_batch()[2]))


def test_batch_through_a_row_stride_against_float64():
    n, seeds, view = _batch()
    chroma, parts = _batch_run()
    assert chroma.shape == (3, 41, 12) and parts["cqt_mag"].shape == (3, 41, 252)
    for b, seed in enumerate(seeds):
        y, r64, r32 = _ref(n, seed)
        _check_tuning(f"C{b}", int(parts["tuning_index"][b]), r64)
        if seed is not None:
            _check(f"C{b}", _outputs(chroma, parts, b), r64, r32)
    # silence: tuning 0.0, and the frames of zeros are left undivided
    assert int(parts["tuning_index"][1]) == 50
    assert (chroma[1] == 0).all() and (parts["cqt_mag"][1] == 0).all() and all((p[1] == 0).all() for p in parts["pyramid"])
    assert not torch.isnan(chroma).any()
    idx, tp = MU.estimate_tuning(view, return_parts=True)
    assert torch.equal(idx, parts["tuning_index"]) and int(tp["n_pitches"][1]) == 0 and int(tp["counts"][1].sum()) == 0
    for b, seed in enumerate(seeds):
        if seed is not None:
            info = _ref(n, seed)[1]["info"]
            print(f"chroma case C{b} n_pitches {int(tp['n_pitches'][b])} reference {info['n_pitches']} "
                  f"threshold {float(tp['threshold'][b]):.6e} reference {info['threshold']:.6e}")
            assert int(tp["counts"][b].argmax()) == int(idx[b]) and int(tp["counts"][b].sum()) > 0
            # no piptrack flag of the reference is within its guard of flipping, so the pitch count is binding too.  With the
            # same pitches the median, an order statistic, moves by no more than the largest change of any magnitude: the
            # STFT's S is held to some 1e-6 of its maximum (tests/test_music_gpu.py) and dskew = avg^2 / (2 den) to a few times
            # that; the threshold is about 0.7 of the maximum, so 1e-4 of it leaves a factor of ten or more
            assert info["unsure_flags"] == 0 and int(tp["n_pitches"][b]) == info["n_pitches"]
            assert abs(float(tp["threshold"][b]) - info["threshold"]) <= 1e-4 * info["threshold"]


def test_given_tuning_reproduces_the_estimate():
    n, seeds, view = _batch()
    chroma, parts = _batch_run()
    given = [float(MU.TUNINGS[int(k)]) for k in parts["tuning_index"].cpu()]
    c2, p2 = _run(view, tuning=given)
    _same(c2, chroma)
    _same(p2["cqt_mag"], parts["cqt_mag"])
    assert torch.equal(p2["tuning_index"], parts["tuning_index"])
    c4, _ = _run(view, tuning=torch.tensor(given, dtype=torch.float64, device=DEV))       # a tensor is read once
    _same(c4, chroma)
    c3, p3 = _run(view[0], tuning=given[0])
    _same(c3[0], chroma[0])
    other, _ = _run(view[0], tuning=-0.5 if given[0] != -0.5 else 0.49)       # (another tuning is another basis)
    assert not torch.equal(other[0], chroma[0])


def test_clip_alone_and_second_run_give_the_same_bits():
    n, seeds, view = _batch()
    chroma, parts = _batch_run()
    for b in range(3):
        c1, p1 = _run(view[b].contiguous())
        _same(c1[0], chroma[b])
        _same(p1["cqt_mag"][0], parts["cqt_mag"][b])
        assert int(p1["tuning_index"][0]) == int(parts["tuning_index"][b])
        for a, p in zip(p1["pyramid"], parts["pyramid"]):
            _same(a[0], p[b])
    c2, p2 = _run(view)
    _same(c2, chroma)
    _same(p2["cqt_mag"], parts["cqt_mag"])
    for a, p in zip(p2["pyramid"], parts["pyramid"]):
        _same(a.contiguous(), p.contiguous())
    _same(MU.chroma_cqt(view), chroma)                    # without the parts: the same chroma


def test_music_cond_computes_or_takes_the_chroma():
    n = 12 * 512 + 137
    Y = torch.from_numpy(np.stack([MR.make_signal(n, seed=2), MR.make_signal(n, seed=6)])).to(DEV)
    feats, parts = MU.music_features(Y, return_parts=True)
    _, onset_beat = MU.beat_track(parts["onset_env"])
    chroma = MU.chroma_cqt(parts["harmonic"])
    cond = MU.music_cond(Y)
    assert cond.shape == (2, 13, 438) and cond.dtype == torch.float32
    _same(cond[..., 40:52].contiguous(), chroma)
    assert torch.isfinite(chroma).all() and float(chroma.max()) == 1.0 and float(chroma.min()) >= 0.0
    _same(cond, MU.assemble_cond(feats, chroma, onset_beat))
    g = torch.Generator().manual_seed(0)
    mine = torch.rand(2, 13, 12, generator=g).to(DEV)
    _same(MU.music_cond(Y, mine), MU.assemble_cond(feats, mine, onset_beat))
