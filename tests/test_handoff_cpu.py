"""The Navigator -> sampler hand-off, host side (no GPU): the gains `navigator.smooth_x0` sends to the device are exactly the K of
io.kalman_smooth_batch's loop, that loop's results are what the per-trajectory restatement gives (atol = 0), the layout contract
the GPU tests use is io.x0_from_navigator's, the launcher is exported and validates before it launches, and the new entry points
refuse to run off-GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handoff_ref as HR  # noqa: E402
from tcdiff_amd import io as IO  # noqa: E402
from tcdiff_amd import navigator as N  # noqa: E402
from tcdiff_amd._lib import TcdiffError  # noqa: E402

PARAMS = [dict(), dict(dt=0.5, process_noise_std=0.1, measurement_noise_std=0.3)]


def _loop_args(kw):
    return kw.get("dt", 1.0), kw.get("process_noise_std", 1e-2), kw.get("measurement_noise_std", 1e-1)


@pytest.mark.parametrize("kw", PARAMS, ids=["default", "other"])
def test_gains_are_the_loops_gains_and_the_batched_filter_is_unchanged(kw):
    """io.kalman_gains(frames) == the K of every frame of the per-trajectory loop, and io.kalman_smooth_batch == that loop's
    filtered positions, both with atol = 0 on float64: the gains function restates the covariance recursion without changing it,
    and the batched filter computes what it computed before the gains were factored out beside it."""
    xy = HR.walks(3, 2, 151, seed=1).astype(np.float64)
    want, gains = HR.kalman_loop(xy, *_loop_args(kw))
    got = IO.kalman_gains(151, **kw)
    assert got.shape == (151, 4, 2) and got.dtype == np.float64
    assert np.array_equal(got, gains)
    for frames in (1, 2, 3):                                   # a shorter table is a prefix
        assert np.array_equal(IO.kalman_gains(frames, **kw), gains[:frames])
    sm = IO.kalman_smooth_batch(xy, **kw)
    assert sm.dtype == np.float64 and np.array_equal(sm, want)
    assert abs(got[0, 0, 0] - 1.0) < 1e-2 and got[0, 0, 0] != 1.0          # first frame: gain ~ 1 (P0 = 10 >> R), not 1


def test_layout_restatement_is_x0_from_navigator():
    """x_0[c, f * dn + d] = (sx, sy, 0): the numpy restatement the GPU tests compare with, against io.x0_from_navigator on a CPU
    tensor (float64 recursion rounded once to the tensor's float32)"""
    xy = HR.walks(3, 2, 40, seed=2)
    want = HR.want_x0(xy)
    assert want.dtype == np.float64 and want.shape == (3, 80, 3)
    x0 = IO.x0_from_navigator(torch.from_numpy(xy))
    assert x0.dtype == torch.float32 and np.array_equal(x0.numpy(), want.astype(np.float32))
    ok, worst = HR.within_bound(x0.numpy(), want)
    assert ok and worst <= 1.0
    ok, _ = HR.within_bound(np.nextafter(x0.numpy(), np.float32(np.inf)), want)      # one float32 ulp off is outside the bound
    assert not ok
    dancer_major = np.zeros((3, 80, 3), dtype=np.float32)                             # token d * frames + f: the wrong order
    dancer_major[..., :2] = IO.kalman_smooth_batch(xy).reshape(3, 80, 2)
    assert not HR.within_bound(dancer_major, want)[0]


def test_launcher_is_exported_and_validates_before_any_launch():
    import ctypes
    from tcdiff_amd import _lib as L
    from tcdiff_amd import build
    build.build(verbose=False)
    lib = L.load()
    assert hasattr(lib, "tcdiff_nav_handoff") and "tcdiff_nav_handoff" in L.EXPORTS
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    three = (ctypes.c_float * 3)(1, 1, 1)
    f = lib.tcdiff_nav_handoff
    assert f(None, 2, 2, 2, 1, 1, 1, 1, 1.0, p, None, None, p, p, None) == -1           # no input
    assert f(p, 2, 2, 2, 1, 1, 1, 1, 1.0, None, None, None, p, p, None) == -1           # no gains
    assert f(p, 2, 2, 2, 1, 1, 1, 1, 1.0, p, None, None, None, None, None) == -1        # no output
    assert f(p, 2, 2, 2, 1, 0, 1, 1, 1.0, p, None, None, p, p, None) == -1              # b < 1
    assert f(p, 2, 2, 2, 1, 1, 1, 0, 1.0, p, None, None, p, p, None) == -1              # frames < 1
    assert f(p, 2, 2, 2, 1, 1, 1, 1, 1.0, p, three, None, p, p, None) == -1             # scale without min_


def test_no_cpu_fallback():
    from tcdiff_amd import TrajDecoder
    with pytest.raises(TcdiffError):
        N.smooth_x0(torch.zeros(2, 3, 5, 2))
    with pytest.raises(TcdiffError):
        N.smooth_x0(torch.zeros(2, 3, 5, 2, dtype=torch.float64))
    with pytest.raises(TcdiffError):
        N.smooth_x0(torch.zeros(2, 3, 5))
    m = TrajDecoder(nfeats=2, trans_layer=2, window_size=20)
    with pytest.raises(TcdiffError):
        N.rollout_x0(m, torch.zeros(1, 2, 20, 2), torch.zeros(1, 61, 438), step=5)
