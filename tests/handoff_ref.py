"""Reference for the Navigator -> sampler hand-off tests (tcdiff_amd.navigator.smooth_x0 / rollout_x0, csrc/handoff.hip): the
per-trajectory Kalman loop written out from the description in tcdiff_amd/io.py, the layout contract of x_0 in numpy, the
yardstick and the bound.

Yardstick: io.kalman_smooth_batch fed float64 (it returns float64; tests/test_io_cpu.py holds it to the per-trajectory loop).
Bound, derived: the kernel runs the same float64 recursion, possibly in another summation order (~1e-16 relative), and rounds
once to float32 (half an ulp: 2^-24 relative), so per element |got - want64| <= 2^-24 |want64| (1 + 2^-20) + 1e-12."""
import numpy as np

from tcdiff_amd import io as IO


def kalman_loop(xy, dt=1.0, q=1e-2, r=1e-1):
    """One trajectory at a time: predict, update (Joseph form), in float64.  xy (b, dn, frames, 2) -> (filtered positions of the
    same shape as float64, the gains of the last trajectory (frames, 4, 2))."""
    xy = np.asarray(xy, dtype=np.float64)
    out = np.zeros_like(xy)
    gains = np.zeros((xy.shape[2], 4, 2))
    F = np.array([[1, 0, dt, 0], [0, 1, 0, dt], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    H = np.array([[1, 0, 0, 0], [0, 1, 0, 0.0]])
    R, Q = np.eye(2) * r ** 2, np.eye(4) * q
    for b in range(xy.shape[0]):
        for d in range(xy.shape[1]):
            P = np.eye(4) * 10.0
            x = np.array([xy[b, d, 0, 0], xy[b, d, 0, 1], 0.0, 0.0])
            for t in range(xy.shape[2]):
                x = F @ x
                P = F @ P @ F.T + Q
                y = xy[b, d, t] - H @ x
                PHT = P @ H.T
                S = H @ PHT + R
                K = PHT @ np.linalg.inv(S)
                x = x + K @ y
                I_KH = np.eye(4) - K @ H
                P = I_KH @ P @ I_KH.T + K @ R @ K.T
                out[b, d, t] = x[:2]
                gains[t] = K
    return out, gains


def x0_layout(sm, z=0.0):
    """(b, dn, frames, 2) -> (b, frames * dn, 3): x_0[c, f * dn + d] = (sx, sy, z), written element by element"""
    sm = np.asarray(sm)
    b, dn, frames, _ = sm.shape
    out = np.empty((b, frames * dn, 3), dtype=sm.dtype)
    for c in range(b):
        for f in range(frames):
            for d in range(dn):
                out[c, f * dn + d] = (sm[c, d, f, 0], sm[c, d, f, 1], z)
    return out


def want_x0(xy32, **kw):
    """the yardstick for an fp32 input (numpy, (b, dn, frames, 2)): float64 x_0"""
    return x0_layout(IO.kalman_smooth_batch(np.asarray(xy32, dtype=np.float64), **kw))


def within_bound(got32, want64):
    """-> (ok, worst ratio |got - want| / bound) over EVERY element"""
    got = np.asarray(got32, dtype=np.float64)
    bound = 2.0 ** -24 * np.abs(want64) * (1.0 + 2.0 ** -20) + 1e-12
    ratio = np.abs(got - want64) / bound
    return bool(np.all(np.isfinite(got)) and np.all(ratio <= 1.0)), float(ratio.max())


def walks(b, dn, frames, seed, step=0.02, noise=0.05):
    """Distinct noisy random walks per trajectory, a different offset per dancer and per clip (a swapped axis cannot pass): fp32"""
    rng = np.random.default_rng(seed)
    w = rng.normal(0, step, (b, dn, frames, 2)).cumsum(axis=2) + rng.normal(0, noise, (b, dn, frames, 2))
    w += 0.3 * np.arange(dn)[None, :, None, None] - 0.11 * np.arange(b)[:, None, None, None]
    w[..., 1] -= 0.05
    return w.astype(np.float32)
