"""The float64 restatement of include/tcdiff_choreo.h in numpy and plain Python floats (IEEE doubles, one rounding an operation, in
the header's operation order), for tests/test_choreo_cpu.py and tests/test_choreo_gpu.py.  Written from the header, with none of the
kernels' tiles or trees: a loop over the keys, a loop over the frames."""
import numpy as np

NAN = float("nan")


def sign(v):
    return (v > 0.0) - (v < 0.0)


def slopes(key, y):
    """the PCHIP slopes at the keys (ints, strictly ascending) of the values y (floats): a list of floats"""
    n = len(key)
    key, y = [int(k) for k in key], [float(v) for v in y]
    if n == 1:
        return [0.0]
    h = [float(key[k + 1] - key[k]) for k in range(n - 1)]
    m = [(y[k + 1] - y[k]) / h[k] for k in range(n - 1)]
    if n == 2:
        return [m[0], m[0]]

    def end(h0, h1, m0, m1):
        d = ((2.0 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
        if sign(d) != sign(m0):
            return 0.0
        if sign(m0) != sign(m1) and abs(d) > 3.0 * abs(m0):
            return 3.0 * m0
        return d

    d = [end(h[0], h[1], m[0], m[1])]
    for k in range(1, n - 1):
        if sign(m[k - 1]) != sign(m[k]) or m[k - 1] == 0.0 or m[k] == 0.0:
            d.append(0.0)
        else:
            w1, w2 = 2.0 * h[k] + h[k - 1], h[k] + 2.0 * h[k - 1]
            d.append((w1 + w2) / (w1 / m[k - 1] + w2 / m[k]))
    d.append(end(h[n - 2], h[n - 3], m[n - 2], m[n - 3]))
    return d


def evaluate(key, y, d, t):
    """one component at frame t, a float"""
    n = len(key)
    if t <= key[0]:
        return float(y[0])
    if t >= key[n - 1]:
        return float(y[n - 1])
    k = max(i for i in range(n) if key[i] <= t)
    h = float(int(key[k + 1]) - int(key[k]))
    s = float(int(t) - int(key[k])) / h
    u = 1.0 - s
    h00, h10, h01, h11 = ((1.0 + 2.0 * s) * u) * u, (s * u) * u, (s * s) * (3.0 - 2.0 * s), (s * s) * (s - 1.0)
    return (h00 * float(y[k]) + h10 * (h * d[k])) + (h01 * float(y[k + 1]) + h11 * (h * d[k + 1]))


def path64(key, pts, frames):
    """key (n,) ints, pts (n, 2) float32 -> (frames, 2) float64: the unrounded path of one dancer"""
    pts = np.asarray(pts, np.float32).astype(np.float64)
    out = np.empty((frames, 2))
    for c in range(2):
        d = slopes(key, pts[:, c])
        for t in range(frames):
            out[t, c] = evaluate(key, pts[:, c], d, t)
    return out


def lane_sum(terms):
    """terms[t] (NaN or inf: left out) summed in the lane order: lane t % 64 in ascending t to 0.0, the lanes in ascending order to 0.0"""
    lanes = [0.0] * 64
    for t, v in enumerate(terms):
        if np.isfinite(v):
            lanes[t % 64] = lanes[t % 64] + float(v)
    tot = 0.0
    for l in range(64):
        tot = tot + lanes[l]
    return tot


def dist(a, b):
    """the floor distance of the float32 rows a, b (..., 2), float64"""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    dx, dy = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(dx * dx + dy * dy)


def largest(v):
    """(value, frame) of the largest finite v, the lower frame on a tie; (NaN, -1) without one"""
    best = (NAN, -1)
    for t, x in enumerate(v):
        if np.isfinite(x) and (best[1] < 0 or x > best[0]):
            best = (float(x), t)
    return best


def smallest(v):
    best = (NAN, -1)
    for t, x in enumerate(v):
        if np.isfinite(x) and (best[1] < 0 or x < best[0]):
            best = (float(x), t)
    return best


def pairs(dn):
    return [(i, j) for i in range(dn) for j in range(i + 1, dn)]


def status_of(key, pts, count, K, frames):
    if not 1 <= count <= K:
        return 1
    key = [int(k) for k in key[:count]]
    if any(k < 0 or k >= frames for k in key) or any(key[i] <= key[i - 1] for i in range(1, count)):
        return 1
    return 0 if np.isfinite(np.asarray(pts[:count], np.float64)).all() else 2


def plan(keys, points, frames, counts=None, fps=30.0, scale=None, min_=None, min_distance=0.5, max_speed=3.0):
    """keys (K,) or (b, dn, K) ints, points (b, dn, K, 2) float32, scale / min_ two float32 each or None -> dict of numpy arrays named
    as tcdiff_amd.choreo.Plan's fields, and traj64, the unrounded path"""
    points = np.asarray(points, np.float32)
    keys = np.asarray(keys)
    b, dn, K, _ = points.shape
    P = len(pairs(dn))
    out = dict(traj=np.empty((b, dn, frames, 2), np.float32), traj64=np.empty((b, dn, frames, 2)), x_0=np.zeros((b, frames * dn, 3), np.float32),
               status=np.zeros((b, dn), np.int32), clamped=np.zeros((b, dn), np.int32), speed_max=np.empty((b, dn)),
               speed_peak=np.empty((b, dn), np.int32), too_fast=np.zeros((b, dn), np.int32), path_length=np.empty((b, dn)),
               dist_min=np.empty((b, P)), dist_min_frame=np.empty((b, P), np.int32), too_close=np.empty((b, P), np.int32))
    x0 = out["x_0"].reshape(b, frames, dn, 3)
    if scale is not None:
        scale, min_ = [float(np.float32(v)) for v in scale], [float(np.float32(v)) for v in min_]
    for c in range(b):
        for d in range(dn):
            n = K if counts is None else int(counts[c][d])
            key = keys if keys.ndim == 1 else keys[c, d]
            st = out["status"][c, d] = status_of(key, points[c, d], n, K, frames)
            if st:
                out["traj"][c, d] = out["traj64"][c, d] = x0[c, :, d, :2] = NAN
                out["speed_max"][c, d] = out["path_length"][c, d] = NAN
                out["speed_peak"][c, d] = -1
                continue
            v = out["traj64"][c, d] = path64(key[:n], points[c, d, :n], frames)
            with np.errstate(over="ignore"):
                f = out["traj"][c, d] = v.astype(np.float32)
            if scale is None:
                x0[c, :, d, :2] = f
            else:
                hit = np.zeros(frames, bool)
                for ch in range(2):
                    nrm = v[:, ch] * scale[ch] + min_[ch]
                    hit |= (nrm < -1.0) | (nrm > 1.0)
                    x0[c, :, d, ch] = np.where(nrm < -1.0, -1.0, np.where(nrm > 1.0, 1.0, nrm)).astype(np.float32)
                out["clamped"][c, d] = hit.sum()
            step = dist(f[:-1], f[1:])
            speed = step * float(fps)
            out["speed_max"][c, d], out["speed_peak"][c, d] = largest(speed)
            out["too_fast"][c, d] = int((np.isfinite(step) & (speed > max_speed)).sum())
            out["path_length"][c, d] = lane_sum(step)
        for p, (i, j) in enumerate(pairs(dn)):
            dd = dist(out["traj"][c, i], out["traj"][c, j])
            out["dist_min"][c, p], out["dist_min_frame"][c, p] = smallest(dd)
            out["too_close"][c, p] = int((np.isfinite(dd) & (dd < min_distance)).sum())
    return out


def trajectory_error(joints, traj, up=2):
    """joints (b, dn, T, 24, 3) float32, traj (b, dn, T, 2) float32 -> dict of (b, dn) arrays named as tcdiff_amd.choreo's"""
    joints, traj = np.asarray(joints, np.float32), np.asarray(traj, np.float32)
    b, dn, T = joints.shape[:3]
    axes = [a for a in range(3) if a != up]
    out = dict(traj_err_mean=np.empty((b, dn)), traj_err_max=np.empty((b, dn)), traj_err_final=np.empty((b, dn)),
               traj_err_peak=np.empty((b, dn), np.int32), traj_frames=np.empty((b, dn), np.int32))
    for c in range(b):
        for d in range(dn):
            e = dist(traj[c, d], joints[c, d, :, 0][:, axes])
            ok = np.isfinite(e)
            n = int(ok.sum())
            out["traj_frames"][c, d] = n
            out["traj_err_mean"][c, d] = lane_sum(e) / float(n) if n else NAN
            out["traj_err_max"][c, d], out["traj_err_peak"][c, d] = largest(e)
            out["traj_err_final"][c, d] = float(e[np.flatnonzero(ok)[-1]]) if n else NAN
    return out


# ---- the seeded cases of the tests -----------------------------------------------------------------------------------------------------
def keys_between(g, frames, n):
    """n strictly ascending keys with frame 0 and frame frames - 1 among them, unevenly spaced"""
    if n == 1:
        return np.array([0], np.int32)
    inner = g.choice(np.arange(1, frames - 1), size=n - 2, replace=False) if n > 2 else np.array([], np.int64)
    return np.sort(np.concatenate([[0, frames - 1], inner])).astype(np.int32)


def case(b, dn, frames, K, seed, per_dancer=False, short=True):
    """seeded waypoints within a few metres; with `short` (and K > 1) dancer 0 of clip 0 uses K - 1 keys and NaN fills its padding"""
    g = np.random.default_rng(seed)
    points = g.uniform(-3.0, 3.0, (b, dn, K, 2)).astype(np.float32)
    counts = np.full((b, dn), K, np.int32)
    if per_dancer:
        keys = np.stack([np.stack([keys_between(g, frames, K) for _ in range(dn)]) for _ in range(b)])
    else:
        keys = keys_between(g, frames, K)
    if short and K > 1:
        counts[0, 0] = K - 1
        points[0, 0, K - 1] = np.nan
    if K >= 4:                                                # a hold: two equal consecutive waypoints
        points[0, dn - 1, 2] = points[0, dn - 1, 1]
    return keys, points, counts
