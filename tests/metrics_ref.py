"""numpy float64 restatement of the four motion metrics of tcdiff_motion_metrics / tcdiff_amd/metrics.py, written from their
definitions (include/tcdiff_hip.h), and the seeded inputs the CPU and GPU tests share.  Inputs are float32 arrays, promoted
to float64 before the first operation."""
import numpy as np

FEET_PFC = (7, 10, 8, 11)          # EDGE: left ankle, left toe, right ankle, right toe
FEET_CONTACT = (7, 8, 10, 11)      # the contact channels' order
DEFAULTS = dict(fps=30, up=2, contact_threshold=0.95, still=0.01, radius=0.3, sigma_smooth=5.0, sigma_beat=3.0)


def _flat(up):
    return [k for k in range(3) if k != up]


def gaussian_weights(sigma):
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x * x)
    return w / w.sum(), r


def reflect_index(i, n):
    """(d c b a | a b c d | d c b a): period 2 n, whatever the distance from the array"""
    m = np.mod(i, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def smooth(v, sigma):
    """scipy.ndimage.gaussian_filter1d(v, sigma) with its defaults (mode "reflect", truncate 4)"""
    v = np.asarray(v, np.float64)
    n = v.shape[0]
    if n == 0:
        return v.copy()
    w, r = gaussian_weights(sigma)
    idx = reflect_index(np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :], n)
    return (v[idx] * w[None, :]).sum(-1)


def minima(s):
    """scipy.signal.argrelextrema(s, np.less)[0]: strict interior local minima"""
    s = np.asarray(s)
    if s.shape[0] < 3:
        return np.zeros(0, np.int64)
    return np.nonzero((s[1:-1] < s[:-2]) & (s[1:-1] < s[2:]))[0] + 1


def speed(J):
    """v[t] = mean_j |J[t + 1, j] - J[t, j]| of one dancer's (T, 24, 3) joints"""
    J = np.asarray(J, np.float64)
    return np.sqrt(((J[1:] - J[:-1]) ** 2).sum(-1)).mean(-1)


def pfc_one(J, fps, up):
    J = np.asarray(J, np.float64)
    T = J.shape[0]
    if T < 3:
        return np.nan
    dt = 1.0 / fps
    rv = (J[1:, 0] - J[:-1, 0]) / dt
    ra = (rv[1:] - rv[:-1]) / dt
    ra[:, up] = np.maximum(ra[:, up], 0.0)
    a = np.sqrt((ra ** 2).sum(-1))
    A = a.max()
    if A == 0:
        return 0.0
    F = J[:, list(FEET_PFC)][:, :, _flat(up)]
    fv = np.sqrt(((F[2:] - F[1:-1]) ** 2).sum(-1))                # (T - 2, 4)
    return float((np.minimum(fv[:, 0], fv[:, 1]) * np.minimum(fv[:, 2], fv[:, 3]) * (a / A)).mean())


def contact_one(J, C, thr, still):
    """(slide, break, frames) and the displacements / mask they come from"""
    J = np.asarray(J, np.float64)
    F = J[:, list(FEET_CONTACT)]
    delta = np.sqrt(((F[1:] - F[:-1]) ** 2).sum(-1))              # (T - 1, 4)
    mask = np.asarray(C, np.float64)[:-1] > thr
    n = int(mask.sum())
    if n == 0:
        return 0.0, 0.0, 0, delta, mask
    return float(delta[mask].mean()), float((delta[mask] >= still).sum() / n), n, delta, mask


def root_distances(Jc, up):
    """(pairs, T) root distance without the up axis, pairs in (d, e > d) order"""
    R = np.asarray(Jc, np.float64)[:, :, 0][:, :, _flat(up)]      # (dn, T, 2)
    dn = R.shape[0]
    out = [np.sqrt(((R[e] - R[d]) ** 2).sum(-1)) for d in range(dn) for e in range(d + 1, dn)]
    return np.stack(out) if out else np.zeros((0, R.shape[1]))


def beat_one(J, beats, sigma_smooth, sigma_beat):
    """(beat_align, |M|, s, M)"""
    s = smooth(speed(J), sigma_smooth)
    M = minima(s)
    B = np.nonzero(np.asarray(beats) != 0)[0]
    if len(M) == 0 or len(B) == 0:
        return np.nan, len(M), s, M
    d2 = ((B[:, None] - M[None, :]).astype(np.float64) ** 2).min(-1)
    return float(np.exp(-d2 / (2 * sigma_beat ** 2)).mean()), len(M), s, M


def metrics(joints, contacts=None, beats=None, **kw):
    p = dict(DEFAULTS, **kw)
    joints = np.asarray(joints)
    assert joints.dtype == np.float32
    b, dn, T = joints.shape[:3]
    out = {"pfc": np.zeros((b, dn)), "collision_rate": np.zeros(b)}
    if contacts is not None:
        out.update(contact_slide=np.zeros((b, dn)), contact_break=np.zeros((b, dn)), contact_frames=np.zeros((b, dn), np.int64))
    if beats is not None:
        out.update(beat_align=np.zeros((b, dn)), motion_beats=np.zeros((b, dn), np.int64))
    for c in range(b):
        dist = root_distances(joints[c], p["up"])
        out["collision_rate"][c] = (dist < p["radius"]).sum() / dist.size if dn > 1 else 0.0
        for d in range(dn):
            out["pfc"][c, d] = pfc_one(joints[c, d], p["fps"], p["up"])
            if contacts is not None:
                sl, br, n, _, _ = contact_one(joints[c, d], contacts[c, d], p["contact_threshold"], p["still"])
                out["contact_slide"][c, d], out["contact_break"][c, d], out["contact_frames"][c, d] = sl, br, n
            if beats is not None:
                ba, nm, _, _ = beat_one(joints[c, d], beats[c], p["sigma_smooth"], p["sigma_beat"])
                out["beat_align"][c, d], out["motion_beats"][c, d] = ba, nm
    return out


def decisions_clear(joints, contacts, beats, **kw):
    """No comparison the metrics make is a near-tie on these inputs, so an implementation that rounds differently in the last
    places still makes every decision the same way."""
    p = dict(DEFAULTS, **kw)
    joints, contacts = np.asarray(joints), np.asarray(contacts)
    b, dn, T = joints.shape[:3]
    if np.abs(contacts.astype(np.float64) - p["contact_threshold"]).min() <= 1e-6:
        return False
    for c in range(b):
        dist = root_distances(joints[c], p["up"])
        if dist.size and np.abs(dist - p["radius"]).min() <= 1e-9:
            return False
        for d in range(dn):
            _, _, _, delta, _ = contact_one(joints[c, d], contacts[c, d], p["contact_threshold"], p["still"])
            if delta.size and np.abs(delta - p["still"]).min() <= 1e-9:
                return False
            s = smooth(speed(joints[c, d]), p["sigma_smooth"])
            if s.shape[0] >= 2 and np.abs(s[1:] - s[:-1]).min() <= 1e-9 * s.max():      # every neighbouring pair, extrema included
                return False
    return True


def beats_from_cond_loop(cond, frames, long=False):
    """plain-loop restatement of tcdiff_amd.metrics.beats_from_cond on a numpy cond (b, n, 438)"""
    b = cond.shape[0]
    if not long:
        out = np.zeros((b, frames), np.uint8)
        for c in range(b):
            for t in range(frames):
                out[c, t] = cond[c, 2 * t, 53] > 0.5 or cond[c, 2 * t + 1, 53] > 0.5
        return out
    S = 2 * frames // (b + 1)
    h = S // 2
    out = np.zeros((1, frames), np.uint8)
    for t in range(frames):
        k = min(t // h, b - 1)
        loc = t - k * h
        out[0, t] = cond[k, 2 * loc, 53] > 0.5 or cond[k, 2 * loc + 1, 53] > 0.5
    return out


SHAPES = [(1, 1, 1), (1, 1, 3), (2, 2, 4), (1, 3, 20), (2, 3, 45), (3, 5, 150), (1, 3, 1125)]
_cache = {}


def synth(b, dn, T, seed=0):
    """A seeded smooth random motion at metre scale, contacts in [0, 1] and about one beat per 15 frames:
    (joints (b, dn, T, 24, 3) float32, contacts (b, dn, T, 4) float32, beats (b, T) uint8).  Cached; treat as read-only."""
    key = (b, dn, T, seed)
    if key in _cache:
        return _cache[key]
    g = np.random.default_rng([seed, b, dn, T])
    sec = np.arange(T, dtype=np.float64).reshape(T, 1, 1, 1, 1) / 30.0

    def waves(joints_, amp, f_lo, f_hi, k=4):
        """(T, b, dn, joints_, 3): k sinusoids of random frequency, phase and amplitude per coordinate"""
        shape = (k, 1, b, dn, joints_, 3)
        f, ph = g.uniform(f_lo, f_hi, shape), g.uniform(0, 2 * np.pi, shape)
        return (g.uniform(0.3, 1.0, shape) * amp / k * np.sin(2 * np.pi * f * sec[None] + ph)).sum(0)

    root = waves(1, 0.5, 0.1, 0.6) + g.uniform(-0.4, 0.4, (1, b, dn, 1, 3)) * np.array([1.0, 1.0, 0.0]) + np.array([0.0, 0.0, 0.9])
    limb = waves(24, 0.12, 0.3, 2.0) + g.uniform(-0.5, 0.5, (1, b, dn, 24, 3))
    limb[:, :, :, 0] = 0.0
    bounce = 0.08 * np.sin(2 * np.pi * g.uniform(0.8, 1.2, (1, b, dn, 1, 1)) * sec + g.uniform(0, 2 * np.pi, (1, b, dn, 1, 1)))
    root = root + bounce * np.array([0.0, 0.0, 1.0])      # a dancer's bounce: the speed has minima even in a 20-frame clip
    joints = np.ascontiguousarray((root + limb).transpose(1, 2, 0, 3, 4)).astype(np.float32)
    contacts = g.uniform(0.0, 1.0, (b, dn, T, 4))
    contacts = np.where(g.uniform(size=contacts.shape) < 0.4, 0.96 + 0.04 * contacts, contacts).astype(np.float32)
    beats = (g.uniform(size=(b, T)) < 1.0 / 15.0).astype(np.uint8)
    if T >= 15:
        beats[:, 7] = 1                                                                 # every clip has music beats
    _cache[key] = (joints, contacts, beats)
    return _cache[key]


def short_wrap_case():
    """T = 8 (N = 7) at sigma_smooth 5: the filter radius 20 exceeds 2 N, so the reflection wraps more than a whole period.
    A speed profile symmetric about frame 3 has no first harmonic in its reflected extension, so the smoothed speed keeps a strict
    minimum there (the second harmonic, ~4e-5 of the profile after smoothing: far above the 1e-9 near-tie margin); a one-sided
    profile has none.  (joints (1, 2, 8, 24, 3), contacts, beats with music beats on frames 3 and 5)"""
    g = np.random.default_rng(8)
    v = np.array([[0.05, 0.03, 0.012, 0.005, 0.012, 0.03, 0.05], [0.005, 0.012, 0.02, 0.03, 0.04, 0.05, 0.06]])
    x = np.concatenate([np.zeros((2, 1)), np.cumsum(v, 1)], 1)                      # (2, 8)
    J = np.broadcast_to(g.uniform(-0.5, 0.5, (1, 2, 1, 24, 3)), (1, 2, 8, 24, 3)).copy()
    J[0, :, :, :, 0] += x[:, :, None]
    J[0, 1, :, :, 1] += 2.0
    beats = np.zeros((1, 8), np.uint8)
    beats[0, [3, 5]] = 1
    return J.astype(np.float32), g.uniform(0, 1, (1, 2, 8, 4)).astype(np.float32), beats
