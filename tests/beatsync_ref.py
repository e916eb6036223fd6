"""A float64 numpy restatement of include/tcdiff_beatsync.h, for the tests: the speed curve and its minima, the matching, the anchors,
the warp and the resampling, written from the header and not from the kernels -- no tiles, no lists in LDS, no ballots; the matching
groups the claims by kinematic beat instead of scanning neighbours.  The PCHIP slopes and values are tests/choreo_ref.py's, the
quaternions tests/smooth_ref.py's (the restatements of the headers this one builds on)."""
import functools

import numpy as np

import choreo_ref as CR
import smooth_ref as SR

NAN = float("nan")
LINEAR = 0.01
INTS = ("status", "kin_count", "music_count", "matched", "dropped", "anchors", "rate_min_frame", "rate_max_frame")
FLOATS = ("shift_max", "rate_min", "rate_max")
# the bounds the GPU tests hold the kernels to (tests/test_beatsync_gpu.py, tests/test_post_chain_gpu.py):
# 4 x the largest difference seen over test_beatsync_gpu's SHAPES x share x contacts on an MI355X, as printed by its
# test_beat_sync_against_the_restatement and kept in profiles/beatsync.txt: the rotations against the restatement's float64 rotation vectors
# (the one float32 rounding of a rotation vector whose components stay below 0.5: 2^-26 sqrt(3) = 2.6e-8 rad), the joints against a float64 FK
# of the returned float32 poses
ROT_MEASURED, FK_MEASURED = 2.53e-8, 7.81e-7
ROT_BOUND, FK_BOUND = 4 * ROT_MEASURED, 4 * FK_MEASURED


def gaussian_table(sigma):
    """the 2 rad + 1 normalised weights, as scipy.ndimage builds them"""
    rad = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-rad, rad + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return w / w.sum()


def speed_of(J):
    """v [T - 1] of one dancer's float32 joints (T, 24, 3): ascending joints to 0.0, over 24"""
    J = np.asarray(J, np.float32).astype(np.float64)
    d = J[1:] - J[:-1]
    acc = np.zeros(d.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(24):
            acc = acc + np.sqrt((d[:, j, 0] * d[:, j, 0] + d[:, j, 1] * d[:, j, 1]) + d[:, j, 2] * d[:, j, 2])
        return acc / 24.0


def pooled(vs):
    """the warp's curve of its dancers' v: one dancer's own, or the mean in ascending dancer order"""
    if len(vs) == 1:
        return vs[0]
    acc = np.zeros_like(vs[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for v in vs:
            acc = acc + v
        return acc / float(len(vs))


def reflect(i, N):
    m = np.mod(i, 2 * N)
    return np.where(m >= N, 2 * N - 1 - m, m)


def filtered(pv, w):
    """s [N]: ascending taps to 0.0"""
    N, rad = pv.shape[0], (len(w) - 1) // 2
    acc = np.zeros(N)
    if N == 0:
        return acc
    t = np.arange(N)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in range(-rad, rad + 1):
            acc = acc + w[x + rad] * pv[reflect(t + x, N)]
    return acc


def curve(vs, w, T):
    """(status, s, kin flags [T]) of a warp"""
    pv = pooled(vs)
    status = int(not np.isfinite(pv).all())
    s = filtered(pv, w)
    kin = np.zeros(T, np.uint8)
    if status:
        return 1, np.full(T - 1, NAN), kin
    for t in range(1, T - 2):
        kin[t] = s[t] < s[t - 1] and s[t] < s[t + 1]
    return 0, s, kin


def match(kin_frames, music_frames, max_shift):
    """the candidates [(m, k)] in ascending m"""
    claims = {}
    for m in music_frames:
        if len(kin_frames) == 0:
            continue
        k = min(kin_frames, key=lambda k: (abs(k - m), k))
        if abs(k - m) <= max_shift:
            claims.setdefault(k, []).append(m)
    return sorted((min(ms, key=lambda m: (abs(k - m), m)), k) for k, ms in claims.items())


def shift_of(m, k, strength):
    return strength * float(k - m)


def anchors(cands, T, strength, max_rate):
    """(keys, values, dropped): the fixed ends and the candidates kept; a value is its key plus the shift strength (k - m)"""
    lo = 1.0 / max_rate
    keys, vals, dropped = [0], [0.0], 0
    for m, k in cands:
        u = float(m) + shift_of(m, k, strength)
        r = (u - vals[-1]) / float(m - keys[-1])
        if lo <= r <= max_rate:
            keys.append(m)
            vals.append(u)
        else:
            dropped += 1
    end = float(T - 1)
    while len(keys) > 1 and not lo <= (end - vals[-1]) / float((T - 1) - keys[-1]) <= max_rate:
        keys.pop()
        vals.pop()
        dropped += 1
    return keys + [T - 1], vals + [end], dropped


def warp_of(keys, vals, T, shifts=None):
    """the PCHIP cubic of the values, evaluated about the diagonal; shifts: value - key as the anchors formed it (default: recomputed,
    exact where both are small integers or halves)"""
    if len(keys) <= 2:
        return np.arange(T, dtype=np.float64)
    shifts = [v - float(k) for k, v in zip(keys, vals)] if shifts is None else shifts
    d1 = [d - 1.0 for d in CR.slopes(keys, vals)]
    return np.array([min(max(float(t) + CR.evaluate(keys, shifts, d1, t), 0.0), float(T - 1)) for t in range(T)])


def first_extreme(v, smaller):
    """(value, frame) of the extreme of v, the lower frame on a tie; (nan, -1) of nothing"""
    if len(v) == 0:
        return NAN, -1
    t = int(np.argmin(v) if smaller else np.argmax(v))          # numpy returns the first of equal extremes
    return float(v[t]), t


def slerp(qa, qb, a):
    """rotation vectors (24, 3) float32 of two frames -> (24, 3) float64"""
    A, B = SR.quat(qa), SR.quat(qb)
    d = ((A[:, 0] * B[:, 0] + A[:, 1] * B[:, 1]) + A[:, 2] * B[:, 2]) + A[:, 3] * B[:, 3]
    neg = d < 0.0
    d = np.where(neg, -d, d)
    B = np.where(neg[:, None], -B, B)
    linear = (1.0 - d) < LINEAR
    with np.errstate(invalid="ignore", divide="ignore"):
        om = np.arccos(np.where(linear, 0.0, d))
        so = np.sin(om)
        w0 = np.where(linear, 1.0 - a, np.sin((1.0 - a) * om) / so)
        w1 = np.where(linear, a, np.sin(a * om) / so)
    R = w0[:, None] * A + w1[:, None] * B
    n = np.sqrt(((R[:, 0] * R[:, 0] + R[:, 1] * R[:, 1]) + R[:, 2] * R[:, 2]) + R[:, 3] * R[:, 3])
    return SR.rotvec(R / n[:, None])


def resample_one(q, pos, contacts, warp):
    """one dancer: q (T, 24, 3), pos (T, 3), contacts (T, 4) or None, float32 -> (q_out, q64, pos_out, contacts_out, moved, copied)"""
    T = q.shape[0]
    q_out, pos_out = np.array(q), np.array(pos)
    q64 = q.astype(np.float64)
    c_out = None if contacts is None else np.array(contacts)
    moved = copied = 0
    for t in range(T):
        u = float(warp[t])
        i = min(max(int(np.floor(u)), 0), T - 1)
        a = u - float(i)
        moved += u != float(t)
        if a == 0.0:
            q_out[t], pos_out[t], q64[t] = q[i], pos[i], q[i].astype(np.float64)
            if c_out is not None:
                c_out[t] = contacts[i]
            continue
        if np.isfinite(pos[i]).all() and np.isfinite(pos[i + 1]).all():
            pos_out[t] = ((1.0 - a) * pos[i].astype(np.float64) + a * pos[i + 1].astype(np.float64)).astype(np.float32)
        else:
            copied += 1
        ok = np.isfinite(q[i]).all(-1) & np.isfinite(q[i + 1]).all(-1)
        with np.errstate(invalid="ignore"):
            r = slerp(q[i], q[i + 1], a)
        q_out[t][ok], q64[t][ok] = r[ok].astype(np.float32), r[ok]
        copied += int((~ok).sum())
        if c_out is not None:
            c_out[t] = contacts[i] if a < 0.5 else contacts[i + 1]
    return q_out, q64, pos_out, c_out, moved, copied


def joints_of(q, pos, dn):
    """the float32 joints (b, dn, T, 24, 3) of poses in rows: the float64 FK of tests/smooth_ref.py, rounded (the CPU tests' stand-in
    for the float32 fk_forward whose joints the device hands the speed curve)"""
    with np.errstate(invalid="ignore"):
        return SR.fk(SR.frames_of(q, dn), SR.frames_of(pos, dn)).astype(np.float32)


def motion_beats(joints, sigma_smooth=5.0, share=False):
    joints = np.asarray(joints)
    b, dn, T = joints.shape[:3]
    W, w = (1 if share else dn), gaussian_table(sigma_smooth)
    out = dict(speed=np.zeros((b, W, T - 1)), kin=np.zeros((b, W, T), np.uint8), kin_count=np.zeros((b, W), np.int32),
               status=np.zeros((b, W), np.int32))
    for c in range(b):
        for x in range(W):
            vs = [speed_of(joints[c, d]) for d in (range(dn) if share else [x])]
            out["status"][c, x], out["speed"][c, x], out["kin"][c, x] = curve(vs, w, T)
            out["kin_count"][c, x] = out["kin"][c, x].sum()
    return out


def beat_sync(q, pos, beats, dn, contacts=None, share=True, max_shift=7, max_rate=1.5, strength=1.0, sigma_smooth=5.0, joints_in=None):
    """q (b, T dn, 24, 3), pos (b, T dn, 3) float32 rows, beats (b, T) uint8, contacts (b, dn, T, 4) or None; joints_in: the float32
    joints of the input the speed is taken from (default: joints_of).  A dict of numpy arrays under BeatSync's names, q64 the
    rotations before their rounding."""
    q, pos, beats = np.asarray(q, np.float32), np.asarray(pos, np.float32), np.asarray(beats)
    b, T = q.shape[0], q.shape[1] // dn
    W = 1 if share else dn
    J = joints_of(q, pos, dn) if joints_in is None else np.asarray(joints_in, np.float32)
    mb = motion_beats(J, sigma_smooth, share)
    fq, fp = SR.frames_of(q, dn), SR.frames_of(pos, dn)
    out = dict(mb, warp=np.zeros((b, W, T)), moved=np.zeros((b, dn), np.int32), copied=np.zeros((b, dn), np.int32))
    out.update({k: np.zeros((b, W), np.int32) for k in INTS if k not in out}, **{k: np.zeros((b, W)) for k in FLOATS})
    oq, oq64, op = np.array(fq), fq.astype(np.float64), np.array(fp)
    oc = None if contacts is None else np.array(contacts, np.float32)
    for c in range(b):
        music = [m for m in range(1, T - 1) if beats[c, m] != 0]
        for x in range(W):
            kin = [int(t) for t in np.nonzero(mb["kin"][c, x])[0]]
            cands = [] if mb["status"][c, x] else match(kin, music, max_shift)
            keys, vals, dropped = anchors(cands, T, strength, max_rate)
            kept = dict(cands)
            warp = warp_of(keys, vals, T, [0.0] + [shift_of(m, kept[m], strength) for m in keys[1:-1]] + [0.0])
            out["warp"][c, x] = warp
            out["music_count"][c, x], out["matched"][c, x], out["dropped"][c, x], out["anchors"][c, x] = len(music), len(cands), dropped, len(keys) - 2
            out["shift_max"][c, x] = float(np.abs(warp - np.arange(T)).max())
            rate = warp[1:] - warp[:-1]
            out["rate_min"][c, x], out["rate_min_frame"][c, x] = first_extreme(rate, True)
            out["rate_max"][c, x], out["rate_max_frame"][c, x] = first_extreme(rate, False)
            for d in (range(dn) if share else [x]):
                oq[c, d], oq64[c, d], op[c, d], cc, out["moved"][c, d], out["copied"][c, d] = \
                    resample_one(fq[c, d], fp[c, d], None if contacts is None else np.asarray(contacts, np.float32)[c, d], warp)
                if oc is not None:
                    oc[c, d] = cc
    out.update(q=SR.rows_of(oq), q64=SR.rows_of(oq64), pos=SR.rows_of(op), contacts=oc)
    return out


# ---- the seeded cases ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(b, dn, T, seed=3, period=7):
    """a clean dance of tests/smooth_ref.py (sinusoids of 0.3-2 Hz), contacts in [0, 1] and music beats every `period` frames from a
    seeded phase on (T = 300: about 40 of them), one beat dropped and one doubled so that the spacing is not all alike.
    Read-only (q, pos, contacts, beats)"""
    q, pos, _, _ = SR.noisy_case(b=b, dn=dn, T=T, seed=seed)
    g = np.random.default_rng(seed + 1000)
    contacts = g.uniform(0, 1, (b, dn, T, 4)).astype(np.float32)
    beats = np.zeros((b, T), np.uint8)
    for c in range(b):
        on = np.arange(int(g.integers(0, period)), T, period)
        beats[c, on] = 1
        if len(on) > 4:
            beats[c, on[2]] = 0
            beats[c, min(on[3] + 1, T - 1)] = 1
    beats[:, [0, T - 1]] = 1                                  # the end frames carry beats that are never music beats
    for a in (contacts, beats):
        a.setflags(write=False)
    return q, pos, contacts, beats


@functools.lru_cache(maxsize=None)
def late_dancers(dn=3, T=160, period=20, seed=4):
    """every rotation component and the root move as A cos(pi (t - lag) / period): every joint's speed is smallest at lag + n period,
    `lag` = 3 or 4 frames (by dancer) after the music's beats at n period; seeded amplitudes, a little seeded noise.
    Read-only (q, pos, beats, lags)"""
    g = np.random.default_rng(seed)
    lags = np.array([3 + d % 2 for d in range(dn)])
    t = np.arange(T)[:, None, None, None]
    ph = np.pi * (t - lags[None, :, None, None]) / period
    q = g.uniform(0.05, 0.3, (1, dn, 24, 3)) * np.cos(ph) + g.normal(0, 1e-4, (T, dn, 24, 3))
    pos = g.uniform(0.1, 0.3, (1, dn, 3)) * np.cos(ph[..., 0]) + np.arange(dn)[None, :, None] * 1.5 + g.normal(0, 1e-5, (T, dn, 3))
    beats = np.zeros((1, T), np.uint8)
    beats[0, period:T - 1:period] = 1
    out = (np.ascontiguousarray(q.reshape(1, T * dn, 24, 3), np.float32), np.ascontiguousarray(pos.reshape(1, T * dn, 3), np.float32), beats, lags)
    for a in out:
        a.setflags(write=False)
    return out
