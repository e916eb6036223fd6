"""include/tcdiff_footlock.h restated in float64, frame by frame, with Python floats (IEEE double, every operation rounded on its own):
the reference the HIP kernels and the host build of csrc/footlock_math.h are held to.  Written from the header, not from the kernel:
plain loops over clips, dancers, legs and frames, no chunks, no wave.  Also the seeded synthetic motion the tests share."""
import math
from functools import lru_cache

import numpy as np

from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS

LEGS = ((1, 4, 7, 10), (2, 5, 8, 11))          # hip, knee, ankle, toe
SMALL, TINY = 1e-3, 1e-9
# the bounds the GPU tests hold the kernels to (tests/test_footlock_gpu.py, tests/test_post_chain_gpu.py)
ROT_BOUND = 1e-6          # the one float32 rounding is 2^-24 pi sqrt(3) = 3.3e-7 rad; a wrong formula errs by 1e-3 or more
PIN_BOUND = 2e-6          # three joints and the pelvis at 3.3e-7 rad over a lever of at most 0.95 m: below 1e-6 m


# ---- vectors and quaternions (w, x, y, z) as tuples of floats -----------------------------------------------------------------------------
def add(a, b): return (a[0] + b[0], a[1] + b[1], a[2] + b[2])
def sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def scale(a, s): return (a[0] * s, a[1] * s, a[2] * s)
def over(a, s): return (a[0] / s, a[1] / s, a[2] / s)
def dot(a, b): return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
def norm(a): return math.sqrt(dot(a, a))
def cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def half_sinc(theta):
    a2 = theta * theta
    return (0.5 - a2 / 48.0) + a2 * a2 / 3840.0 if theta < SMALL else math.sin(theta / 2.0) / theta


def quat(r):
    r0, r1, r2 = float(r[0]), float(r[1]), float(r[2])
    theta = math.sqrt((r0 * r0 + r1 * r1) + r2 * r2)
    k = half_sinc(theta)
    return (math.cos(theta / 2.0), k * r0, k * r1, k * r2)


def mul(a, b):
    return (((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3], ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
            ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1], ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0])


def conj(q): return (q[0], -q[1], -q[2], -q[3])


def rot(q, v):
    u = q[1:]
    t = scale(cross(u, v), 2.0)
    return add(add(v, scale(t, q[0])), cross(u, t))


def about(n, phi):
    s = math.sin(phi / 2.0)
    return (math.cos(phi / 2.0), n[0] * s, n[1] * s, n[2] * s)


def rotvec(q):
    if q[0] < 0.0:
        q = (-q[0], -q[1], -q[2], -q[3])
    u = q[1:]
    return over(u, half_sinc(2.0 * math.atan2(norm(u), q[0])))


def angle_between(ra, rb):
    """the relative rotation angle of two rotation vectors, in radians"""
    q = mul(conj(quat(ra)), quat(rb))
    return 2.0 * math.atan2(norm(q[1:]), abs(q[0]))


# ---- step 1 ---------------------------------------------------------------------------------------------------------------------------------
def chain(pose, root, leg, offsets=SMPL_OFFSETS):
    """pose (24, 3) float32, root (3,) float32 -> dict of the leg's world positions and rotations"""
    h, k, a, e = LEGS[leg]
    off = [tuple(float(np.float32(c)) for c in offsets[j]) for j in (h, k, a, e)]
    R0, P0 = quat(pose[0]), tuple(float(c) for c in root)
    Ph = add(P0, rot(R0, off[0]))
    Rh = mul(R0, quat(pose[h]))
    Pk = add(Ph, rot(Rh, off[1]))
    Rk = mul(Rh, quat(pose[k]))
    Pa = add(Pk, rot(Rk, off[2]))
    Ra = mul(Rk, quat(pose[a]))
    Pe = add(Pa, rot(Ra, off[3]))
    return dict(R0=R0, Ph=Ph, Pk=Pk, Pa=Pa, Pe=Pe, Rh=Rh, Rk=Rk, Ra=Ra, l1=norm(off[1]), l2=norm(off[2]))


# ---- step 3 ---------------------------------------------------------------------------------------------------------------------------------
def ease(t, t0, t1, d0, d1, blend):
    if t0 is not None and t1 is not None and (t1 - t0) - 1 <= 2 * blend:
        w0, w1, G = float(t1 - t), float(t - t0), float(t1 - t0)
        return tuple((w0 * d0[c] + w1 * d1[c]) / G for c in range(3))
    n = float(blend + 1)
    a = scale(d0, max(0.0, 1.0 - float(t - t0) / n)) if t0 is not None else (0.0, 0.0, 0.0)
    b = scale(d1, max(0.0, 1.0 - float(t1 - t) / n)) if t1 is not None else (0.0, 0.0, 0.0)
    return add(a, b)


# ---- step 4 ---------------------------------------------------------------------------------------------------------------------------------
def reach_of(c, d, reach):
    """(status, r'): 0 left as it is, 1 within reach, 2 clamped"""
    if d[0] == 0.0 and d[1] == 0.0 and d[2] == 0.0:
        return 0, None
    r = norm(sub(c["Pa"], c["Ph"]))
    nv = norm(sub(add(c["Pa"], d), c["Ph"]))
    if nv < TINY:
        return 0, None
    l1, l2 = c["l1"], c["l2"]
    rmax, rmin = (l1 + l2) * (1.0 - reach), abs(l1 - l2) + reach * (l1 + l2)
    rp = max(min(nv, max(rmax, r)), rmin)
    return (2 if rp != nv else 1), rp


def solve(c, d, reach):
    """-> (status, (q_h, q_k, q_a) float64 rotation vectors or None, dict of what the tests look at)"""
    status, rp = reach_of(c, d, reach)
    if status == 0:
        return 0, None, {}
    H, K, A, l1, l2 = c["Ph"], c["Pk"], c["Pa"], c["l1"], c["l2"]
    r = norm(sub(A, H))
    vp = sub(add(A, d), H)
    nv = norm(vp)
    a, b = sub(K, H), sub(A, K)
    cr = cross(a, b)
    nc = norm(cr)
    theta = math.atan2(nc, dot(a, b))
    fallback = nc < TINY * l1 * l2
    if fallback:
        x = rot(c["Rh"], (1.0, 0.0, 0.0))
        p = sub(x, scale(a, dot(x, a) / dot(a, a)))
        if norm(p) < TINY:
            return 0, None, {}
        n = over(p, norm(p))
    else:
        n = over(cr, nc)
    cs = max(-1.0, min(1.0, ((l1 * l1 + l2 * l2) - rp * rp) / ((2.0 * l1) * l2)))
    delta = 0.0 if rp == r else (math.pi - math.acos(cs)) - theta
    S1 = about(n, delta)
    w = sub(add(K, rot(S1, b)), H)
    u1, u2 = over(w, norm(w)), over(vp, nv)
    c2 = cross(u1, u2)
    n2, dt = norm(c2), dot(u1, u2)
    S2 = (1.0, 0.0, 0.0, 0.0)
    if n2 < 1e-300:
        if dt < 0.0:
            return 0, None, {}
    else:
        S2 = about(over(c2, n2), math.atan2(n2, dt))
    Rh2 = mul(S2, c["Rh"])
    Rk2 = mul(mul(S2, S1), c["Rk"])
    out = (rotvec(mul(conj(c["R0"]), Rh2)), rotvec(mul(conj(Rh2), Rk2)), rotvec(mul(conj(Rk2), c["Ra"])))
    return status, out, dict(rp=rp, nv=nv, fallback=fallback, target=add(H, scale(u2, rp)))


# ---- the whole of it --------------------------------------------------------------------------------------------------------------------------
def foot_lock(q, pos, contacts=None, *, dn, contact_threshold=0.95, still=0.01, blend=5, reach=1e-3, offsets=SMPL_OFFSETS):
    """q (b, T dn, 24, 3), pos (b, T dn, 3) float32 arrays, contacts (b, dn, T, 4) float32 or None.  Returns a dict:
    q (float32, rounded once), q64 (the same before the rounding), planted, clamped (b, dn, 2) int, max_shift (b, dn, 2) float64,
    g (b, dn, 2, T) labels 0 / 1 ankle / 2 toe, d (b, dn, 2, T, 3) shifts, anchor (b, dn, 2, T, 3; NaN outside runs),
    status (b, dn, 2, T), info[(c, dd, leg, t)] -> solve's dict, min_margin: the least | displacement - still | (motion labels)."""
    q = np.asarray(q, np.float32)
    pos = np.asarray(pos, np.float32)
    b, rows = q.shape[:2]
    T = rows // dn
    thr = np.float32(contact_threshold)
    q64 = q.astype(np.float64)
    planted, clamped = np.zeros((b, dn, 2), np.int64), np.zeros((b, dn, 2), np.int64)
    max_shift = np.zeros((b, dn, 2))
    G = np.zeros((b, dn, 2, T), np.int64)
    D = np.zeros((b, dn, 2, T, 3))
    anchor = np.full((b, dn, 2, T, 3), np.nan)
    status = np.zeros((b, dn, 2, T), np.int64)
    info, margin = {}, math.inf
    for c in range(b):
        for dd in range(dn):
            for leg in range(2):
                ch = [chain(q[c, t * dn + dd], pos[c, t * dn + dd], leg, offsets) for t in range(T)]
                g = []
                for t in range(T):
                    if contacts is not None:
                        ca = np.float32(contacts[c, dd, t, leg]) > thr
                        ce = np.float32(contacts[c, dd, t, 2 + leg]) > thr
                    elif t == T - 1:
                        ca = ce = True
                    else:
                        sa, se = norm(sub(ch[t + 1]["Pa"], ch[t]["Pa"])), norm(sub(ch[t + 1]["Pe"], ch[t]["Pe"]))
                        margin = min(margin, abs(sa - still), abs(se - still))
                        ca, ce = sa < still, se < still
                    g.append(1 if ca else (2 if ce else 0))
                d = [None] * T
                t = 0
                while t < T:
                    if g[t] == 0:
                        t += 1
                        continue
                    end = t
                    while end + 1 < T and g[end + 1] == g[t]:
                        end += 1
                    key = "Pa" if g[t] == 1 else "Pe"
                    s = (0.0, 0.0, 0.0)
                    for u in range(t, end + 1):
                        s = add(s, ch[u][key])
                    A = over(s, float(end - t + 1))
                    for u in range(t, end + 1):
                        d[u] = sub(A, ch[u][key])
                        anchor[c, dd, leg, u] = A
                    t = end + 1
                isp = [x != 0 for x in g]
                for t in range(T):
                    if isp[t]:
                        continue
                    t0 = next((u for u in range(t - 1, -1, -1) if isp[u]), None)
                    t1 = next((u for u in range(t + 1, T) if isp[u]), None)
                    d[t] = ease(t, t0, t1, d[t0] if t0 is not None else None, d[t1] if t1 is not None else None, blend)
                for t in range(T):
                    st, out, inf = solve(ch[t], d[t], reach)
                    clamped[c, dd, leg] += reach_of(ch[t], d[t], reach)[0] == 2
                    status[c, dd, leg, t] = st
                    if st:
                        info[(c, dd, leg, t)] = inf
                        for j, r in zip(LEGS[leg][:3], out):
                            q64[c, t * dn + dd, j] = r
                    max_shift[c, dd, leg] = max(max_shift[c, dd, leg], norm(d[t]))
                planted[c, dd, leg] = sum(isp)
                G[c, dd, leg] = g
                D[c, dd, leg] = d
    return dict(q=q64.astype(np.float32), q64=q64, planted=planted, clamped=clamped, max_shift=max_shift, g=G, d=D, anchor=anchor,
                status=status, info=info, min_margin=margin)


# ---- the shared synthetic motion ----------------------------------------------------------------------------------------------------------------
DN = 2
DRIFT = (0.006, 0.0, 0.003)          # metres per frame on the root: a planted foot slides by 6.7 mm a frame, less the wobble

# name -> (T, blend, runs[dancer][leg] = [(first, last, "a" | "e")]); b = 1
CASES = {
    "T1": (1, 5, [[[(0, 0, "a")], []], [[], [(0, 0, "e")]]]),
    "T2": (2, 5, [[[(0, 1, "a")], [(1, 1, "e")]], [[(0, 0, "e")], []]]),
    "T64": (64, 5, [[[(0, 63, "a")], []], [[], [(0, 63, "e")]]]),
    "T65": (65, 5, [[[(60, 64, "a")], [(3, 9, "e")]], [[(60, 64, "e")], []]]),
    "T130-one": (130, 5, [[[(50, 129, "a")], []], [[], [(60, 129, "e")]]]),
    "T130-edges": (130, 5, [[[(55, 63, "a"), (64, 72, "e")], [(58, 63, "e"), (64, 70, "a"), (120, 127, "a"), (128, 129, "e")]],
                            [[(64, 80, "a")], [(40, 63, "a")]]]),
    "ends": (40, 5, [[[(0, 3, "a"), (36, 39, "a")], [(0, 0, "e")]], [[(39, 39, "e")], [(0, 5, "e"), (30, 39, "a")]]]),
    # blend 3: gaps of 2 blend = 6, 2 blend + 1 = 7 and 2 blend + 2 = 8 frames
    "gaps": (40, 3, [[[(0, 4, "a"), (11, 14, "a"), (22, 25, "e"), (34, 36, "a")], [(2, 5, "e"), (14, 18, "a")]],
                     [[(5, 6, "a"), (15, 16, "a")], [(0, 1, "a"), (8, 9, "a")]]]),
    "blend0": (40, 0, [[[(0, 4, "a"), (11, 14, "a"), (22, 25, "e")], [(2, 5, "e")]], [[(5, 6, "a"), (8, 8, "e")], []]]),
    "off": (33, 5, [[[], []], [[], []]]),
}


def motion(T, seed, drift=DRIFT, dn=DN, speed=None):
    """q (1, T dn, 24, 3), pos (1, T dn, 3) float32: a random pose of sigma 0.3 rad per dancer, the knees flexed by a further 0.9 rad so
    that the legs have reach to spare, a wobble of 3 mrad, and a root that drifts; ``speed`` (T,) scales the drift frame by frame"""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None, None, None]
    base = rng.normal(0.0, 0.3, (1, dn, 24, 3))
    base[:, :, 4, 0] += 0.9
    base[:, :, 5, 0] += 0.9
    q = base + 0.003 * np.sin(rng.uniform(0.05, 0.2, (1, dn, 24, 3)) * t + rng.uniform(0, 6.28, (1, dn, 24, 3)))
    steps = np.ones(T) if speed is None else np.asarray(speed, np.float64)
    along = np.concatenate([[0.0], np.cumsum(steps)[:-1]])
    pos = rng.normal(0.0, 0.5, (1, dn, 3)) + along[:, None, None] * np.asarray(drift)
    return q.reshape(1, T * dn, 24, 3).astype(np.float32), pos.reshape(1, T * dn, 3).astype(np.float32)


def contacts_of(T, runs, dn=DN):
    c = np.zeros((1, dn, T, 4), np.float32)
    for d in range(dn):
        for leg in range(2):
            for first, last, kind in runs[d][leg]:
                c[0, d, first:last + 1, leg if kind == "a" else 2 + leg] = 1.0
    return c


@lru_cache(maxsize=None)
def case(name):
    """-> (q, pos, contacts, blend, the reference's result); computed once and shared, never written to"""
    T, blend, runs = CASES[name]
    q, pos = motion(T, seed=sum(map(ord, name)))
    contacts = contacts_of(T, runs)
    ref = foot_lock(q, pos, contacts, dn=DN, blend=blend)
    for a in (q, pos, contacts):
        a.setflags(write=False)
    return q, pos, contacts, blend, ref


MOTION_SEED = 11


@lru_cache(maxsize=None)
def motion_case():
    """contacts=None: the root alternates between 6.7 mm a frame (planted by the dataset's rule, still = 0.01) and 33 mm a frame"""
    T = 70
    speed = np.where((np.arange(T) // 9) % 2 == 0, 1.0, 5.0)
    q, pos = motion(T, seed=MOTION_SEED, speed=speed)
    ref = foot_lock(q, pos, None, dn=DN)
    return q, pos, ref


@lru_cache(maxsize=None)
def reach_case():
    """a foot pinned for 20 frames while the root drifts 1 m away"""
    T = 20
    q, pos = motion(T, seed=5, drift=(0.05, 0.0, 0.0))
    contacts = contacts_of(T, [[[(0, 19, "a")], []], [[], [(0, 19, "e")]]])
    return q, pos, contacts, foot_lock(q, pos, contacts, dn=DN)


assert SMPL_PARENTS[1] == SMPL_PARENTS[2] == 0 and [SMPL_PARENTS[j] for j in (4, 5, 7, 8, 10, 11)] == [1, 2, 4, 5, 7, 8]
