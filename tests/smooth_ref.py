"""The numpy float64 restatement of include/tcdiff_smooth.h: the tap tables, the filter of the root and of the rotations, the
change statistics and the jitter scores, every sum in the header's order (numpy's elementwise float64 operations round each product
and sum on its own, as the header asks).  Nothing here imports the package's filter; the GPU tests and the host build are held to it.
Also the seeded cases the tests share: a noisy dance over a clean one, and a rotation whose vector flips sign mid-clip."""
import functools

import numpy as np

from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS

J = 24
SMALL = 1e-3                              # TCK_SMALL: the series of sin(theta / 2) / theta below it
MIN_NORM = 1e-6
ALL = (1 << 24) - 1
# the bounds the GPU tests hold the kernels to (tests/test_smooth_gpu.py, tests/test_post_chain_gpu.py)
ROT_BOUND = 1e-6          # the one float32 rounding is 2^-24 pi sqrt(3) = 3.3e-7 rad, as tests/test_footlock_gpu.py
FK_BOUND = 1e-5
FLOATS = ("accel_mean", "jitter", "jitter_local", "root_jitter", "accel_max", "jitter_max")
INTS = ("accel_peak", "jitter_peak", "terms")


# ---- the tap tables ---------------------------------------------------------------------------------------------------------------------------
def table(W, p):
    R = (W - 1) // 2
    A = np.vander(np.arange(-R, R + 1, dtype=np.float64), p + 1, increasing=True)
    return A @ np.linalg.pinv(A)


def windows(T, W):
    """the first frame of every frame's window and the row of the table it uses"""
    t = np.arange(T)
    s = np.clip(t - (W - 1) // 2, 0, T - W)
    return s, t - s


def filter_signal(y, W, p):
    """a (T,) or (T, C) float64 signal through the table, taps in ascending frame order: what scipy's mode="interp" computes"""
    y = np.asarray(y, np.float64)
    tab = table(W, p)
    s, row = windows(y.shape[0], W)
    acc = np.zeros_like(y)
    for u in range(W):
        k = tab[row, u]
        acc = acc + (k if y.ndim == 1 else k[:, None]) * y[s + u]
    return acc


# ---- quaternions, as csrc/footlock_math.h forms them --------------------------------------------------------------------------------------------
def half_sinc(theta):
    a2 = theta * theta
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(theta < SMALL, (0.5 - a2 / 48.0) + a2 * a2 / 3840.0, np.sin(theta / 2.0) / theta)


def quat(r):
    """rotation vectors (..., 3) float32 -> unit quaternions (..., 4) float64, (w, x, y, z)"""
    return quat64(np.asarray(r, np.float32).astype(np.float64))


def quat64(r):
    r = np.asarray(r, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        theta = np.sqrt((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2])
        k = half_sinc(theta)
        return np.stack([np.cos(theta / 2.0), k * r[..., 0], k * r[..., 1], k * r[..., 2]], -1)


def rotvec(Q):
    Q = np.where(Q[..., :1] < 0.0, -Q, Q)
    u = Q[..., 1:]
    n = np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])
    theta = 2.0 * np.arctan2(n, Q[..., 0])
    return u / half_sinc(theta)[..., None]


def qmul(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([((aw * bw - ax * bx) - ay * by) - az * bz, ((aw * bx + ax * bw) + ay * bz) - az * by,
                     ((aw * by - ax * bz) + ay * bw) + az * bx, ((aw * bz + ax * by) - ay * bx) + az * bw], -1)


def rot_change(a, b):
    """the relative rotation angle of rotation vectors a and b (float32 values), elementwise"""
    Qa = quat(a)
    d = qmul(Qa * np.array([1.0, -1.0, -1.0, -1.0]), quat(b))
    with np.errstate(invalid="ignore"):
        return 2.0 * np.arctan2(np.sqrt((d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]), np.abs(d[..., 0]))


def angles(a, b):
    """the relative rotation angle of float64 rotation vectors, elementwise over the leading dimensions"""
    d = qmul(quat64(a) * np.array([1.0, -1.0, -1.0, -1.0]), quat64(b))
    return 2.0 * np.arctan2(np.sqrt((d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]), np.abs(d[..., 0]))


def angle_between(a, b):
    """the same of float64 rotation vectors that need not be float32 values: through rotation matrices"""
    def mat(r):
        r = np.asarray(r, np.float64)
        th = np.linalg.norm(r)
        if th < 1e-12:
            return np.eye(3)
        k = r / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M = mat(a).T @ mat(b)
    return float(np.arctan2(np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2.0, (np.trace(M) - 1.0) / 2.0))


# ---- the filter -------------------------------------------------------------------------------------------------------------------------------
def frames_of(a, dn):
    """(b, T dn, ...) rows -> (b, dn, T, ...)"""
    a = np.asarray(a)
    return np.moveaxis(a.reshape((a.shape[0], a.shape[1] // dn, dn) + a.shape[2:]), 2, 1)


def rows_of(a):
    """(b, dn, T, ...) -> (b, T dn, ...)"""
    a = np.moveaxis(np.asarray(a), 1, 2)
    return a.reshape((a.shape[0], a.shape[1] * a.shape[2]) + a.shape[3:])


def filter_root(pos, W, p):
    """pos (T, 3) float32 -> (unrounded float64 output, copied (T,) bool); a copied output is the input"""
    x = np.asarray(pos, np.float32).astype(np.float64)
    T = x.shape[0]
    s, _ = windows(T, W)
    with np.errstate(invalid="ignore", over="ignore"):
        out = filter_signal(x, W, p)
    bad = ~np.isfinite(x).all(-1)
    copied = np.array([bad[s[t]:s[t] + W].any() for t in range(T)])
    out[copied] = x[copied]
    return out, copied


def filter_rot(q, W, p, mask=ALL):
    """q (T, 24, 3) float32 -> (unrounded float64 rotation vectors, copied (T, 24) bool); copied and masked-out outputs are the input"""
    q = np.asarray(q, np.float32)
    T = q.shape[0]
    Q = quat(q)                                                        # (T, 24, 4)
    tab = table(W, p)
    s, row = windows(T, W)
    acc = np.zeros_like(Q)
    with np.errstate(invalid="ignore"):
        for u in range(W):
            Qu = Q[s + u]
            dot = ((Q[..., 0] * Qu[..., 0] + Q[..., 1] * Qu[..., 1]) + Q[..., 2] * Qu[..., 2]) + Q[..., 3] * Qu[..., 3]
            k = np.where(dot < 0.0, -tab[row, u][:, None], tab[row, u][:, None])
            acc = acc + k[..., None] * Qu
        n = np.sqrt(((acc[..., 0] * acc[..., 0] + acc[..., 1] * acc[..., 1]) + acc[..., 2] * acc[..., 2]) + acc[..., 3] * acc[..., 3])
        listed = np.array([(mask >> j) & 1 == 1 for j in range(J)])
        copied = ~(n >= MIN_NORM) & listed[None]
        out = rotvec(acc / np.where(n >= MIN_NORM, n, 1.0)[..., None])
    bad = ~np.isfinite(q.astype(np.float64)).all(-1)                   # the header's words: a non-finite float of the joint in the window
    by_window = np.array([bad[s[t]:s[t] + W].any(0) for t in range(T)]) & listed[None]
    assert np.array_equal(by_window & ~copied, np.zeros_like(copied)), "a non-finite window must come out as copied"
    keep = copied | ~listed[None]
    out[keep] = q.astype(np.float64)[keep]
    return out, copied


def smooth(q, pos, dn, window=9, polyorder=3, root_window=None, root_polyorder=None, joints_mask=ALL):
    """q (b, T dn, 24, 3), pos (b, T dn, 3) float32 -> dict: q64 / pos64 the unrounded outputs, q / pos their float32 roundings (the
    copied ones the input's words), copied_q (b, dn, T, 24) / copied_pos (b, dn, T) bool, copied (b, dn) int32, max_pos_change"""
    q, pos = np.asarray(q, np.float32), np.asarray(pos, np.float32)
    rw = window if root_window is None else root_window
    rp = polyorder if root_polyorder is None else root_polyorder
    qf, pf = frames_of(q, dn), frames_of(pos, dn)
    b = q.shape[0]
    q64, p64 = np.empty(qf.shape, np.float64), np.empty(pf.shape, np.float64)
    cq, cp = np.zeros(qf.shape[:4], bool), np.zeros(pf.shape[:3], bool)
    for c in range(b):
        for d in range(dn):
            q64[c, d], cq[c, d] = filter_rot(qf[c, d], window, polyorder, joints_mask)
            p64[c, d], cp[c, d] = filter_root(pf[c, d], rw, rp)
    q32, p32 = q64.astype(np.float32), p64.astype(np.float32)
    listed = np.array([(joints_mask >> j) & 1 == 1 for j in range(J)])
    keep = cq | ~listed[None, None, None]
    q32[keep] = qf[keep]
    p32[cp] = pf[cp]
    out = dict(q64=rows_of(q64), pos64=rows_of(p64), q=rows_of(q32), pos=rows_of(p32), copied_q=cq, copied_pos=cp,
               copied=(cq.sum((2, 3)) + cp.sum(2)).astype(np.int32))
    out.update(stats(q, pos, out["q"], out["pos"], dn))
    return out


def stats(q, pos, q_out, pos_out, dn):
    """max_rot_change and max_pos_change (b, dn) of the float32 values as stored"""
    a, b = frames_of(np.asarray(q, np.float32), dn), frames_of(np.asarray(q_out, np.float32), dn)
    ch = rot_change(a, b)
    ch = np.where(np.isfinite(ch), ch, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = frames_of(np.asarray(pos_out, np.float32), dn).astype(np.float64) - frames_of(np.asarray(pos, np.float32), dn).astype(np.float64)
        sh = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    sh = np.where(np.isfinite(sh), sh, 0.0)
    return dict(max_rot_change=ch.max((2, 3)), max_pos_change=sh.max(2))


# ---- the scores -------------------------------------------------------------------------------------------------------------------------------
def _norm(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def _lane_sum(frames, terms, ok):
    """terms (n, k) of the frames `frames`, ok which of them count: joints ascending to 0.0, frames ascending on lane t % 64, lanes
    ascending"""
    lanes = [0.0] * 64
    for i, t in enumerate(frames):
        fs = 0.0
        for j in range(terms.shape[1]):
            if ok[i, j]:
                fs = fs + float(terms[i, j])
        lanes[t % 64] = lanes[t % 64] + fs
    tot = 0.0
    for l in range(64):
        tot = tot + lanes[l]
    return tot


def _peak(frames, terms, ok):
    best = (np.nan, -1, -1)
    for i, t in enumerate(frames):
        for j in range(terms.shape[1]):
            if ok[i, j] and (best[1] < 0 or terms[i, j] > best[0]):          # ascending (frame, joint): the first of equals stays
                best = (float(terms[i, j]), int(t), j)
    return best


def smoothness_one(P, fps=30):
    """P (T, 24, 3) float32 -> the header's outputs of one dancer"""
    P = np.asarray(P, np.float32).astype(np.float64)
    T = P.shape[0]
    f2 = float(fps) * float(fps)
    f3 = f2 * float(fps)
    with np.errstate(invalid="ignore", over="ignore"):
        ta, tk = np.arange(1, T - 1), np.arange(1, T - 2)
        a = _norm((P[ta + 1] - 2.0 * P[ta]) + P[ta - 1]) * f2
        k = _norm(((P[tk + 2] - 3.0 * P[tk + 1]) + 3.0 * P[tk]) - P[tk - 1]) * f3
        L = P[:, 1:] - P[:, :1]
        kl = _norm(((L[tk + 2] - 3.0 * L[tk + 1]) + 3.0 * L[tk]) - L[tk - 1]) * f3
    oa, ok, ol = np.isfinite(a), np.isfinite(k), np.isfinite(kl)
    nan = float("nan")
    mean = lambda tot, n: tot / float(n) if n else nan
    out = dict(accel_mean=mean(_lane_sum(ta, a, oa), oa.sum()), jitter=mean(_lane_sum(tk, k, ok), ok.sum()),
               jitter_local=mean(_lane_sum(tk, kl, ol), ol.sum()), root_jitter=mean(_lane_sum(tk, k[:, :1], ok[:, :1]), ok[:, 0].sum()),
               terms=int(ok.sum()))
    pa, pk = _peak(ta, a, oa), _peak(tk, k, ok)
    out.update(accel_max=pa[0], accel_peak=list(pa[1:]), jitter_max=pk[0], jitter_peak=list(pk[1:]))
    return out


def smoothness(joints, fps=30):
    """joints (b, dn, T, 24, 3) float32 -> dict of (b, dn) float64 / (b, dn, 2) and (b, dn) int32 arrays"""
    joints = np.asarray(joints)
    b, dn = joints.shape[:2]
    rows = [[smoothness_one(joints[c, d], fps) for d in range(dn)] for c in range(b)]
    out = {k: np.array([[r[k] for r in row] for row in rows], np.float64) for k in FLOATS}
    out.update({k: np.array([[r[k] for r in row] for row in rows], np.int32) for k in INTS})
    return out


# ---- a forward kinematics (quaternions, float64) for the CPU tests; the GPU tests write another ---------------------------------------------------
def qrot(Q, v):
    u = Q[..., 1:]
    t = 2.0 * np.cross(u, v)
    return v + Q[..., :1] * t + np.cross(u, t)


def fk(q, pos):
    """q (..., 24, 3), pos (..., 3) -> joints (..., 24, 3) float64"""
    Ql = quat(np.asarray(q, np.float32))
    off = np.asarray(SMPL_OFFSETS, np.float32).astype(np.float64)
    P, W = [None] * J, [None] * J
    for j in range(J):
        p = SMPL_PARENTS[j]
        if p < 0:
            P[j], W[j] = np.asarray(pos, np.float64), Ql[..., j, :]
        else:
            P[j] = P[p] + qrot(W[p], off[j])
            W[j] = qmul(W[p], Ql[..., j, :])
    return np.stack(P, -2)


# ---- the seeded cases ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noisy_case(b=1, dn=1, T=150, seed=1, rot_sigma=0.02, pos_sigma=0.003):
    """a clean dance -- sinusoids of 0.3-2 Hz on every rotation component and on the root -- and the same with N(0, rot_sigma rad) on
    every rotation component and N(0, pos_sigma m) on the root; rows = frame dn + dancer.  Returns read-only (q_clean, pos_clean, q, pos)"""
    g = np.random.default_rng(seed)
    t = np.arange(T)[None, :, None, None, None] / 30.0
    shape = (b, 1, dn, J, 3)
    f, ph, amp = g.uniform(0.3, 2.0, shape), g.uniform(0, 2 * np.pi, shape), g.uniform(0.05, 0.4, shape)
    qc = amp * np.sin(2 * np.pi * f * t + ph)
    tp = t[..., 0]
    fp, pp, ap = g.uniform(0.3, 2.0, shape[:3] + (3,)), g.uniform(0, 2 * np.pi, shape[:3] + (3,)), g.uniform(0.05, 0.5, shape[:3] + (3,))
    pc = ap * np.sin(2 * np.pi * fp * tp + pp) + np.arange(dn)[None, None, :, None] * 1.5
    qn = qc + g.normal(0, rot_sigma, qc.shape)
    pn = pc + g.normal(0, pos_sigma, pc.shape)
    out = tuple(np.ascontiguousarray(a.reshape((b, T * dn) + a.shape[3:]), np.float32) for a in (qc, pc, qn, pn))
    for a in out:
        a.setflags(write=False)
    return out


def rms_joint_error(q, pos, q_clean, pos_clean):
    d = fk(q, pos) - fk(q_clean, pos_clean)
    return float(np.sqrt((d ** 2).sum(-1).mean()))


@functools.lru_cache(maxsize=None)
def flip_case(T=40, dn=1):
    """joint 3 turns about a fixed axis by an angle that runs from 3.0 to 3.28 rad, stored as rotation vectors wrapped into (-pi, pi]:
    the vector flips sign where the angle passes pi.  Returns read-only (q, pos, the clean angles (T,), the unit axis)"""
    axis = np.array([0.6, -0.48, 0.64])
    ang = np.linspace(3.0, 3.28, T)
    wrapped = np.where(ang > np.pi, ang - 2 * np.pi, ang)
    q = np.zeros((1, T, dn, J, 3))
    q[0, :, :, 3] = (wrapped[:, None] * axis[None])[:, None]
    q = np.ascontiguousarray(q.reshape(1, T * dn, J, 3), np.float32)
    pos = np.zeros((1, T * dn, 3), np.float32)
    assert (q.reshape(T, dn, J, 3)[0, 0, 3] @ axis > 0) and (q.reshape(T, dn, J, 3)[-1, 0, 3] @ axis < 0)
    for a in (q, pos):
        a.setflags(write=False)
    return q, pos, ang, axis
