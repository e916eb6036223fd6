"""numpy float64 restatement of include/tcdiff_ground.h, written from the header: loops over clips, dancers and runs; the frames of a
dancer are evaluated elementwise as arrays where the header's order allows it (every numpy operation rounds once, as the header's
arithmetic does) and one by one where it fixes an order (the sums).  Seeded inputs for the GPU test, built on footlock_ref's motion
with vertical profiles added, and the check that no decision the construction makes on them is a near-tie."""
import numpy as np

import footlock_ref as FR
import group_ref as G
from tcdiff_amd.fk import SMPL_OFFSETS

DEFAULTS = dict(up=2, radii=None, parents=None, contact_threshold=0.95, still=0.01, tolerance=0.005, blend=5, max_lift=0.5)
COUNTS = ("planted_frames", "penetration_frames", "float_frames")
VALUES = ("penetration_max", "penetration_mean", "float_mean")
GUARD = 1e-9
# the bound the GPU tests hold the float64 outputs to (tests/test_ground_gpu.py, tests/test_post_chain_gpu.py)
MEASURED = 0.0            # metres: the largest difference of a float64 output from the restatement over every case of tests/test_ground_gpu.py (profiles/ground.txt)
FLOAT_BOUND = min(100 * MEASURED, 1e-9)


def w(k, blend):
    """the envelope's weight k frames away: 1 - k / (blend + 1), Python floats (IEEE double, one rounding per operation)"""
    return 1.0 - float(k) / (float(blend) + 1.0)


def pos0(x):
    """max(x, 0) as the header takes it: +0 unless x > 0"""
    with np.errstate(invalid="ignore"):
        return np.where(x > 0.0, x, 0.0)


def lows(J, up, radii, parents):
    """J (T, 24, 3) float32 -> L, lo_l, lo_r (T,) float64: the body low over the 23 bones, the two foot lows"""
    Z = J[..., up].astype(np.float64)
    with np.errstate(invalid="ignore"):
        per_bone = np.stack([np.minimum(Z[:, parents[i]], Z[:, i]) - radii[i] for i in range(1, 24)], 1)
        L = per_bone.min(1)
        return L, np.minimum(Z[:, 7], Z[:, 10]) - radii[10], np.minimum(Z[:, 8], Z[:, 11]) - radii[11]


def labels(J, C, good, thr, still, det=None):
    """-> left, right (T,) bool: contacts C (T, 4) float32 or None (the still rule on J)"""
    T = J.shape[0]
    if C is not None:
        t32 = np.float32(thr)
        left = (C[:, 0] > t32) | (C[:, 2] > t32)
        right = (C[:, 1] > t32) | (C[:, 3] > t32)
        if det is not None:
            det["threshold"].extend(np.abs(C[good].astype(np.float64) - float(t32)).ravel().tolist())
    else:
        P = J.astype(np.float64)
        st = {}
        with np.errstate(invalid="ignore"):
            for j in (7, 8, 10, 11):
                d = P[1:, j] - P[:-1, j]
                n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                st[j] = np.concatenate([n < still, [True]])
                if det is not None:
                    ok = good[:-1] & ~np.isnan(n)
                    det["still"].extend(np.abs(n[ok] - still).tolist())
        left, right = st[7] | st[10], st[8] | st[11]
    return left & good, right & good


def foot_low(left, right, lo_l, lo_r):
    return np.where(left & right, np.minimum(lo_l, lo_r), np.where(left, lo_l, lo_r))


def base_shift(F, planted, Lf, blend):
    """step 5: B (T,) float64"""
    T = planted.shape[0]
    B = np.zeros(T)
    t = 0
    while t < T:
        if not planted[t]:
            t += 1
            continue
        s, acc = t, 0.0
        while s < T and planted[s]:
            acc = acc + (F - float(Lf[s]))
            s += 1
        B[t:s] = acc / float(s - t)
        t = s
    where = np.flatnonzero(planted)
    for t in range(T):
        if planted[t]:
            continue
        k = np.searchsorted(where, t)
        i = int(where[k - 1]) if k > 0 else -1
        j = int(where[k]) if k < where.size else -1
        if i >= 0 and j >= 0 and j - i - 1 <= 2 * blend:
            B[t] = B[i] + (B[j] - B[i]) * (float(t - i) / float(j - i))
        elif i >= 0 and t - i <= blend:
            B[t] = B[i] * w(t - i, blend)
        elif j >= 0 and j - t <= blend:
            B[t] = B[j] * w(j - t, blend)
    return B


def envelope(e, blend):
    """U[t] = max over |s - t| <= blend of e[s] w(|s - t|); a maximum of exact candidates, so its order is free"""
    T = e.shape[0]
    U = e * w(0, blend)
    for k in range(1, min(blend, T - 1) + 1):
        f = w(k, blend)
        U[k:] = np.maximum(U[k:], e[:-k] * f)
        U[:-k] = np.maximum(U[:-k], e[k:] * f)
    return U


def metrics(L, lo_l, lo_r, good, left, right, F, tolerance, det=None):
    """step 8 for one dancer -> counts (3,), values (3,)"""
    planted = left | right
    Lf = foot_low(left, right, lo_l, lo_r)
    n_good, n_planted = int(good.sum()), int(planted.sum())
    if not np.isfinite(F):
        return [n_planted, 0, 0], [np.nan] * 3
    low, high = F - tolerance, F + tolerance
    pen = int((good & (L < low)).sum())
    flo = int((planted & (Lf > high)).sum())
    x = pos0(F - L[good])
    y = pos0(Lf[planted] - F)
    sp = float(np.cumsum(x)[-1]) if x.size else 0.0           # np.cumsum adds in ascending order, one rounding a step
    sf = float(np.cumsum(y)[-1]) if y.size else 0.0
    if det is not None:
        det["tolerance"].extend(np.abs(L[good] - low).tolist() + np.abs(Lf[planted] - high).tolist())
    return [n_planted, pen, flo], [float(x.max()) if x.size else 0.0, sp / n_good if n_good else np.nan, sf / n_planted if n_planted else np.nan]


def ground(pos, joints, contacts=None, *, dn=None, floor=None, up=2, radii=None, parents=None, contact_threshold=0.95, still=0.01,
           tolerance=0.005, blend=5, max_lift=0.5, details=False):
    """pos (b, T dn, 3), joints (b, dn, T, 24, 3) float32, contacts (b, dn, T, 4) float32 or None; floor None, a number or (b,) -> the
    fields of tcdiff_amd.ground.Ground as numpy arrays (before / after as dicts with ground_metrics' keys), shift (b, dn, T); with
    ``details`` the planes B, U, L and the margins that judge() looks at"""
    pos, joints = np.asarray(pos), np.asarray(joints)
    assert joints.dtype == np.float32 and pos.dtype == np.float32 and joints.shape[3:] == (24, 3)
    b, dn_, T = joints.shape[:3]
    assert dn in (None, dn_) and pos.shape == (b, T * dn_, 3)
    dn = dn_
    radii = G.capsule_radii() if radii is None else np.asarray(radii, np.float64)
    parents = G.SMPL_PARENTS if parents is None else list(parents)
    det = {"threshold": [], "still": [], "tolerance": [], "excess": [], "cap": []}
    D = np.zeros((b, dn, T))
    capped = np.zeros((b, dn, T), bool)
    out_j, out_p = joints.copy(), pos.copy().reshape(b, T, dn, 3)
    F_of = np.zeros(b)
    before = {k: np.zeros((b, dn), np.int64) for k in COUNTS} | {k: np.zeros((b, dn)) for k in VALUES}
    after = {k: np.zeros((b, dn), np.int64) for k in COUNTS} | {k: np.zeros((b, dn)) for k in VALUES}
    planes = {k: np.zeros((b, dn, T)) for k in ("B", "U", "L", "L_after", "Lf_after")}
    planes["planted"] = np.zeros((b, dn, T), bool)
    for c in range(b):
        per = []
        for d in range(dn):
            J = joints[c, d]
            good = np.isfinite(J).all((1, 2))
            L, ll, lr = lows(J, up, radii, parents)
            left, right = labels(J, None if contacts is None else np.asarray(contacts[c, d], np.float32), good, contact_threshold, still,
                                 det if details else None)
            per.append((J, good, L, ll, lr, left, right))
        if floor is not None:
            F = float(np.broadcast_to(np.asarray(floor, np.float64), (b,))[c])
        else:
            feet = np.concatenate([np.concatenate([ll[left], lr[right]]) for _, _, _, ll, lr, left, right in per])
            body = np.concatenate([L[good] for _, good, L, _, _, _, _ in per])
            F = float(np.median(feet)) if feet.size else (float(np.median(body)) if body.size else np.nan)
        F_of[c] = F
        for d, (J, good, L, ll, lr, left, right) in enumerate(per):
            planted = left | right
            Lf = foot_low(left, right, ll, lr)
            if np.isfinite(F):
                B = base_shift(F, planted, Lf, blend)
                with np.errstate(invalid="ignore"):
                    ex = (F - L) - B
                e = np.where(good, pos0(ex), 0.0)
                U = envelope(e, blend)
                raw = B + U
                cap = good & ((raw > max_lift) | (raw < -max_lift))
                Dd = np.where(raw > max_lift, max_lift, np.where(raw < -max_lift, -max_lift, raw))
                Dd = np.where(good, Dd, 0.0)
                if details:
                    nz = ex[good]
                    det["excess"].extend(np.abs(nz[nz != 0.0]).tolist())          # an exact 0: B = F - Lf of a one-frame run with L = Lf
                    det["cap"].extend(np.abs(raw[good] - max_lift).tolist() + np.abs(raw[good] + max_lift).tolist())
                planes["B"][c, d], planes["U"][c, d] = B, U
            else:
                Dd, cap = np.zeros(T), np.zeros(T, bool)
            D[c, d], capped[c, d] = Dd, cap
            move = Dd != 0.0
            out_j[c, d, move, :, up] = (J[move, :, up].astype(np.float64) + Dd[move][:, None]).astype(np.float32)
            out_p[c, move, d, up] = (pos.reshape(b, T, dn, 3)[c, move, d, up].astype(np.float64) + Dd[move]).astype(np.float32)
            La, lla, lra = lows(out_j[c, d], up, radii, parents)
            cb, vb = metrics(L, ll, lr, good, left, right, F, tolerance, det if details else None)
            ca, va = metrics(La, lla, lra, good, left, right, F, tolerance, det if details else None)
            for n, k in enumerate(COUNTS):
                before[k][c, d], after[k][c, d] = cb[n], ca[n]
            for n, k in enumerate(VALUES):
                before[k][c, d], after[k][c, d] = vb[n], va[n]
            planes["L"][c, d], planes["L_after"][c, d], planes["planted"][c, d] = L, La, planted
            planes["Lf_after"][c, d] = foot_low(left, right, lla, lra)
    before["floor"] = after["floor"] = F_of
    step = np.abs(np.diff(D, axis=-1)).max(-1) if T > 1 else np.zeros((b, dn))
    out = dict(pos=out_p.reshape(b, T * dn, 3), joints=out_j, floor=F_of, before=before, after=after, capped=capped.sum(-1).astype(np.int64),
               max_shift=np.abs(D).max(-1), max_step=step, shift=D)
    if details:
        out["details"], out["planes"] = det, planes
    return out


def ground_metrics(joints, contacts=None, **kw):
    """ground_metrics' dict from the restatement: the "before" of ground() (nothing of the shift is needed for it)"""
    joints = np.asarray(joints)
    b, dn, T = joints.shape[:3]
    pos = np.ascontiguousarray(np.moveaxis(joints[:, :, :, 0], 1, 2).reshape(b, T * dn, 3))
    return ground(pos, joints, contacts, **kw)["before"]


def judge(ref):
    """(ok, reasons) from a ground(..., details=True) result: every margin of a discontinuous decision at least GUARD"""
    why = []
    for name, what in (("threshold", "a contact within {:.3e} of contact_threshold"), ("still", "a step within {:.3e} of still"),
                       ("tolerance", "a low within {:.3e} of floor -/+ tolerance"), ("excess", "an excess within {:.3e} of 0"),
                       ("cap", "a lift within {:.3e} of max_lift")):
        m = np.asarray(ref["details"][name], np.float64)
        if m.size and m.min() < GUARD:
            why.append(what.format(m.min()))
    return not why, why


def decisions_clear(pos, joints, contacts=None, **kw):
    """No discontinuous decision of the construction is a near-tie on these inputs, so an implementation that rounded differently in
    the last places would still decide the same way: the contact threshold, the still rule, the two tolerance counts (before and
    after), the excess > 0 test and the cap each at least 1e-9 from their boundary.  An excess of exactly 0 is left out: it is
    (F - L) - B with B = F - Lf of a one-frame run whose L is Lf, the same correctly rounded operations on the same operands."""
    return judge(ground(pos, joints, contacts, details=True, **kw))


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 2, 1), (1, 2, 2), (1, 2, 7), (2, 3, 5), (1, 5, 70), (2, 3, 150), (1, 2, 1125)]
JUMP = 0.2                                                   # metres at the top of the jump
_cache = {}


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r, axis=-1)[..., None, None]
    Kx = np.zeros(r.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -r[..., 2], r[..., 1], r[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -r[..., 0], -r[..., 1], r[..., 0]
    s = np.sin(th) / np.where(th < 1e-9, 1.0, th)
    c = (1 - np.cos(th)) / np.where(th < 1e-9, 1.0, th) ** 2
    return np.eye(3) + s * Kx + c * (Kx @ Kx)


def fk64(q, pos):
    """q (..., 24, 3), pos (..., 3) -> world positions (..., 24, 3), float64, SMPL's tree (y up)"""
    local = rodrigues(q)
    off = np.asarray(SMPL_OFFSETS, np.float32).astype(np.float64)
    P, W = [None] * 24, [None] * 24
    for j in range(24):
        p = G.SMPL_PARENTS[j]
        if p < 0:
            P[j], W[j] = np.asarray(pos, np.float64), local[..., j, :, :]
        else:
            P[j] = P[p] + W[p] @ off[j]
            W[j] = W[p] @ local[..., j, :, :]
    return np.stack(P, -2)


def windows(T):
    """the unplanted frames of the seeded contacts: a short gap (bridged), a long one around the jump (faded), one around the capped
    frame; -> (gap, jump frames or None, dip frame or None, capped frame or None, NaN frame or None)"""
    gap = np.zeros(T, bool)
    gap[T // 4:T // 4 + 3] = True
    jump = None
    if T >= 40:
        gap[T // 2 - 12:T // 2 + 13] = True
        jump = np.arange(T // 2 - 3, T // 2 + 4)
    gap[max(0, 3 * T // 4 - 1):3 * T // 4 + 2] = True
    return gap, jump, (T // 4 + 1 if T >= 7 else None), (3 * T // 4 if T >= 7 else None), (T // 3 if T >= 5 else None)


def seeded(b, dn, T):
    """-> pos (b, T dn, 3), joints (b, dn, T, 24, 3), contacts (b, dn, T, 4), float32, z up, read-only, cached.  footlock_ref.motion's
    dancers through SMPL's forward kinematics, each levelled so that the median of its body lows is 0, then: dancer 0 sunk
    3 cm throughout, dancer 1 floating 4 cm with a jump of 20 cm in the middle of a long unplanted stretch (10 cm up) and a hand dipping 5 cm
    below the floor on one unplanted frame, dancer 0's other hand 0.8 m below it on one frame (more than max_lift), one frame of the
    last dancer not finite, and in clips of two or more the last clip with no planted frame.  The contacts alternate the feet in
    steps of 6 frames, through ankle and toe channels."""
    key = (b, dn, T)
    if key in _cache:
        return _cache[key]
    J = np.zeros((b, dn, T, 24, 3))
    C = np.zeros((b, dn, T, 4), np.float32)
    radii = G.capsule_radii()
    gap, jump, dip, deep, bad = windows(T)
    t = np.arange(T)
    for c in range(b):
        q, root = FR.motion(T, seed=1000 + 97 * c + 13 * dn + T, dn=dn)
        P = fk64(q.reshape(T, dn, 24, 3), root.reshape(T, dn, 3))
        P = np.moveaxis(P, 1, 0)[..., [0, 2, 1]]               # (dn, T, 24, 3), the y up of SMPL made z
        for d in range(dn):
            left = (((t // 6 + d) % 2 == 0) | (t % 6 == 0)) & ~gap
            right = (((t // 6 + d) % 2 == 1) | (t % 6 == 0)) & ~gap
            if b >= 2 and c == b - 1:
                left[:] = right[:] = False
            C[c, d, :, 0] = np.where(left & (t % 3 != 0), 1.0, 0.0)
            C[c, d, :, 2] = np.where(left & (t % 3 == 0), 1.0, 0.0)
            C[c, d, :, 1] = np.where(right & (t % 3 != 1), 1.0, 0.0)
            C[c, d, :, 3] = np.where(right & (t % 3 == 1), 1.0, 0.0)
            Z = P[d, :, :, 2] - np.median(lows(P[d].astype(np.float32), 2, radii, G.SMPL_PARENTS)[0])
            if d == 0:
                Z = Z - 0.03
                if deep is not None:
                    Z[deep, 21] = -0.8
            if d == 1:
                Z = Z + 0.04
                if jump is not None:                              # the long gap 6 cm higher still, the jump on top of it
                    Z[T // 2 - 12:T // 2 + 13] = Z[T // 2 - 12:T // 2 + 13] + 0.06
                    Z[jump] = Z[jump] + (JUMP * np.sin(np.pi * (np.arange(jump.size) + 1) / (jump.size + 1)))[:, None]
                if dip is not None:
                    Z[dip, 20] = -0.05
            P[d, :, :, 2] = Z
        J[c] = P
    J = J.astype(np.float32)
    if bad is not None:
        J[:, dn - 1, bad, 15, 0] = np.nan
    pos = np.ascontiguousarray(np.moveaxis(J[:, :, :, 0], 1, 2).reshape(b, T * dn, 3))
    J, C = np.ascontiguousarray(J), np.ascontiguousarray(C)
    for a in (pos, J, C):
        a.setflags(write=False)
    _cache[key] = (pos, J, C)
    return _cache[key]


def permuted(pos, joints, contacts, up):
    """the same motion with the axis `up` up instead of z: the components (floor 0, floor 1, up) = (x, y, z) of the input"""
    order = {0: [2, 0, 1], 1: [0, 2, 1], 2: [0, 1, 2]}[up]
    return np.ascontiguousarray(pos[..., order]), np.ascontiguousarray(joints[..., order]), contacts


def variants():
    """(name, contacts given, floor) of the runs of every seeded shape: the floor estimated and given, contacts given and None"""
    return [("contacts", True, None), ("contacts, floor 0.01", True, 0.01), ("still rule", False, None), ("still rule, floor 0", False, 0.0)]


def parameter_cases():
    """(name, (pos, joints, contacts), keyword arguments) of the GPU test's runs with other parameters; tests/test_ground_cpu.py holds
    each to decisions_clear"""
    base = seeded(1, 5, 70)
    return [("blend=0", base, dict(blend=0)), ("blend>T", seeded(2, 3, 5), dict(blend=9)), ("up=1", permuted(*base, 1), dict(up=1)),
            ("max_lift=0.1", base, dict(max_lift=0.1)), ("tolerance=0.02", base, dict(tolerance=0.02))]
