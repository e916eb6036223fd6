"""numpy float64 restatement of the geometric (relational) features of tcdiff_amd/set_metrics.py (csrc/geometric.hip, csrc/geo_math.h),
written from the text of include/tcdiff_hip_ext.h with its own copy of the 32-row table, and the seeded inputs the CPU and GPU
tests share.  Beside the features it returns the smallest *margin* over all decisions it took -- |v - lo| / |lo| for the threshold
kinds, the distance to the nearer bound / 180 for angles -- so that a test can show, on the restatement alone, that no decision is
a near-tie before it asks another implementation for the same bits."""
import numpy as np

import set_metrics_ref as SR

PLANE, NPLANE, MOVE, NMOVE, ANGLE, FAST = range(6)
KINDS = ("PLANE", "NPLANE", "MOVE", "NMOVE", "ANGLE", "FAST")
(ROOT, LHIP, RHIP, BELLY, LKNEE, RKNEE, SPINE, LANKLE, RANKLE, CHEST, LTOES, RTOES, NECK, LINSHOULDER, RINSHOULDER, HEAD, LSHOULDER,
 RSHOULDER, LELBOW, RELBOW, LWRIST, RWRIST, LHAND, RHAND, ZERO, UP, NUP, FLOOR) = range(28)
MIN_MARGIN = 1e-9

_LSHOULDER = np.array([0.199113488, 0.236807942, -0.0180702247])
_LELBOW = np.array([0.454445392, 0.221158922, -0.0410167128])
_RSHOULDER = np.array([-0.191692337, 0.236928746, -0.0123055102])
_LHIP = np.array([0.0564076714, -0.323069185, 0.0109197125])
_RHIP = np.array([-0.0624834076, -0.331302464, 0.0150412619])
HL = float(np.sqrt(((_LSHOULDER - _LELBOW) ** 2).sum()))
SW = float(np.sqrt(((_LSHOULDER - _RSHOULDER) ** 2).sum()))
HW = float(np.sqrt(((_LHIP - _RHIP) ** 2).sum()))

# (kind, a, b, c, p, lo, hi); hi of a threshold row repeats lo and is not read; MOVE does not read c, FAST reads only p
ROWS = [
    (NMOVE, NECK, RHIP, LHIP, RWRIST, 1.8 * HL, None),
    (NMOVE, NECK, LHIP, RHIP, LWRIST, 1.8 * HL, None),
    (NPLANE, CHEST, NECK, NECK, RWRIST, 0.2 * HL, None),
    (NPLANE, CHEST, NECK, NECK, LWRIST, 0.2 * HL, None),
    (MOVE, BELLY, CHEST, RWRIST, CHEST, 1.8 * HL, None),
    (MOVE, BELLY, CHEST, LWRIST, CHEST, 1.8 * HL, None),
    (ANGLE, RELBOW, RSHOULDER, RELBOW, RWRIST, 0.0, 110.0),
    (ANGLE, LELBOW, LSHOULDER, LELBOW, LWRIST, 0.0, 110.0),
    (NPLANE, LSHOULDER, RSHOULDER, LWRIST, RWRIST, 2.5 * SW, None),
    (MOVE, LWRIST, RWRIST, LWRIST, RWRIST, 1.4 * HL, None),
    (MOVE, RWRIST, ROOT, ROOT, LWRIST, 1.4 * HL, None),
    (MOVE, LWRIST, ROOT, ROOT, RWRIST, 1.4 * HL, None),
    (FAST, RWRIST, RWRIST, RWRIST, RWRIST, 2.5 * HL, None),
    (FAST, LWRIST, LWRIST, LWRIST, LWRIST, 2.5 * HL, None),
    (PLANE, ROOT, LHIP, LTOES, RANKLE, 0.38 * HL, None),
    (PLANE, ROOT, RHIP, RTOES, LANKLE, 0.38 * HL, None),
    (NPLANE, ZERO, UP, FLOOR, RANKLE, 1.2 * HL, None),
    (NPLANE, ZERO, UP, FLOOR, LANKLE, 1.2 * HL, None),
    (NPLANE, LHIP, RHIP, LANKLE, RANKLE, 2.1 * HW, None),
    (ANGLE, RKNEE, RHIP, RKNEE, RANKLE, 0.0, 110.0),
    (ANGLE, LKNEE, LHIP, LKNEE, LANKLE, 0.0, 110.0),
    (FAST, RANKLE, RANKLE, RANKLE, RANKLE, 2.5 * HL, None),
    (FAST, LANKLE, LANKLE, LANKLE, LANKLE, 2.5 * HL, None),
    (ANGLE, NECK, ROOT, RSHOULDER, RELBOW, 25.0, 180.0),
    (ANGLE, NECK, ROOT, LSHOULDER, LELBOW, 25.0, 180.0),
    (ANGLE, NECK, ROOT, RHIP, RKNEE, 50.0, 180.0),
    (ANGLE, NECK, ROOT, LHIP, LKNEE, 50.0, 180.0),
    (PLANE, RANKLE, NECK, LANKLE, ROOT, 0.5 * HL, None),
    (ANGLE, NECK, ROOT, ZERO, UP, 70.0, 110.0),
    (NPLANE, ZERO, NUP, FLOOR, RWRIST, -1.2 * HL, None),
    (NPLANE, ZERO, NUP, FLOOR, LWRIST, -1.2 * HL, None),
    (FAST, ROOT, ROOT, ROOT, ROOT, 2.3 * HL, None),
]


def default_table():
    """-> table (32, 5) int32, range (32, 2) float64"""
    table = np.array([r[:5] for r in ROWS], np.int32)
    rng = np.array([[r[5], r[5] if r[6] is None else r[6]] for r in ROWS], np.float64)
    return table, rng


# ---- the definitions ---------------------------------------------------------------------------------------------------------
def points(J, up):
    """(T, 24, 3) joints -> (T, 28, 3) float64: the joints, zero, up, -up, floor"""
    J = np.asarray(J, np.float64)
    P = np.zeros((J.shape[0], 28, 3))
    P[:, :24] = J
    P[:, UP, up] = 1.0
    P[:, NUP, up] = -1.0
    with np.errstate(invalid="ignore"):
        P[:, FLOOR, up] = np.min(J[:, :, up], axis=1)                  # (NaN if one of them is NaN)
    return P


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def norm(x):
    return np.sqrt(dot(x, x))


def values(row, P, tau):
    """the row's v at the frames t = 1 .. T - 1 of the points P (T, 28, 3)"""
    kind, ia, ib, ic, ip = (int(x) for x in row)
    a, b, c, p = P[1:, ia], P[1:, ib], P[1:, ic], P[1:, ip]
    a0, p0 = P[:-1, ia], P[:-1, ip]
    with np.errstate(all="ignore"):
        if kind == PLANE:
            n = cross(c - a, b - a)
            return dot(n, p - a) / norm(n)
        if kind == NPLANE:
            n = b - a
            return dot(n, p - c) / norm(n)
        if kind in (MOVE, NMOVE):
            w = (p - a) - (p0 - a0)
            n = b - a if kind == MOVE else cross(c - a, b - a)
            return dot(w, n) / norm(n) / tau
        if kind == ANGLE:
            u, w = b - a, p - c
            cs = dot(u, w) / (norm(u) * norm(w))
            cs = np.where(cs > 1.0, 1.0, np.where(cs < -1.0, -1.0, cs))
            return np.arccos(cs) * (180.0 / np.pi)
        if kind == FAST:
            return norm(p - p0) / tau
    raise ValueError(kind)


def one_dancer(J, up=2, tau=1 / 120, table=None, rng=None):
    """(T, 24, 3) float32 -> counts (R,) int64 and the smallest margin of a decision (inf if none was taken)"""
    if table is None:
        table, rng = default_table()
    R = len(table)
    counts, margin = np.zeros(R, np.int64), np.inf
    if J.shape[0] < 2:
        return counts, margin
    P = points(J, up)
    for r in range(R):
        kind = int(table[r][0])
        if not (0 <= kind < 6 and all(0 <= int(i) < 28 for i in table[r][1:])):
            continue                                                   # counts nothing
        v = values(table[r], P, tau)
        lo, hi = float(rng[r][0]), float(rng[r][1])
        fin = np.isfinite(v)
        with np.errstate(invalid="ignore"):
            holds = fin & (v > lo) & ((v < hi) if kind == ANGLE else True)
        counts[r] = int(holds.sum())
        if fin.any():
            if kind == ANGLE:
                m = np.minimum(np.abs(v[fin] - lo), np.abs(v[fin] - hi)) / 180.0
            else:
                m = np.abs(v[fin] - lo) / (abs(lo) if lo != 0.0 else 1.0)
            margin = min(margin, float(m.min()))
    return counts, margin


def geometric_features(joints, up=2, tau=1 / 120, table=None, rng=None):
    """(b, dn, T, 24, 3) float32 -> features (b, dn, R) float64 (NaN for T < 2), counts (b, dn, R) int64, the smallest margin"""
    b, dn, T = joints.shape[:3]
    R = 32 if table is None else len(table)
    counts, margin = np.zeros((b, dn, R), np.int64), np.inf
    for c in range(b):
        for d in range(dn):
            counts[c, d], m = one_dancer(joints[c, d], up, tau, table, rng)
            margin = min(margin, m)
    feats = counts.astype(np.float64) / np.float64(T - 1) if T >= 2 else np.full((b, dn, R), np.nan)
    return feats, counts, margin


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------
SEED = 5
# family A: set_metrics_ref.synth_joints as it is, at 1 / 120 s per frame; family B: its positions doubled, at 1 / 8 s per frame
# (without it row 8 never fires and the FAST rows are almost always 1)
CASES = [("A", (1, 1, 1)), ("A", (1, 1, 2)), ("A", (2, 3, 4)), ("A", (1, 2, 5)), ("A", (1, 2, 64)), ("A", (1, 2, 65)),
         ("A", (1, 1, 66)), ("A", (1, 1, 129)), ("A", (2, 3, 150)), ("A", (1, 1, 600)), ("A", (1, 2, 257)), ("B", (2, 3, 40)),
         ("B", (1, 2, 65))]
TAU = {"A": 1 / 120, "B": 1 / 8}
_cache = {}


def case_joints(family, shape):
    J = SR.synth_joints(*shape, seed=SEED)
    return J if family == "A" else (J * np.float32(2.0)).astype(np.float32)


def case(family, shape):
    """-> joints, tau, (features, counts, margin) of the default table; computed once and left unchanged"""
    key = (family, shape)
    if key not in _cache:
        J = case_joints(family, shape)
        J.setflags(write=False)
        _cache[key] = (J, TAU[family], geometric_features(J, 2, TAU[family]))
    return _cache[key]


def case_id(c):
    return c[0] + "-" + "x".join(map(str, c[1]))
