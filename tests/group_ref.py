"""numpy float64 restatement of include/tcdiff_group.h, written from the header: loops over clips, pairs and frames; the 529 bone
pairs of a frame are evaluated elementwise as arrays (every numpy operation rounds once, as the header's arithmetic does).
Seeded inputs for the GPU test and the check that no decision the metrics make on them is a near-tie."""
import numpy as np

SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
DEFAULTS = dict(fps=30, up=2, radii=None, parents=None, window=None, max_lag=15, sigma_floor=1e-6)
SMALL = 1e-18
MARGIN = 1e-9


def capsule_radii():
    r = np.zeros(24)
    for value, bones in ((0.10, (1, 2)), (0.075, (4, 5)), (0.05, (7, 8)), (0.04, (10, 11)), (0.13, (3, 6, 9)), (0.06, (12,)),
                         (0.07, (13, 14)), (0.10, (15,)), (0.06, (16, 17)), (0.045, (18, 19)), (0.04, (20, 21)), (0.035, (22, 23))):
        r[list(bones)] = value
    return r


def pairs(dn):
    return [(a, b) for a in range(dn) for b in range(a + 1, dn)]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def clamp(x):
    return np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))


def seg_dist(p1, q1, p2, q2):
    """the header's clamped closest-point construction, elementwise over the leading dimensions of (..., 3) float64 arrays"""
    p1, q1, p2, q2 = (np.asarray(v, np.float64) for v in (p1, q1, p2, q2))
    with np.errstate(all="ignore"):
        d1, d2, r = q1 - p1, q2 - p2, p1 - p2
        A, E, F, C, B = dot(d1, d1), dot(d2, d2), dot(d2, r), dot(d1, r), dot(d1, d2)
        a_small, e_small = A <= SMALL, E <= SMALL
        den = A * E - B * B
        s = np.where(den > 0.0, clamp((B * F - C * E) / den), 0.0)
        u = (B * s + F) / E
        s = np.where(u < 0.0, clamp(-C / A), np.where(u > 1.0, clamp((B - C) / A), s))
        u = np.where(u < 0.0, 0.0, np.where(u > 1.0, 1.0, u))
        s = np.where(a_small, 0.0, np.where(e_small, clamp(-C / A), s))
        u = np.where(e_small, 0.0, np.where(a_small, clamp(F / E), u))
        c1 = p1 + s[..., None] * d1
        c2 = p2 + u[..., None] * d2
        diff = c1 - c2
        return np.sqrt(dot(diff, diff))


def frame_gaps(Ja, Jb, radii, parents):
    """the 23 x 23 gaps of one frame: Ja, Jb (24, 3) float32 -> (23, 23) float64, entry [i - 1, j - 1]"""
    Ja, Jb = np.asarray(Ja).astype(np.float64), np.asarray(Jb).astype(np.float64)
    bones = np.arange(1, 24)
    par = np.asarray(parents)[bones]
    d = seg_dist(Ja[par][:, None, :], Ja[bones][:, None, :], Jb[par][None, :, :], Jb[bones][None, :, :])
    return (d - radii[bones][:, None]) - radii[bones][None, :]


def frame_min(g):
    """(gap, code, runner-up) of a frame: a NaN precedes every number, then the smaller value, then the smaller code"""
    flat = g.reshape(-1)                                     # ascending code: entry 23 (i - 1) + (j - 1)
    nan = np.isnan(flat)
    k = int(np.argmax(nan)) if nan.any() else int(np.argmin(flat))          # both give the first such entry
    second = np.inf if nan.any() else float(np.partition(flat, 1)[1])
    return flat[k], 24 * (k // 23 + 1) + (k % 23 + 1), second


def floor_of(J, up):
    """(T, 24, 3) -> the root's two floor coordinates (T, 2) float64, in axis order"""
    keep = [k for k in range(3) if k != up]
    return np.asarray(J)[:, 0, keep].astype(np.float64)


def orient(x, y, z):
    return (y[..., 0] - x[..., 0]) * (z[..., 1] - x[..., 1]) - (y[..., 1] - x[..., 1]) * (z[..., 0] - x[..., 0])


def crossings_of(pa, pb, window, values=None):
    """the crossing steps (t, s) of two floor paths (T, 2); ``values`` collects every orientation value"""
    N = pa.shape[0] - 1
    out = []
    for t in range(N):
        a0, a1 = pa[t], pa[t + 1]
        lo, hi = max(0, t - window), min(N - 1, t + window)
        b0, b1 = pb[lo:hi + 1], pb[lo + 1:hi + 2]          # the steps s = lo .. hi of b, elementwise
        o = (orient(a0, a1, b0), orient(a0, a1, b1), orient(b0, b1, a0), orient(b0, b1, a1))
        if values is not None:
            values.extend(np.concatenate(o).tolist())
        hit = (o[0] * o[1] < 0.0) & (o[2] * o[3] < 0.0)
        out.extend((t, lo + int(k)) for k in np.flatnonzero(hit))
    return out


def speeds(J):
    """(T, 24, 3) float32 -> x (24, N): the root's speed and the root-relative speeds of the other joints"""
    J = np.asarray(J).astype(np.float64)
    rel = J - J[:, :1]
    rel[:, 0] = J[:, 0]
    d = rel[1:] - rel[:-1]                                  # (J[t + 1, j] - J[t + 1, 0]) - (J[t, j] - J[t, 0]); the root as it is
    return np.sqrt(dot(d, d)).T


def standardise(x):
    """x (24, N) -> z (24, N), sigma (24,)"""
    with np.errstate(all="ignore"):
        N = x.shape[1]
        mu = x.sum(1) / N if N else np.full(24, np.nan)
        sigma = np.sqrt(((x - mu[:, None]) ** 2).sum(1) / N) if N else np.full(24, np.nan)
        return (x - mu[:, None]) / sigma[:, None], sigma


def lag_range(T, max_lag):
    N = T - 1
    return -1 if N < 2 else min(max_lag, N - 2)


def better_lag(R, lag, best, best_lag):
    if R != best:
        return R > best
    if abs(lag) != abs(best_lag):
        return abs(lag) < abs(best_lag)
    return lag < best_lag


def sync_of(za, sa, zb, sb, T, max_lag, sigma_floor):
    """-> sync, lag, sync_zero, {lag: R}, participating joints"""
    L = lag_range(T, max_lag)
    part = [j for j in range(24) if sa[j] > sigma_floor and sb[j] > sigma_floor]
    if L < 0 or not part:
        return np.nan, 0, np.nan, {}, part
    N = T - 1
    R = {}
    for l in range(-L, L + 1):
        lo, hi = max(0, -l), min(N, N - l)
        total = 0.0
        for j in part:
            total = total + float(np.sum(za[j, lo:hi] * zb[j, lo + l:hi + l])) / (N - abs(l))
        R[l] = total / len(part)
    best, best_lag = R[-L], -L
    for l in range(-L + 1, L + 1):
        if better_lag(R[l], l, best, best_lag):
            best, best_lag = R[l], l
    return best, best_lag, R[0], R, part


def group_metrics(joints, *, fps=30, up=2, radii=None, parents=None, window=None, max_lag=15, sigma_floor=1e-6, details=False):
    """joints (b, dn, T, 24, 3) float32 -> the dictionary of tcdiff_amd.group_metrics.group_metrics with return_frames, as numpy
    arrays; ``details`` adds what decisions_clear looks at"""
    joints = np.asarray(joints)
    assert joints.dtype == np.float32 and joints.shape[3:] == (24, 3)
    b, dn, T = joints.shape[:3]
    radii = capsule_radii() if radii is None else np.asarray(radii, np.float64)
    parents = SMPL_PARENTS if parents is None else list(parents)
    window = int(round(fps)) if window is None else window
    pr = pairs(dn)
    P = len(pr)
    out = {"body_contact_rate": np.zeros((b, P)), "body_gap_min": np.zeros((b, P)), "body_contact_episodes": np.zeros((b, P), np.int64),
           "body_closest": np.zeros((b, P, 3), np.int64), "path_crossings": np.zeros((b, P), np.int64),
           "path_crossing_rate": np.zeros((b, P)), "sync": np.zeros((b, P)), "sync_lag": np.zeros((b, P), np.int64),
           "sync_zero": np.zeros((b, P)), "gap": np.zeros((b, P, T)), "closest": np.zeros((b, P, T), np.int32)}
    det = {"frame_lead": np.inf, "pair_lead": np.inf, "orient": [], "sigma_in": [], "sigma_out": [], "lag_lead": np.inf}
    for c in range(b):
        zs = [standardise(speeds(joints[c, d])) for d in range(dn)]
        for p, (a, bb) in enumerate(pr):
            # 1. the body gap
            for t in range(T):
                g, code, second = frame_min(frame_gaps(joints[c, a, t], joints[c, bb, t], radii, parents))
                out["gap"][c, p, t], out["closest"][c, p, t] = g, code
                if np.isfinite(g):
                    det["frame_lead"] = min(det["frame_lead"], second - g)
            gap = out["gap"][c, p]
            neg = gap < 0.0
            out["body_contact_rate"][c, p] = neg.sum() / T
            out["body_contact_episodes"][c, p] = sum(1 for t in range(T) if neg[t] and not (t > 0 and neg[t - 1]))
            best_t = -1
            for t in range(T):
                if np.isfinite(gap[t]) and (best_t < 0 or gap[t] < gap[best_t]):
                    best_t = t
            if best_t < 0:
                out["body_gap_min"][c, p], out["body_closest"][c, p] = np.nan, (-1, -1, -1)
            else:
                code = int(out["closest"][c, p, best_t])
                out["body_gap_min"][c, p], out["body_closest"][c, p] = gap[best_t], (best_t, code // 24, code % 24)
                others = [gap[t] for t in range(T) if t != best_t and np.isfinite(gap[t])]
                if others:
                    det["pair_lead"] = min(det["pair_lead"], min(others) - gap[best_t])
            # 2. the crossings
            hits = crossings_of(floor_of(joints[c, a], up), floor_of(joints[c, bb], up), window, det["orient"] if details else None)
            out["path_crossings"][c, p] = len(hits)
            out["path_crossing_rate"][c, p] = len(hits) / (T - 1) if T >= 2 else 0.0
            # 3. synchrony
            (za, sa), (zb, sb) = zs[a], zs[bb]
            s, lag, s0, R, part = sync_of(za, sa, zb, sb, T, max_lag, sigma_floor)
            out["sync"][c, p], out["sync_lag"][c, p], out["sync_zero"][c, p] = s, lag, s0
            if T >= 2:
                for j in range(24):
                    (det["sigma_in"] if j in part else det["sigma_out"]).extend([sa[j], sb[j]] if j in part else
                                                                                 [v for v in (sa[j], sb[j]) if not v > sigma_floor])
            if len(R) > 1:
                ranked = sorted(R.values(), reverse=True)
                det["lag_lead"] = min(det["lag_lead"], ranked[0] - ranked[1])
    if details:
        out["details"] = det
    return out


def judge(ref, sigma_floor=1e-6):
    """(ok, reasons) from a group_metrics(..., details=True) result; see decisions_clear"""
    det = ref["details"]
    gap = ref["gap"][np.isfinite(ref["gap"])]
    why = []
    if gap.size and np.abs(gap).min() <= MARGIN:
        why.append(f"a gap of {np.abs(gap).min():.3e}")
    if det["frame_lead"] <= MARGIN:
        why.append(f"a frame's smallest gap leads by {det['frame_lead']:.3e}")
    if det["pair_lead"] <= MARGIN:
        why.append(f"a pair's smallest gap leads by {det['pair_lead']:.3e}")
    o = np.abs(np.asarray(det["orient"], np.float64))
    o = o[~np.isnan(o)]
    if o.size and ((o != 0.0) & (o <= MARGIN)).any():
        why.append(f"an orientation value of {o[o != 0.0].min():.3e}")
    if det["sigma_in"] and min(det["sigma_in"]) <= 10.0 * sigma_floor:
        why.append(f"a participating sigma of {min(det['sigma_in']):.3e}")
    bad = [v for v in det["sigma_out"] if not (v == 0.0 or np.isnan(v))]
    if bad:
        why.append(f"an excluded sigma of {bad[0]:.3e}")
    if det["lag_lead"] <= MARGIN:
        why.append(f"the best lag leads by {det['lag_lead']:.3e}")
    return not why, why


def decisions_clear(joints, **kw):
    """No comparison the metrics make is a near-tie on these inputs, so an implementation that rounds differently in the last places
    still makes every decision the same way: every |gap| above 1e-9; the smallest gap of a frame and of a pair ahead of its runner-up
    by more than 1e-9; every orientation value exactly 0 or above 1e-9 in magnitude; every participating sigma above 10 sigma_floor and
    every excluded one exactly 0 (a NaN input aside); the best R(l) ahead of the runner-up by more than 1e-9.  Returns (ok, reasons)."""
    return judge(group_metrics(joints, details=True, **kw), dict(DEFAULTS, **kw)["sigma_floor"])


# ---- bodies that can be checked by hand -----------------------------------------------------------------------------------------------------------
def point_dancer(at, T=1):
    """every joint at one point: 23 bones of no length"""
    return np.broadcast_to(np.asarray(at, np.float32), (T, 24, 3)).copy()


def stick_dancer(x, T=1):
    """an upright body on the vertical through (x, 0): joint j at height j / 8, exactly representable"""
    J = np.zeros((T, 24, 3), np.float32)
    J[:, :, 0] = x
    J[:, :, 2] = np.arange(24, dtype=np.float32) / 8
    return J


def stepper(steps):
    """a rigid upright dancer whose root advances along x by the given steps (multiples of 1 / 64: exact in float32)"""
    x = np.concatenate([[0.0], np.cumsum(steps)])
    J = stick_dancer(0.0, T=len(x))
    J[:, :, 0] = x.astype(np.float32)[:, None]
    assert (np.diff(J[:, 0, 0].astype(np.float64)) == np.asarray(steps)).all()
    return J


def clip(*dancers):
    return np.stack(dancers)[None]


# ---- radii from a body model ------------------------------------------------------------------------------------------------------------------
def radii_from_body(v, J, w, parents):
    """rest-pose vertices (V, 3), joints (24, 3), dense weights (V, 24): loops, float64"""
    v, J, w = np.asarray(v, np.float64), np.asarray(J, np.float64), np.asarray(w, np.float64)
    near = {i: [] for i in range(1, 24)}
    for n in range(v.shape[0]):
        k = int(np.argmax(w[n]))
        cand = []
        for i in range(1, 24):
            if parents[i] == k or i == k:
                p, q = J[parents[i]], J[i]
                d = q - p
                dd = d @ d
                s = 0.0 if dd <= SMALL else min(1.0, max(0.0, ((v[n] - p) @ d) / dd))
                cand.append((np.linalg.norm(v[n] - (p + s * d)), i))
        if cand:
            dist, i = min(cand)
            near[i].append(dist)
    r = capsule_radii()
    for i in range(1, 24):
        if near[i]:
            r[i] = np.median(near[i])
    return r


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 2, 1), (1, 2, 2), (1, 2, 3), (2, 3, 5), (1, 5, 70), (2, 3, 150), (1, 2, 1125)]
SEEDS = {(1, 2, 1): 0, (1, 2, 2): 0, (1, 2, 3): 0, (2, 3, 5): 0, (1, 5, 70): 0, (2, 3, 150): 0, (1, 2, 1125): 0}
DELAY = 4                                                   # frames by which the copied dancer trails
# a rest pose with z up, arms hanging a little forward of the sides (metres): a body, not a cloud of points
_REST = np.array([[0.0, 0.0, 0.0], [0.06, 0.0, -0.08], [-0.06, 0.0, -0.09], [0.0, -0.03, 0.12], [0.10, 0.0, -0.47], [-0.10, 0.0, -0.47],
                  [0.0, -0.01, 0.26], [0.09, -0.03, -0.90], [-0.09, -0.03, -0.89], [0.0, -0.01, 0.32], [0.13, 0.09, -0.96],
                  [-0.13, 0.10, -0.95], [0.0, -0.04, 0.53], [0.07, -0.03, 0.43], [-0.08, -0.03, 0.43], [0.01, 0.01, 0.62],
                  [0.19, -0.05, 0.47], [-0.19, -0.04, 0.48], [0.30, -0.02, 0.24], [-0.31, -0.03, 0.24], [0.36, 0.12, 0.02],
                  [-0.37, 0.13, 0.03], [0.38, 0.17, -0.06], [-0.39, 0.18, -0.05]])
SPINE = ((3, 0.12), (6, 0.26), (9, 0.32))                  # joint, metres along the spine from the root
_cache = {}


def synth(b, dn, T, seed=None):
    """Seeded dancers at metre scale, (b, dn, T, 24, 3) float32, z up: roots on smooth closed paths around a shared centre, so that
    the paths cross and the bodies meet now and then; limbs posed by smooth waves about a rest pose.  Dancer 1 of every clip is dancer
    0 shifted aside and delayed by DELAY frames, plus noise of a millimetre; with three or more dancers the last one stands still
    (the same float32 words in every frame).  The spine (joints 0, 3, 6, 9) is kept straight: its three bones have one radius, and
    beside a bent spine lies a wedge of space whose nearest point on two of them is the joint they share -- there the two gaps are
    equal to the last bit and the smallest code decides, which tests/test_group_cpu.py and a hand-made case of the GPU test check,
    while the comparison on these inputs wants every minimum to lead by a margin.  Cached; treat as read-only."""
    seed = SEEDS.get((b, dn, T), 0) if seed is None else seed
    key = (b, dn, T, seed)
    if key in _cache:
        return _cache[key]
    g = np.random.default_rng([seed, b, dn, T])
    n = T + DELAY
    sec = (np.arange(n, dtype=np.float64) - DELAY).reshape(n, 1, 1) / 30.0

    def waves(shape, amp, f_lo, f_hi, k=3):
        f, ph = g.uniform(f_lo, f_hi, (k, 1) + shape), g.uniform(0, 2 * np.pi, (k, 1) + shape)
        return (g.uniform(0.3, 1.0, (k, 1) + shape) * amp / k * np.sin(2 * np.pi * f * sec[None] + ph)).sum(0)

    out = np.zeros((b, dn, T, 24, 3))
    for c in range(b):
        for d in range(dn):
            root = waves((1, 3), 0.9, 0.15, 0.5) * np.array([1.0, 1.0, 0.05]) + np.array([0.0, 0.0, 0.95])
            root = root + g.uniform(-0.25, 0.25, (1, 1, 3)) * np.array([1.0, 1.0, 0.0])
            body = _REST[None] + waves((24, 3), 0.16, 0.4, 1.6)
            body[:, 0] = 0.0
            lean = np.array([0.0, -0.05, 1.0]) + waves((1, 3), 0.25, 0.3, 1.0) * np.array([1.0, 1.0, 0.0])
            for j, along in SPINE:                        # a straight spine that leans: see the docstring
                body[:, j] = along * lean[:, 0]
            turn = g.uniform(0, 2 * np.pi)
            rot = np.array([[np.cos(turn), -np.sin(turn), 0.0], [np.sin(turn), np.cos(turn), 0.0], [0.0, 0.0, 1.0]])
            J = root + body @ rot.T                                                   # (n, 24, 3)
            if d == 1:
                noise, bend = g.normal(0.0, 1e-3, (T, 24, 3)), g.normal(0.0, 3e-3, (T, 3))
                for j, along in SPINE:                                                # the noise leaves the spine straight
                    noise[:, j] = noise[:, 0] + along * bend
                J = out_full[0][:n - DELAY] + np.array([0.45, 0.2, 0.0]) + noise
                out[c, d] = J
                continue
            if d == dn - 1 and dn >= 3:
                J = np.broadcast_to(J[DELAY + T // 2], (n, 24, 3))
            if d == 0:
                out_full = [J]
            out[c, d] = J[DELAY:]
    _cache[key] = np.ascontiguousarray(out.astype(np.float32))
    _cache[key].setflags(write=False)
    return _cache[key]


def custom_skeleton():
    """another valid tree (every parent before its child) and seeded radii between 2 and 15 cm, for the tests of other parameters"""
    g = np.random.default_rng(24)
    parents = [-1] + [int(g.integers(max(0, j - 3), j)) for j in range(1, 24)]
    return parents, np.concatenate([[0.0], g.uniform(0.02, 0.15, 23)])


def parameter_cases():
    """(shape, keyword arguments) of the GPU test's runs with other parameters; tests/test_group_cpu.py holds each to decisions_clear"""
    parents, radii = custom_skeleton()
    shape = (1, 5, 70)
    return [(shape, dict(up=1, window=0, max_lag=0)), (shape, dict(window=200, max_lag=64, fps=60)),
            (shape, dict(radii=radii, parents=parents, fps=60, sigma_floor=1e-5))]
