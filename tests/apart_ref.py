"""numpy float64 restatement of include/tcdiff_apart.h, written from the header: loops over clips, rounds and pairs; the frames of a
pair and their 529 bone pairs are evaluated elementwise as arrays (every numpy operation rounds once, as the header's arithmetic
does).  The distance is tests/group_ref.py's, imported, not edited.  Seeded inputs for the GPU test and the check that no decision the
construction makes on them is a near-tie."""
import numpy as np

import group_ref as G

DEFAULTS = dict(up=2, radii=None, parents=None, margin=0.02, iterations=8, rounds=3, blend=5, max_push=0.6, mobility=None)
SMALL = 1e-18
GUARD = 1e-9
# the bound the GPU tests hold the float64 outputs to (tests/test_apart_gpu.py, tests/test_post_chain_gpu.py)
MEASURED = 0.0            # metres: the largest difference of a float64 output from the restatement over every case of tests/test_apart_gpu.py (profiles/apart.txt)
FLOAT_BOUND = min(100 * MEASURED, 1e-9)
ROUNDING_GUARD = 1e-14                                      # a hundred times what two float64 evaluations of a shift differ by


def floor_axes(up):
    return [k for k in range(3) if k != up]


def gaps(Ja, Jb, radii, parents):
    """the body gap of every frame: Ja, Jb (T, 24, 3) float64 -> (T,) float64; a NaN precedes every number"""
    bones = np.arange(1, 24)
    par = np.asarray(parents)[bones]
    d = G.seg_dist(Ja[:, par][:, :, None, :], Ja[:, bones][:, :, None, :], Jb[:, par][:, None, :, :], Jb[:, bones][:, None, :, :])
    g = ((d - radii[bones][None, :, None]) - radii[bones][None, None, :]).reshape(d.shape[0], -1)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(g).any(1), np.nan, np.min(np.where(np.isnan(g), np.inf, g), axis=1))


def moved(J, fl, q, u, sign):
    """J (T, 24, 3) with (q u) subtracted from (sign -1) or added to (sign +1) the floor components of every joint"""
    out = J.copy()
    for n, k in enumerate(fl):
        step = (q * u[:, n])[:, None]
        out[:, :, k] = J[:, :, k] - step if sign < 0 else J[:, :, k] + step
    return out


def direction(Ja, Jb, fl):
    """(T, 2) unit floor vectors from root a to root b, (1, 0) where they coincide; and n2"""
    with np.errstate(all="ignore"):
        d0, d1 = Jb[:, 0, fl[0]] - Ja[:, 0, fl[0]], Jb[:, 0, fl[1]] - Ja[:, 0, fl[1]]
        n2 = d0 * d0 + d1 * d1
        ok = n2 > SMALL
        n = np.sqrt(np.where(ok, n2, 1.0))
        return np.stack([np.where(ok, d0 / n, 1.0), np.where(ok, d1 / n, 0.0)], 1), n2


def shares(ma, mb):
    if ma == 0.0 and mb == 0.0:
        return None
    wa = ma / (ma + mb)
    return wa, 1.0 - wa


def demand(Ja, Jb, fl, w, radii, parents, margin, iterations, max_push, det=None):
    """step 1 for the T frames of a pair: Ja, Jb (T, 24, 3) float64 with the shift already added -> m, u, entry gap, pushed, capped"""
    T = Ja.shape[0]
    u, n2 = direction(Ja, Jb, fl)
    g0 = gaps(Ja, Jb, radii, parents)
    m, capped = np.zeros(T), np.zeros(T, bool)
    if det is not None:
        det["n2"].extend(n2[~np.isnan(n2)].tolist())
    if w is not None:
        g, active = g0.copy(), ~np.isnan(g0)
        for _ in range(iterations):
            with np.errstate(invalid="ignore"):
                need = margin - g
                active = active & (need > 0.0)
            if not active.any():
                break
            idx = np.flatnonzero(active)
            raw = m[idx] + need[idx]
            if det is not None:
                det["cap"].extend((raw - max_push).tolist())
            m[idx] = np.minimum(raw, max_push)
            g[idx] = gaps(moved(Ja[idx], fl, w[0] * m[idx], u[idx], -1), moved(Jb[idx], fl, w[1] * m[idx], u[idx], +1), radii, parents)
            hit = m[idx] == max_push
            capped[idx[hit]] = True
            active[idx[hit]] = False
    return m, u, g0, m > 0.0, capped


def envelope(m, blend):
    """e[t] = max over |t' - t| <= blend of m[t'] (1 - |t - t'| / (blend + 1))"""
    T = m.shape[0]
    e = m.copy()
    for k in range(1, min(blend, T - 1) + 1):
        f = 1.0 - float(k) / (float(blend) + 1.0)
        e[k:] = np.maximum(e[k:], m[:-k] * f)
        e[:-k] = np.maximum(e[:-k], m[k:] * f)
    return e


def keep_apart(pos, joints, *, dn=None, up=2, radii=None, parents=None, margin=0.02, iterations=8, rounds=3, blend=5, max_push=0.6,
               mobility=None, details=False):
    """pos (b, T dn, 3), joints (b, dn, T, 24, 3) float32 -> the fields of tcdiff_amd.apart.Apart as a dictionary of numpy arrays, with
    `shift`; ``details`` adds what decisions_clear looks at and the per-frame planes"""
    pos, joints = np.asarray(pos), np.asarray(joints)
    assert joints.dtype == np.float32 and pos.dtype == np.float32 and joints.shape[3:] == (24, 3)
    b, dn_, T = joints.shape[:3]
    assert dn in (None, dn_) and pos.shape == (b, T * dn_, 3)
    dn = dn_
    radii = G.capsule_radii() if radii is None else np.asarray(radii, np.float64)
    parents = G.SMPL_PARENTS if parents is None else list(parents)
    mobility = np.ones(dn) if mobility is None else np.asarray(mobility, np.float64)
    fl = floor_axes(up)
    pr = G.pairs(dn)
    P = len(pr)
    S = np.zeros((b, dn, T, 2))
    before, after = np.full((b, P, T), np.nan), np.full((b, P, T), np.nan)
    pushed, capped = np.zeros((b, P, T), bool), np.zeros((b, P, T), bool)
    det = {"n2": [], "entry": [], "cap": [], "round": []}
    J64 = joints.astype(np.float64)

    def shifted(c, d):
        J = J64[c, d].copy()
        for n, k in enumerate(fl):
            J[:, :, k] = J[:, :, k] + S[c, d, :, n][:, None]
        return J

    for r in range(rounds):
        for c in range(b):
            plan = []
            for p, (a, bb) in enumerate(pr):
                w = shares(mobility[a], mobility[bb])
                m, u, g0, psh, cap = demand(shifted(c, a), shifted(c, bb), fl, w, radii, parents, margin, iterations, max_push,
                                            det if details else None)
                if r == 0:
                    before[c, p] = g0
                if w is not None:                             # the needs that decide `pushed`: those of frames not pushed before
                    det["entry"].extend((margin - g0)[~pushed[c, p] & ~np.isnan(g0)].tolist())
                pushed[c, p] |= psh
                capped[c, p] |= cap
                plan.append((a, bb, w, envelope(m, blend), u))
            for a, bb, w, e, u in plan:                       # ascending pair order: for every dancer its pairs in that order
                if w is None:
                    continue
                S[c, a] = S[c, a] - ((w[0] * e)[:, None] * u)
                S[c, bb] = S[c, bb] + ((w[1] * e)[:, None] * u)
    # the output
    out_j, out_p = joints.copy(), pos.copy().reshape(b, T, dn, 3)
    y64 = []
    for c in range(b):
        for d in range(dn):
            move = (S[c, d, :, 0] != 0.0) | (S[c, d, :, 1] != 0.0)
            for n, k in enumerate(fl):
                with np.errstate(invalid="ignore"):
                    yj = J64[c, d, :, :, k] + S[c, d, :, n][:, None]
                    yp = out_p[c, :, d, k].astype(np.float64) + S[c, d, :, n]
                    out_j[c, d, move, :, k] = yj[move].astype(np.float32)
                    out_p[c, move, d, k] = yp[move].astype(np.float32)
                y64 += [yj[move].reshape(-1), yp[move]]
    out_p = out_p.reshape(b, T * dn, 3)
    O64 = out_j.astype(np.float64)
    for c in range(b):
        for p, (a, bb) in enumerate(pr):
            after[c, p] = gaps(O64[c, a], O64[c, bb], radii, parents)
    if rounds == 0:
        before = after.copy()

    def finite_min(g):
        f = g[np.isfinite(g)]
        return f.min() if f.size else np.nan

    with np.errstate(invalid="ignore"):
        out = {"pos": out_p, "joints": out_j, "contact_before": (before < 0.0).sum(-1).astype(np.int64),
               "contact_after": (after < 0.0).sum(-1).astype(np.int64),
               "gap_min_before": np.array([[finite_min(before[c, p]) for p in range(P)] for c in range(b)]).reshape(b, P),
               "gap_min_after": np.array([[finite_min(after[c, p]) for p in range(P)] for c in range(b)]).reshape(b, P),
               "pushed": pushed.sum(-1).astype(np.int64), "capped": capped.sum(-1).astype(np.int64),
               "max_shift": np.sqrt(S[..., 0] * S[..., 0] + S[..., 1] * S[..., 1]).max(-1), "shift": S}
    dS = S[:, :, 1:] - S[:, :, :-1]
    out["max_step"] = np.sqrt(dS[..., 0] * dS[..., 0] + dS[..., 1] * dS[..., 1]).max(-1) if T > 1 else np.zeros((b, dn))
    if details:
        det["y64"] = np.concatenate(y64) if y64 else np.zeros(0)
        out["details"] = det
        out["gap_before"], out["gap_after"], out["flags"] = before, after, pushed.astype(np.int64) + 2 * capped.astype(np.int64)
    return out


def judge(ref):
    """(ok, reasons) from a keep_apart(..., details=True) result; see decisions_clear"""
    det, why = ref["details"], []
    n2 = np.asarray(det["n2"], np.float64)
    if ((n2 != 0.0) & (n2 < 1e-12)).any():
        why.append(f"a squared root distance of {n2[n2 != 0.0].min():.3e}")
    need = np.asarray(det["entry"], np.float64)
    if need.size and np.abs(need).min() <= GUARD:
        why.append(f"a need of {np.abs(need).min():.3e} at a round's entry")
    cap = np.asarray(det["cap"], np.float64)
    if cap.size and np.abs(cap).min() <= GUARD:
        why.append(f"a push within {np.abs(cap).min():.3e} of max_push")
    for name in ("gap_before", "gap_after"):
        g = ref[name][~np.isnan(ref[name])]
        if not np.isfinite(g).all():
            why.append(f"an infinite {name}")
        if g.size and np.abs(g).min() <= GUARD:
            why.append(f"a {name} of {np.abs(g).min():.3e}")
    y = det["y64"][np.isfinite(det["y64"]) & (det["y64"] != 0.0)]          # an exact 0 is the sum of exact inputs
    if y.size and not (np.array_equal((y - ROUNDING_GUARD).astype(np.float32), (y + ROUNDING_GUARD).astype(np.float32))):
        why.append(f"a shifted coordinate within {ROUNDING_GUARD:g} of a float32 rounding boundary")
    return not why, why


def decisions_clear(pos, joints, **kw):
    """No discontinuous decision of the construction is a near-tie on these inputs, so an implementation that rounds differently in the
    last places still decides the same way: every squared root distance exactly 0 or at least 1e-12 (the 1e-18 fallback); every
    m + need more than 1e-9 from max_push (m == max_push); every gap finite or NaN; every need at a round's entry of a frame that no
    earlier round pushed, which decides `pushed`, more than 1e-9 from 0 (a frame pushed before stays pushed, and its m is continuous in
    the need); every before and after gap more than 1e-9 from 0 (the contact counts); every shifted coordinate
    that is not exactly 0 more than 1e-14 from a float32 rounding boundary (the after gaps are evaluated on the rounded output)."""
    return judge(keep_apart(pos, joints, details=True, **kw))


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 2, 1), (1, 2, 2), (1, 2, 7), (2, 3, 5), (1, 5, 70), (2, 3, 150), (1, 2, 1125)]
SPREAD = 0.8                                                # metres along x between neighbouring dancers
SEEDS = {}                                                  # shape -> seed of group_ref.synth, where 0 leaves a near-tie
_cache = {}


def pos_of(joints):
    """the root joints as export_poses lays pos out: (b, T dn, 3), row = frame dn + dancer"""
    b, dn, T = joints.shape[:3]
    return np.ascontiguousarray(np.moveaxis(joints[:, :, :, 0], 1, 2).reshape(b, T * dn, 3))


def spread(b, dn, T, seed=None, by=SPREAD):
    """group_ref.synth(b, dn, T) with dancer d moved by `by` d metres along x: dancers that meet now and then instead of walking through
    each other.  -> pos, joints (float32, read-only, cached); by = 0 gives the unspread input"""
    seed = SEEDS.get((b, dn, T), 0) if seed is None else seed
    key = (b, dn, T, seed, by)
    if key not in _cache:
        J = G.synth(b, dn, T, seed).astype(np.float64)
        J[..., 0] += by * np.arange(dn).reshape(1, dn, 1, 1)
        J = np.ascontiguousarray(J.astype(np.float32))
        p = pos_of(J)
        J.setflags(write=False)
        p.setflags(write=False)
        _cache[key] = (p, J)
    return _cache[key]


def permuted(pos, joints, up):
    """the same motion with the axis `up` up instead of z: the components (floor 0, floor 1, up) = (x, y, z) of the input"""
    order = {0: [2, 0, 1], 1: [0, 2, 1], 2: [0, 1, 2]}[up]
    return np.ascontiguousarray(pos[..., order]), np.ascontiguousarray(joints[..., order])


def parameter_cases():
    """(name, (pos, joints), keyword arguments) of the GPU test's runs with other parameters; tests/test_apart_cpu.py holds each to
    decisions_clear"""
    parents, radii = G.custom_skeleton()
    base, small = spread(1, 5, 70), spread(2, 3, 5, by=0.0)
    return [("up=1", permuted(*base, 1), dict(up=1)), ("rounds=0", base, dict(rounds=0)), ("rounds=1", base, dict(rounds=1)),
            ("iterations=1", base, dict(iterations=1)), ("blend=0", base, dict(blend=0)), ("blend>T", small, dict(blend=9)),
            ("mobility", base, dict(mobility=[1.0, 0.0, 2.0, 0.0, 0.5])), ("skeleton", base, dict(radii=radii, parents=parents)),
            ("unspread", small, dict())]
