"""numpy float64 restatement of the set-level metrics of tcdiff_amd/set_metrics.py (csrc/set_metrics.hip), written as straight
loops from the definitions in include/tcdiff_hip.h, and the seeded inputs the CPU and GPU tests share.  The Frechet distance's
eigenvalues come from numpy.linalg.eigh / eigvalsh (LAPACK's tridiagonal QR), an algorithm independent of the kernel's Jacobi."""
import numpy as np

FEATURE_SHAPES = [(1, 1, 1), (1, 1, 2), (1, 1, 3), (2, 3, 4), (1, 2, 5), (1, 2, 6), (2, 3, 150), (1, 1, 600)]     # (b, dn, T)
STATS_SHAPES = [(2, 1), (3, 5), (257, 72), (40, 12)]                                                               # (N, D)
SCORE_SHAPES = [(72, 200, 150), (72, 40, 30), (12, 40, 9), (72, 3, 2), (5, 2, 2), (1, 4, 3)]                       # (D, N_ref, M)
CLAMP_MARGIN = 3.0


# ---- kinetic features ------------------------------------------------------------------------------------------------------
def kinetic_one(J, fps=30, up=2, window=2):
    """one dancer's (T, 24, 3) float32 joints -> (72,)"""
    J = np.asarray(J, np.float64)
    T = J.shape[0]
    out = np.full(72, np.nan)
    if T < 3:
        return out
    dt = 1.0 / fps
    w = int(window)
    flat = [k for k in range(3) if k != up]
    for j in range(24):
        d = np.zeros((T, 3))
        d[1:] = J[1:, j] - J[:-1, j]                                 # d[s] = J[s] - J[s - 1]; d[0] is never read
        keh = kev = ee = 0.0
        for i in range(1, T):
            sv, nv, sa, na = np.zeros(3), 0, np.zeros(3), 0
            for s in range(i - w, i + w + 1):
                if s - 1 >= 0 and s <= T - 1:
                    sv = sv + d[s]
                    nv += 1
                if s - 1 >= 0 and s + 1 <= T - 1:
                    sa = sa + (d[s + 1] - d[s]) / (dt * dt)
                    na += 1
            v = sv / (nv * dt)
            a = sa / na
            keh += v[flat[0]] * v[flat[0]] + v[flat[1]] * v[flat[1]]
            kev += v[up] * v[up]
            ee += np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        out[3 * j:3 * j + 3] = keh / (T - 1), kev / (T - 1), ee / (T - 1)
    return out


def kinetic_features(joints, **kw):
    b, dn = joints.shape[:2]
    return np.stack([np.stack([kinetic_one(joints[c, d], **kw) for d in range(dn)]) for c in range(b)])


# ---- statistics --------------------------------------------------------------------------------------------------------------
def normalise(X, mean, std):
    return (np.asarray(X, np.float64) - mean[None, :]) / (std[None, :] + 1e-10)


def moments(Z):
    """mean and covariance (divisor n - 1, two-pass) of the rows of Z"""
    n, D = Z.shape
    mu = np.array([Z[:, c].sum() / n for c in range(D)])
    C = Z - mu[None, :]
    cov = np.zeros((D, D))
    for i in range(D):
        for j in range(i, D):
            cov[i, j] = cov[j, i] = (C[:, i] * C[:, j]).sum() / (n - 1)
    return mu, cov


def fit_reference(X):
    X = np.asarray(X, np.float64)
    n, D = X.shape
    mean = np.array([X[:, c].sum() / n for c in range(D)])
    std = np.array([np.sqrt(((X[:, c] - mean[c]) ** 2).sum() / n) for c in range(D)])
    mu, cov = moments(normalise(X, mean, std))
    return dict(n=n, mean=mean, std=std, mu_z=mu, cov_z=cov)


# ---- scores --------------------------------------------------------------------------------------------------------------------
def clamp_threshold(eig):
    return len(eig) * 2.0 ** -52 * max(float(np.max(eig)), 0.0)


def clamped_roots(eig):
    thr = clamp_threshold(eig)
    return np.array([np.sqrt(x) if x > thr else 0.0 for x in eig])


def frechet_parts(mu1, S1, mu2, S2):
    """-> fid, its scale |mu2 - mu1|^2 + tr S1 + tr S2, and the eigenvalues of both decompositions"""
    w, V = np.linalg.eigh(S1)
    R = (V * clamped_roots(w)[None, :]) @ V.T
    Mm = R @ S2 @ R
    lam = np.linalg.eigvalsh((Mm + Mm.T) * 0.5)
    dm = float(((mu2 - mu1) ** 2).sum())
    scale = dm + float(np.trace(S1)) + float(np.trace(S2))
    return scale - 2.0 * float(clamped_roots(lam).sum()), scale, (w, lam)


def clamp_clear(eigs, margin=CLAMP_MARGIN):
    """no eigenvalue of either decomposition within a factor `margin` of its threshold; also returns the closest factor"""
    closest = np.inf
    for eig in eigs:
        thr = clamp_threshold(eig)
        if thr == 0.0:
            continue                                                 # nothing is positive: every root is clamped, no decision
        for x in eig:
            f = x / thr if x > thr else (np.inf if x <= 0.0 else thr / x)
            closest = min(closest, f)
    return bool(closest > margin), float(closest)


def diversity(Z):
    m = Z.shape[0]
    s = 0.0
    for i in range(m):
        for j in range(i + 1, m):
            e = Z[i] - Z[j]
            s += np.sqrt((e * e).sum())
    return s / (m * (m - 1) / 2)


def set_scores(X, ref):
    """-> dict(fid, div, scale, eigs, mu, cov, z)"""
    Z = normalise(X, ref["mean"], ref["std"])
    mu, cov = moments(Z)
    fid, scale, eigs = frechet_parts(ref["mu_z"], ref["cov_z"], mu, cov)
    return dict(fid=fid, div=diversity(Z), scale=scale, eigs=eigs, mu=mu, cov=cov, z=Z)


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------
def synth_joints(b, dn, T, seed=0):
    """a body per dancer on a smooth random walk with limbs that swing: (b, dn, T, 24, 3) float32, metres"""
    g = np.random.default_rng(1000 + seed + 7 * T + 31 * dn + 101 * b)
    pose = g.uniform(-0.5, 0.5, (b, dn, 1, 24, 3))
    pose[..., 2] += 0.9
    root = np.cumsum(g.normal(0.0, 0.02, (b, dn, T, 1, 3)), axis=2)
    t = np.arange(T)[None, None, :, None, None]
    swing = g.uniform(0.0, 0.15, (b, dn, 1, 24, 3)) * np.sin(t * g.uniform(0.1, 0.6, (b, dn, 1, 24, 3)) + g.uniform(0, 6.28, (b, dn, 1, 24, 3)))
    return (pose + root + swing).astype(np.float32)


def synth_feats(n, D, seed, shift=0.0, constant=None):
    """(n, D) float64: columns of different scale and offset; `constant`: that column is 3.25 in every row"""
    g = np.random.default_rng(seed)
    scale, off = g.uniform(0.5, 20.0, D), g.uniform(-5.0, 5.0, D)      # (drawn first: the same columns for every n of a seed)
    X = (g.normal(0.0, 1.0, (n, D)) * (1.0 + shift) + shift) * scale[None, :] + off[None, :]
    if constant is not None:
        X[:, constant] = 3.25
    return X


SCORE_SEED = {s: 11 for s in SCORE_SHAPES}


def score_case(shape):
    """(D, N_ref, M) -> the reference set and the scored set, drawn from distributions a little apart"""
    D, n_ref, m = shape
    seed = SCORE_SEED[shape]
    ref = synth_feats(n_ref, D, seed)
    g = np.random.default_rng(seed + 1)
    gen = synth_feats(m, D, seed, shift=0.25) + g.normal(0.0, 0.1, (m, D))
    return ref, gen


def stats_case(shape):
    n, D = shape
    return synth_feats(n, D, 5 + n, constant=D // 2 if D > 1 else None)
