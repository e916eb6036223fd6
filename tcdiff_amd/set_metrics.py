"""Did the checkpoint get better?  The set-level numbers of the dance-generation papers (Bailando's FID_k and Div_k, as EDGE,
AIOZ-GDance and TCDiff report them): a set of generated dances against a set of real ones, on the device, float64 throughout
(csrc/set_metrics.hip, the definitions in include/tcdiff_hip.h).

    ref = reference_from_joints(real_joints)                     # once per dataset; ref.save("kinetic_ref.npz")
    print(summarize(evaluate_set(samples, normalizer, dn, ref)))

* ``kinetic_features``: 72 kinetic features per (clip, dancer) -- per joint the horizontal and vertical kinetic energy and the
  energy expenditure -- one launch;
* ``fit_reference``: column mean / std of a reference set, and the mean and covariance of its normalised rows, two launches;
* ``set_scores``: ``fid`` and ``div`` of a set normalised with the reference's mean / std, three launches; the Frechet distance's
  two symmetric eigen-decompositions are a Jacobi solver resident in LDS.

The set functions take any (N, D) float64 matrix with D <= 72, so a caller can bring other features.  One other set is built in:
``geometric_features`` (csrc/geometric.hip, the definitions in include/tcdiff_hip_ext.h), the 32 relational boolean features on
which Bailando and FACT report FID_g and Div_g, one launch of a table-driven evaluator; ``features="geometric"`` selects them in
``reference_from_joints`` / ``evaluate_set``, and ``evaluate_set_all`` scores both sets from one ``export_poses``.  The table is
restated from memory of the AIST++ API and Bailando's copy of it: parity with those packages is NOT pinned.  Two of their quirks
are kept on purpose, because published numbers carry them: the "move" rows 4, 5 and 9-11 test the velocity of the THIRD joint
name (the fourth is never read), and the time per frame is 1 / 120 whatever the clip's frame rate."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .export import export_poses

N_KINETIC = 72


def _check_view(fn, name, t, shape, inner, cuda=True):
    """the rules of metrics._check_view, under this module's function names; cuda=False leaves the device to the caller"""
    if not isinstance(t, torch.Tensor) or t.dim() != len(shape) or any(w is not None and s != w for s, w in zip(t.shape, shape)):
        want = ", ".join("*" if w is None else str(w) for w in shape)
        raise L.TcdiffError(f"{fn}: {name} must be ({want}), got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if t.dtype != torch.float32:
        raise L.TcdiffError(f"{fn}: {name} must be float32, got {t.dtype}")
    want = 1
    for k in range(1, inner + 1):                  # the trailing dimensions are read as one contiguous run
        if t.shape[-k] != 1 and t.stride(-k) != want:
            raise L.TcdiffError(f"{fn}: the trailing {inner} dimension(s) of {name} must be contiguous (strides {tuple(t.stride())})")
        want *= t.shape[-k]
    if cuda and not t.is_cuda:
        raise L.TcdiffError(f"{fn} runs on MI355X only (no CPU fallback)")


def kinetic_features(joints, *, fps=30, up=2, window=2) -> torch.Tensor:
    """joints (b, dn, T, 24, 3) float32 on the device, in metres, read in place through its strides (only the trailing 24 x 3 must
    be contiguous) -> (b, dn, 72) float64, column 3 j + k of joint j: k = 0 horizontal kinetic energy, 1 vertical kinetic energy,
    2 energy expenditure, from velocities / accelerations averaged over ``window`` frames to either side.  T < 3 gives NaN."""
    _check_view("kinetic_features", "joints", joints, (None, None, None, 24, 3), 2)
    b, dn, T = joints.shape[:3]
    if min(b, dn, T) < 1:
        raise L.TcdiffError(f"kinetic_features: joints {tuple(joints.shape)} has an empty dimension")
    if up not in (0, 1, 2):
        raise L.TcdiffError(f"kinetic_features: up must be 0, 1 or 2, got {up!r}")
    if int(window) != window or window < 1:
        raise L.TcdiffError(f"kinetic_features: window must be a whole number of frames >= 1, got {window!r}")
    fps = float(fps)
    if not fps > 0:
        raise L.TcdiffError("kinetic_features: fps must be positive")
    feats = torch.empty(b, dn, N_KINETIC, dtype=torch.float64, device=joints.device)
    with torch.cuda.device(joints.device):
        K.kinetic_features(joints, int(up), min(int(window), 1 << 30), fps, feats)
    return feats


# ---- geometric features ----------------------------------------------------------------------------------------------------------
GEO_KINDS = ("PLANE", "NPLANE", "MOVE", "NMOVE", "ANGLE", "FAST")               # L.GEO_PLANE .. L.GEO_FAST
GEO_POINTS = ("root", "lhip", "rhip", "belly", "lknee", "rknee", "spine", "lankle", "rankle", "chest", "ltoes", "rtoes", "neck",
              "linshoulder", "rinshoulder", "head", "lshoulder", "rshoulder", "lelbow", "relbow", "lwrist", "rwrist", "lhand",
              "rhand", "zero", "up", "-up", "floor")                             # the 24 joints and the four made-up points
# the points of the SMPL rest pose the AIST++ API hard-codes, and the three lengths the thresholds are multiples of
GEO_REST = {"lshoulder": (0.199113488, 0.236807942, -0.0180702247), "lelbow": (0.454445392, 0.221158922, -0.0410167128),
            "rshoulder": (-0.191692337, 0.236928746, -0.0123055102), "lhip": (0.0564076714, -0.323069185, 0.0109197125),
            "rhip": (-0.0624834076, -0.331302464, 0.0150412619)}
GEO_LENGTHS = {"hl": ("lshoulder", "lelbow"), "sw": ("lshoulder", "rshoulder"), "hw": ("lhip", "rhip")}
# (kind, a, b, c, p, factor, length) or, for angles, (kind, a, b, c, p, lo, hi) in degrees.  MOVE does not read c and FAST reads
# only p: c holds the package's ignored fourth name there, and a FAST row repeats p.
GEOMETRIC_TABLE = (
    ("NMOVE", "neck", "rhip", "lhip", "rwrist", 1.8, "hl"),
    ("NMOVE", "neck", "lhip", "rhip", "lwrist", 1.8, "hl"),
    ("NPLANE", "chest", "neck", "neck", "rwrist", 0.2, "hl"),
    ("NPLANE", "chest", "neck", "neck", "lwrist", 0.2, "hl"),
    ("MOVE", "belly", "chest", "rwrist", "chest", 1.8, "hl"),
    ("MOVE", "belly", "chest", "lwrist", "chest", 1.8, "hl"),
    ("ANGLE", "relbow", "rshoulder", "relbow", "rwrist", 0.0, 110.0),
    ("ANGLE", "lelbow", "lshoulder", "lelbow", "lwrist", 0.0, 110.0),
    ("NPLANE", "lshoulder", "rshoulder", "lwrist", "rwrist", 2.5, "sw"),
    ("MOVE", "lwrist", "rwrist", "lwrist", "rwrist", 1.4, "hl"),
    ("MOVE", "rwrist", "root", "root", "lwrist", 1.4, "hl"),
    ("MOVE", "lwrist", "root", "root", "rwrist", 1.4, "hl"),
    ("FAST", "rwrist", "rwrist", "rwrist", "rwrist", 2.5, "hl"),
    ("FAST", "lwrist", "lwrist", "lwrist", "lwrist", 2.5, "hl"),
    ("PLANE", "root", "lhip", "ltoes", "rankle", 0.38, "hl"),
    ("PLANE", "root", "rhip", "rtoes", "lankle", 0.38, "hl"),
    ("NPLANE", "zero", "up", "floor", "rankle", 1.2, "hl"),
    ("NPLANE", "zero", "up", "floor", "lankle", 1.2, "hl"),
    ("NPLANE", "lhip", "rhip", "lankle", "rankle", 2.1, "hw"),
    ("ANGLE", "rknee", "rhip", "rknee", "rankle", 0.0, 110.0),
    ("ANGLE", "lknee", "lhip", "lknee", "lankle", 0.0, 110.0),
    ("FAST", "rankle", "rankle", "rankle", "rankle", 2.5, "hl"),
    ("FAST", "lankle", "lankle", "lankle", "lankle", 2.5, "hl"),
    ("ANGLE", "neck", "root", "rshoulder", "relbow", 25.0, 180.0),
    ("ANGLE", "neck", "root", "lshoulder", "lelbow", 25.0, 180.0),
    ("ANGLE", "neck", "root", "rhip", "rknee", 50.0, 180.0),
    ("ANGLE", "neck", "root", "lhip", "lknee", 50.0, 180.0),
    ("PLANE", "rankle", "neck", "lankle", "root", 0.5, "hl"),
    ("ANGLE", "neck", "root", "zero", "up", 70.0, 110.0),
    ("NPLANE", "zero", "-up", "floor", "rwrist", -1.2, "hl"),
    ("NPLANE", "zero", "-up", "floor", "lwrist", -1.2, "hl"),
    ("FAST", "root", "root", "root", "root", 2.3, "hl"),
)
N_GEOMETRIC = len(GEOMETRIC_TABLE)
_geo_tables = {}          # device -> the default table's device copy (table, range)


def geometric_lengths() -> dict:
    """hl (upper arm), sw (shoulder width) and hw (hip width) of the rest pose, float64"""
    return {k: math.sqrt(sum((x - y) * (x - y) for x, y in zip(GEO_REST[p], GEO_REST[q]))) for k, (p, q) in GEO_LENGTHS.items()}


def geometric_table(lengths=None):
    """``GEOMETRIC_TABLE`` as the launcher reads it, on the host: table (R, 5) int32 of (kind, a, b, c, p) and range (R, 2) float64
    of (lo, hi); a threshold row has lo = factor * length and hi = lo (only ANGLE reads hi).  ``lengths``: a dict replacing some
    of ``geometric_lengths()``."""
    ln = geometric_lengths()
    for k, v in dict(lengths or {}).items():
        if k not in ln or not math.isfinite(float(v)):
            raise L.TcdiffError(f"geometric_table: lengths takes finite {', '.join(ln)}, got {k!r}: {v!r}")
        ln[k] = float(v)
    table = np.zeros((N_GEOMETRIC, 5), np.int32)
    rng = np.zeros((N_GEOMETRIC, 2), np.float64)
    for r, (kind, a, b, c, p, x, y) in enumerate(GEOMETRIC_TABLE):
        table[r] = [GEO_KINDS.index(kind)] + [GEO_POINTS.index(n) for n in (a, b, c, p)]
        rng[r] = (x, y) if kind == "ANGLE" else (x * ln[y], x * ln[y])
    return table, rng


def _check_table(table):
    """a caller's (table, range) -> int32 (R, 5) and float64 (R, 2) on the host, or TcdiffError"""
    fn = "geometric_features"
    try:
        t, r = table
        t, r = np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t), np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r)
    except (TypeError, ValueError):
        raise L.TcdiffError(f"{fn}: table must be a pair (table (R, 5) of integers, range (R, 2) of floats)") from None
    if t.ndim != 2 or t.shape[1] != 5 or r.shape != (t.shape[0], 2) or t.dtype.kind not in "iu" or r.dtype.kind not in "fiu":
        raise L.TcdiffError(f"{fn}: table must be a pair (table (R, 5) of integers, range (R, 2) of floats), got "
                            f"{t.dtype} {t.shape} and {r.dtype} {r.shape}")
    R = t.shape[0]
    if R < 1 or R > L.SET_MAX_D:
        raise L.TcdiffError(f"{fn}: 1 to {L.SET_MAX_D} table rows are supported, got {R}")
    if ((t[:, 0] < 0) | (t[:, 0] >= len(GEO_KINDS))).any():
        raise L.TcdiffError(f"{fn}: a kind of the table is outside 0..{len(GEO_KINDS) - 1}")
    if ((t[:, 1:] < 0) | (t[:, 1:] >= L.GEO_POINTS)).any():
        raise L.TcdiffError(f"{fn}: a point of the table is outside 0..{L.GEO_POINTS - 1}")
    r = r.astype(np.float64)
    if not np.isfinite(r).all():
        raise L.TcdiffError(f"{fn}: the table's ranges must be finite")
    return np.ascontiguousarray(t, np.int32), np.ascontiguousarray(r)


def geometric_features(joints, *, up=2, time_per_frame=1 / 120, lengths=None, table=None) -> torch.Tensor:
    """joints (b, dn, T, 24, 3) float32 on the device, in metres, read in place through its strides (only the trailing 24 x 3 must
    be contiguous) -> (b, dn, R) float64: per table row the fraction of the frames 1 .. T - 1 at which its predicate holds
    (include/tcdiff_hip_ext.h).  The default table is ``geometric_table(lengths)``, R = 32, uploaded once per device; ``table`` is
    a caller's own (table (R, 5), range (R, 2)), R <= 72, checked on the host.  ``time_per_frame`` defaults to the AIST++ API's
    hard-coded 1 / 120, whatever the clip's frame rate.  T < 2 gives NaN.  Parity with the AIST++ API / Bailando is not pinned."""
    fn = "geometric_features"
    _check_view(fn, "joints", joints, (None, None, None, 24, 3), 2, cuda=False)
    b, dn, T = joints.shape[:3]
    if min(b, dn, T) < 1:
        raise L.TcdiffError(f"{fn}: joints {tuple(joints.shape)} has an empty dimension")
    if up not in (0, 1, 2):
        raise L.TcdiffError(f"{fn}: up must be 0, 1 or 2, got {up!r}")
    tau = float(time_per_frame)
    if not (tau > 0 and math.isfinite(tau)):
        raise L.TcdiffError(f"{fn}: time_per_frame must be positive and finite, got {time_per_frame!r}")
    if table is not None and lengths is not None:
        raise L.TcdiffError(f"{fn}: lengths scale the default table; a caller's table carries its own thresholds")
    default = table is None and lengths is None           # the one table that is kept on the device
    host = None if default else (_check_table(table) if table is not None else geometric_table(lengths))
    if not joints.is_cuda:
        raise L.TcdiffError(f"{fn} runs on MI355X only (no CPU fallback)")
    dev = _geo_tables.get(str(joints.device)) if default else None
    if dev is None:
        dev = tuple(torch.from_numpy(a).to(joints.device) for a in (host or geometric_table()))
        if default:
            _geo_tables[str(joints.device)] = dev
    t_dev, r_dev = dev
    feats = torch.empty(b, dn, t_dev.shape[0], dtype=torch.float64, device=joints.device)
    with torch.cuda.device(joints.device):
        K.geometric_features(joints, int(up), t_dev, r_dev, tau, feats)
    return feats


def _check_feats(fn, feats, D=None):
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2:
        raise L.TcdiffError(f"{fn}: feats must be (N, D), got {tuple(feats.shape) if isinstance(feats, torch.Tensor) else type(feats)}")
    if feats.dtype != torch.float64:
        raise L.TcdiffError(f"{fn}: feats must be float64, got {feats.dtype}")
    n, d = feats.shape
    if n < 2:
        raise L.TcdiffError(f"{fn}: a set needs at least 2 rows, got {n}")
    if d < 1 or d > L.SET_MAX_D:
        raise L.TcdiffError(f"{fn}: 1 to {L.SET_MAX_D} feature columns are supported, got {d}")
    if D is not None and d != D:
        raise L.TcdiffError(f"{fn}: feats has {d} columns, the reference {D}")
    if not feats.is_cuda:
        raise L.TcdiffError(f"{fn} runs on MI355X only (no CPU fallback)")
    return feats.contiguous()


class SetStats:
    """What ``set_scores`` needs of a reference set, float64 device tensors: ``n`` rows; columnwise ``mean`` and population ``std``
    (D,); ``mu_z`` (D,) and ``cov_z`` (D, D), mean and covariance (divisor n - 1) of the rows normalised with them."""
    _FIELDS = ("mean", "std", "mu_z", "cov_z")

    def __init__(self, n, mean, std, mu_z, cov_z):
        self.n, self.mean, self.std, self.mu_z, self.cov_z = int(n), mean, std, mu_z, cov_z
        D = mean.numel()
        for k in self._FIELDS:
            t = getattr(self, k)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != ((D, D) if k == "cov_z" else (D,)):
                raise L.TcdiffError(f"SetStats: {k} must be a float64 tensor of {'(D, D)' if k == 'cov_z' else '(D,)'}, D = {D}")

    @property
    def dim(self) -> int:
        return self.mean.numel()

    def save(self, path) -> None:
        """an .npz of n and the four arrays (numpy only)"""
        with open(path, "wb") as f:
            np.savez(f, n=np.int64(self.n), **{k: getattr(self, k).detach().cpu().numpy() for k in self._FIELDS})

    @classmethod
    def load(cls, path, device) -> "SetStats":
        with np.load(path) as f:
            return cls(int(f["n"]), *(torch.from_numpy(np.ascontiguousarray(f[k], dtype=np.float64)).to(device) for k in cls._FIELDS))


def _stats(feats, fit, mean, std, want_div):
    """tcdiff_set_stats -> mu, cov, div_rows"""
    n, d = feats.shape
    dev = feats.device
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    z, zc, mu, cov = f64(d, n), f64(d, n), f64(d), f64(d, d)
    rows = f64(n) if want_div else None
    K.set_stats(feats, fit, mean, std, z, zc, mu, cov, rows)
    return mu, cov, rows


def fit_reference(feats) -> SetStats:
    """feats (N, D) float64 on the device, N >= 2 -> the ``SetStats`` of the set.  A constant column has std 0, normalises to zeros
    and leaves a zero row and column in ``cov_z``."""
    feats = _check_feats("fit_reference", feats)
    n, d = feats.shape
    mean = torch.empty(d, dtype=torch.float64, device=feats.device)
    std = torch.empty_like(mean)
    with torch.cuda.device(feats.device):
        mu, cov, _ = _stats(feats, True, mean, std, False)
    return SetStats(n, mean, std, mu, cov)


def set_scores(feats, ref: SetStats, *, check=False, _max_sweeps=L.SET_MAX_SWEEPS) -> dict:
    """feats (M, D) float64 on the device, M >= 2, against ``ref`` -> float64 device scalars

    * ``fid``: the Frechet distance between the Gaussians of the two sets' rows, both normalised with ``ref.mean`` / ``ref.std``:
      |mu - ref.mu_z|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), the last term from the eigenvalues of sqrt(S1) S2 sqrt(S1) with
      eigenvalues at rounding level clamped to zero, so sets of fewer rows than columns are well defined;
    * ``div``: the mean distance between two normalised rows of ``feats``.

    Nothing comes to the host.  Should the eigen-solver hit its cap of 30 sweeps, ``fid`` is NaN; ``check=True`` waits for the
    result and raises ``TcdiffError`` instead."""
    if not isinstance(ref, SetStats):
        raise L.TcdiffError(f"set_scores: ref must be a SetStats, got {type(ref)}")
    feats = _check_feats("set_scores", feats, ref.dim)
    dev = feats.device
    for k in SetStats._FIELDS:
        if getattr(ref, k).device != dev:
            raise L.TcdiffError("set_scores: feats and the reference must be on one device")
    fid = torch.empty((), dtype=torch.float64, device=dev)
    div = torch.empty_like(fid)
    status = torch.empty(3, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        mu, cov, rows = _stats(feats, False, ref.mean.contiguous(), ref.std.contiguous(), True)
        K.set_scores(ref.mu_z.contiguous(), ref.cov_z.contiguous(), mu, cov, rows, int(_max_sweeps), fid, div, status)
        if check:
            K.set_check(status)
    return {"fid": fid, "div": div}


_FEATURES = {"kinetic": kinetic_features, "geometric": geometric_features}


def _rows(poses, kw, features="kinetic"):
    if features not in _FEATURES:
        raise L.TcdiffError(f"features must be one of {', '.join(_FEATURES)}, got {features!r}")
    f = _FEATURES[features](poses, **kw)
    return f.view(f.shape[0] * f.shape[1], f.shape[2])


def evaluate_set(samples, normalizer, dn, ref: SetStats, mode="normal", *, check=False, features="kinetic", **kw) -> dict:
    """The sampler's normalised samples (b, S * dn, 151) -> ``set_scores`` of their kinetic features against ``ref``:
    ``export_poses``, ``kinetic_features`` (``**kw``: fps, up, window), one row per (clip, dancer), ``set_scores``; everything on
    the device.  In "long" mode the b windows are one song, so the set has dn rows.  ``features="geometric"``: the same with
    ``geometric_features`` (``**kw``: up, time_per_frame, lengths, table), ``fid`` and ``div`` then being FID_g and Div_g."""
    if features not in _FEATURES:
        raise L.TcdiffError(f"features must be one of {', '.join(_FEATURES)}, got {features!r}")
    _, _, poses, _ = export_poses(samples, normalizer, mode, dn)
    return set_scores(_rows(poses, kw, features), ref, check=check)


def evaluate_set_all(samples, normalizer, dn, refs: dict, mode="normal", *, check=False, kinetic=None, geometric=None) -> dict:
    """Both halves of the papers' table from ONE ``export_poses``: ``refs`` maps "kinetic" and / or "geometric" to the ``SetStats``
    of that feature set -> ``fid_k``, ``div_k``, ``fid_g``, ``div_g`` (float64 device scalars); a missing key leaves its two
    numbers out.  ``kinetic`` / ``geometric``: keyword arguments of the two feature functions, as dicts."""
    if not isinstance(refs, dict) or not refs or any(k not in _FEATURES for k in refs):
        raise L.TcdiffError(f"evaluate_set_all: refs maps {' and / or '.join(_FEATURES)} to a SetStats, got {refs!r}")
    _, _, poses, _ = export_poses(samples, normalizer, mode, dn)
    out = {}
    for features, kw in (("kinetic", kinetic), ("geometric", geometric)):
        if features in refs:
            res = set_scores(_rows(poses, kw or {}, features), refs[features], check=check)
            out["fid_" + features[0]], out["div_" + features[0]] = res["fid"], res["div"]
    return out


def reference_from_joints(joints, features="kinetic", **kw) -> SetStats:
    """ground-truth joints (b, dn, T, 24, 3) float32 on the device -> the ``SetStats`` of their b * dn feature rows: the kinetic
    features, or with ``features="geometric"`` the geometric ones (``**kw`` goes to the feature function)"""
    return fit_reference(_rows(joints, kw, features))
