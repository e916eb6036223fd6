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

The set functions take any (N, D) float64 matrix with D <= 72, so a caller can bring other features."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .export import export_poses

N_KINETIC = 72


def _check_view(fn, name, t, shape, inner):
    """the rules of metrics._check_view, under this module's function names"""
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
    if not t.is_cuda:
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


def _rows(poses, kw):
    f = kinetic_features(poses, **kw)
    return f.view(f.shape[0] * f.shape[1], N_KINETIC)


def evaluate_set(samples, normalizer, dn, ref: SetStats, mode="normal", *, check=False, **kw) -> dict:
    """The sampler's normalised samples (b, S * dn, 151) -> ``set_scores`` of their kinetic features against ``ref``:
    ``export_poses``, ``kinetic_features`` (``**kw``: fps, up, window), one row per (clip, dancer), ``set_scores``; everything on
    the device.  In "long" mode the b windows are one song, so the set has dn rows."""
    _, _, poses, _ = export_poses(samples, normalizer, mode, dn)
    return set_scores(_rows(poses, kw), ref, check=check)


def reference_from_joints(joints, **kw) -> SetStats:
    """ground-truth joints (b, dn, T, 24, 3) float32 on the device -> the ``SetStats`` of their b * dn kinetic-feature rows"""
    return fit_reference(_rows(joints, kw))
