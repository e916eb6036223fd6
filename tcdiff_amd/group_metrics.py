"""Is the GROUP any good?  Three questions about every pair of dancers of a clip, answered in closed form from the joint positions
``export_poses`` (or ``foot_lock``) leaves on the device, in three launches (``tcg_group_metrics``, csrc/group.hip), float64 throughout:

* ``body_contact_rate`` / ``body_gap_min`` / ``body_contact_episodes`` / ``body_closest``: do the bodies touch?  Each dancer is 23
  capsules (bone segments with a radius); the gap of two dancers is the smallest distance of two capsules, negative when they overlap.
* ``path_crossings`` / ``path_crossing_rate``: do the dancers walk through each other's paths?  Proper crossings of the root's floor
  steps that lie at most ``window`` frames apart.
* ``sync`` / ``sync_lag`` / ``sync_zero``: do they move together?  The mean over the joints of the lagged correlation of the
  standardised root-relative joint speeds, maximised over ``|lag| <= max_lag``; a positive lag means that the second dancer trails.

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)        # what evaluate_group does
    print(summarize(group_metrics(poses)))

include/tcdiff_group.h is the definition.  The metrics are the project's own, in the spirit of AIOZ-GDance's TIF and GMC; parity with
AIOZ-GDance's code is unpinned.  The radii, the window, the lag range and ``sigma_floor`` are choices, not measurements.  Not built:
GMR (it needs a trained feature extractor), drawing a contact.  Resolving one is ``keep_apart`` (tcdiff_amd/apart.py); the surfaces
themselves are measured by ``mesh_contact`` (tcdiff_amd/mesh_contact.py); contact between parts of one dancer is ``self_contact``
(tcdiff_amd/self_contact.py).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .export import export_poses
from .fk import SMPL_PARENTS

MAX_LAG = L.GROUP.constants["TC_GROUP_MAX_LAG"]

# metres, by bone (= the joint the bone ends at); a stated choice for an adult of SMPL's mean shape
_RADII = {0.10: (1, 2, 15), 0.075: (4, 5), 0.05: (7, 8), 0.04: (10, 11, 20, 21), 0.13: (3, 6, 9), 0.06: (12, 16, 17), 0.07: (13, 14),
          0.045: (18, 19), 0.035: (22, 23)}


def capsule_radii() -> np.ndarray:
    """The default capsule radius of every bone, (24,) float64 in metres; bone i runs from joint parents[i] to joint i, entry 0 is
    unused.  Hips 0.10, thighs 0.075, shins 0.05, feet 0.04, spine 0.13, neck 0.06, collars 0.07, head 0.10, shoulders 0.06, upper
    arms 0.045, forearms 0.04, hands 0.035: a choice, not a measurement (``radii_from_body`` measures a body model instead)."""
    r = np.zeros(24, np.float64)
    for value, bones in _RADII.items():
        r[list(bones)] = value
    return r


def pairs(dn) -> list:
    """the pairs (a, b), a < b, in the order of the outputs' second dimension: (0,1), (0,2), ..., (1,2), ...; dn (dn - 1) / 2 of them"""
    if isinstance(dn, bool) or not isinstance(dn, (int, np.integer)) or dn < 1:
        raise L.TcdiffError(f"pairs: dn must be an int >= 1, got {dn!r}")
    return [(a, b) for a in range(dn) for b in range(a + 1, dn)]


def _point_segment(v, p, q):
    d = q - p
    dd = float(d @ d)
    s = 0.0 if dd <= 1e-18 else min(1.0, max(0.0, float((v - p) @ d) / dd))
    return float(np.linalg.norm(v - (p + s * d)))


def radii_from_body(body) -> np.ndarray:
    """Capsule radii measured on the rest pose of a ``BodyModel`` (``load_body_model``), host numpy in float64, done once: each vertex
    goes to the bone nearest to it (point-to-segment distance, the smaller bone index on a tie) among the bones that start or end at
    the joint of its largest skinning weight (the first such joint on a tie); a bone's radius is the median distance of its vertices;
    a bone with no vertex keeps ``capsule_radii``'s value."""
    for name in ("v_shaped", "J", "weights", "parents"):
        if not hasattr(body, name):
            raise L.TcdiffError(f"radii_from_body: a BodyModel is needed (no {name!r}), got {type(body).__name__}")
    v, J, w = np.asarray(body.v_shaped, np.float64), np.asarray(body.J, np.float64), np.asarray(body.weights, np.float64)
    parents = list(body.parents)
    dist = [[] for _ in range(24)]
    for n in range(v.shape[0]):
        k = int(np.argmax(w[n]))
        best, best_d = -1, math.inf
        for i in range(1, 24):
            if parents[i] == k or i == k:
                d = _point_segment(v[n], J[parents[i]], J[i])
                if d < best_d:
                    best, best_d = i, d
        if best > 0:
            dist[best].append(best_d)
    r = capsule_radii()
    for i in range(1, 24):
        if dist[i]:
            r[i] = float(np.median(np.array(dist[i], np.float64)))
    return r


def _check_joints(joints):
    if not isinstance(joints, torch.Tensor) or joints.dim() != 5 or tuple(joints.shape[3:]) != (24, 3):
        raise L.TcdiffError(f"group_metrics: joints must be (b, dn, T, 24, 3), got "
                            f"{tuple(joints.shape) if isinstance(joints, torch.Tensor) else type(joints)}")
    if joints.dtype != torch.float32:
        raise L.TcdiffError(f"group_metrics: joints must be float32, got {joints.dtype}")
    if min(joints.shape[:3]) < 1:
        raise L.TcdiffError(f"group_metrics: joints {tuple(joints.shape)} has an empty dimension")
    if joints.stride(-1) != 1 or joints.stride(-2) != 3:
        raise L.TcdiffError(f"group_metrics: the trailing 2 dimension(s) of joints must be contiguous (strides {tuple(joints.stride())})")


def _int(v, what, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise L.TcdiffError(f"group_metrics: {what}, got {v!r}")
    return int(v)


def group_metrics(joints, *, fps=30, up=2, radii=None, parents=None, window=None, max_lag=15, sigma_floor=1e-6,
                  return_frames=False) -> dict:
    """joints (b, dn, T, 24, 3) float32 on the device, in metres, read in place through its strides (only the trailing 24 x 3 must
    be contiguous: the permuted view of a frame-major buffer is read without a copy).

    Returns device tensors per clip and pair (``pairs(dn)`` gives the order; P = dn (dn - 1) / 2): float64 (b, P)
    ``body_contact_rate``, ``body_gap_min`` (metres, negative = penetration depth), ``path_crossing_rate``, ``sync``, ``sync_zero``;
    int64 (b, P) ``body_contact_episodes``, ``path_crossings``, ``sync_lag`` and (b, P, 3) ``body_closest`` (frame, bone of a, bone of
    b of the smallest gap).  With ``return_frames`` also ``gap`` float64 and ``closest`` int32 (= 24 i + j), both (b, P, T).
    One dancer gives empty (b, 0) tensors and launches nothing.  Nothing is copied to the host; ``metrics.summarize`` does that.

    ``radii`` (24,) capsule radii by bone (default ``capsule_radii()``), ``parents`` the skeleton (default SMPL's), ``window`` the
    largest distance in frames of two steps that can cross (None: ``fps`` frames, one second), ``max_lag`` the lag range in frames
    (at most 64), ``sigma_floor`` the deviation of a joint's speed at or below which the joint is left out of ``sync``: choices, not
    measurements.  The definitions: include/tcdiff_group.h."""
    _check_joints(joints)
    b, dn, T = joints.shape[:3]
    if isinstance(up, bool) or up not in (0, 1, 2):
        raise L.TcdiffError(f"group_metrics: up must be 0, 1 or 2, got {up!r}")
    if isinstance(fps, bool) or not isinstance(fps, (int, float)) or not math.isfinite(fps) or not fps > 0:
        raise L.TcdiffError(f"group_metrics: fps must be a positive number, got {fps!r}")
    window = max(int(round(fps)), 0) if window is None else _int(window, "window must be an int >= 0", 0, 2 ** 31 - 1)
    max_lag = _int(max_lag, f"max_lag must be an int in [0, {MAX_LAG}]", 0, MAX_LAG)
    if isinstance(sigma_floor, bool) or not isinstance(sigma_floor, (int, float)) or not (0 <= sigma_floor < math.inf):
        raise L.TcdiffError(f"group_metrics: sigma_floor must be a finite number >= 0, got {sigma_floor!r}")
    radii = capsule_radii() if radii is None else np.asarray(radii, np.float64)
    if radii.shape != (24,) or not np.isfinite(radii[1:]).all() or (radii[1:] < 0).any():
        raise L.TcdiffError("group_metrics: radii must be 24 finite numbers >= 0 (entry 0 is unused)")
    parents = list(SMPL_PARENTS if parents is None else parents)
    if len(parents) != 24 or any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) for p in parents) or \
            any(not 0 <= parents[j] < j for j in range(1, 24)):
        raise L.TcdiffError("group_metrics: parents must be 24 ints, every parent before its child")
    if not joints.is_cuda:
        raise L.TcdiffError("group_metrics runs on MI355X only (no CPU fallback)")
    dev = joints.device
    joints = joints.detach()
    P = dn * (dn - 1) // 2
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)
    out = {"body_contact_rate": f64(b, P), "body_gap_min": f64(b, P), "body_contact_episodes": i64(b, P), "body_closest": i64(b, P, 3),
           "path_crossings": i64(b, P), "path_crossing_rate": f64(b, P), "sync": f64(b, P), "sync_lag": i64(b, P), "sync_zero": f64(b, P)}
    if return_frames:
        out.update(gap=f64(b, P, T), closest=torch.empty(b, P, T, dtype=torch.int32, device=dev))
    if P == 0:
        return out
    with torch.cuda.device(dev):
        workspace = torch.empty(K.group_workspace(b, dn, T, max_lag), dtype=torch.uint8, device=dev)
        K.group_metrics(joints, int(up), float(fps), [-1 if j == 0 else int(p) for j, p in enumerate(parents)], radii.tolist(), window,
                        max_lag, float(sigma_floor), workspace, out.get("gap"), out.get("closest"), out["body_contact_rate"],
                        out["body_gap_min"], out["body_contact_episodes"], out["body_closest"], out["path_crossings"],
                        out["path_crossing_rate"], out["sync"], out["sync_lag"], out["sync_zero"])
    return out


def evaluate_group(samples, normalizer, dn, mode="normal", **kw) -> dict:
    """The sampler's normalised samples (b, S * dn, 151) -> ``group_metrics`` of the exported poses: ``export_poses``, then
    ``group_metrics``, everything on the device.  In "long" mode the b windows are one song, so the result has one row."""
    _, _, poses, _ = export_poses(samples, normalizer, mode, dn)
    return group_metrics(poses, **kw)
