"""Does a dancer pass through ITSELF?  A forearm through the chest, a hand through the head, a shin through the other thigh: contact
between two capsules of ONE dancer, per clip and dancer, from the joint positions ``export_poses`` (or ``foot_lock``, ``keep_apart``,
``ground``) leaves on the device, in two launches (``tci_self_contact``, csrc/selfcontact.hip), float64 throughout:

* ``self_contact_rate`` / ``self_contact_episodes``: the share of frames in which two listed bones overlap by more than ``tolerance``,
  and the runs of such frames.
* ``self_gap_min`` / ``self_closest``: the smallest gap of two listed capsules (negative: the penetration depth) and the frame and
  the two bones that attain it.  ``self_depth_mean``: the mean depth over the contact frames.
* ``self_pair_frames``: per bone pair (``pair_index()`` gives the order) the number of frames in which that pair is in contact --
  the answer to "which limbs?".

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)        # what evaluate_self_contact does
    print(summarize(self_contact(poses)))

include/tcdiff_selfcontact.h is the definition.  The capsules are those of ``group_metrics``.  Neighbouring capsules of a body
overlap by construction, so only LISTED bone pairs are measured; ``self_pairs`` builds the default list: a pair is left out if the two
bones are at most ``hops`` apart in the skeleton or closer than ``rest_margin`` in the rest pose.  ``hops``, ``rest_margin``,
``tolerance`` and the radii are choices, not measurements: with the default radii the two thighs overlap by 3 cm in SMPL's rest pose
and the head and shoulder bones by 3-4 cm, and with a tolerance of 0 a dancer standing naturally would be "in contact" most of the time.
The reference has no counterpart; the metric is the project's own and parity with any other tool is unpinned.  Not built: resolving a
self-contact (bending an arm to dodge), mesh-level self-contact (a sub-mesh of one body is not closed, so the winding number of
``mesh_contact`` does not apply), drawing it, any use inside the sampler.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .export import export_poses
from .fk import SMPL_OFFSETS, SMPL_PARENTS
from .group_metrics import capsule_radii

PAIRS = L.SELF.constants["TC_SELF_PAIRS"]
_INDEX = [(i, j) for i in range(1, 24) for j in range(i + 1, 24)]
_SMALL = 1e-18


def pair_index() -> list:
    """the 253 bone pairs (i, j), 1 <= i < j <= 23, in the order of ``self_pair_frames``' last dimension: (1,2), (1,3), ..., (22,23)"""
    return list(_INDEX)


def pair_of(k) -> tuple:
    """pair k of ``pair_index()``"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < PAIRS:
        raise L.TcdiffError(f"pair_of: k must be an int in [0, {PAIRS}), got {k!r}")
    return _INDEX[int(k)]


def pair_mask(pairs) -> np.ndarray:
    """bone pairs [(i, j), ...] (either order of the two bones) -> the (253,) bool mask that lists them"""
    m = np.zeros(PAIRS, bool)
    try:
        pairs = [(int(i), int(j)) for i, j in pairs]
    except (TypeError, ValueError):
        raise L.TcdiffError(f"pair_mask: pairs must be (i, j) tuples of bones, got {pairs!r}") from None
    for i, j in pairs:
        i, j = min(i, j), max(i, j)
        if not 1 <= i < j <= 23:
            raise L.TcdiffError(f"pair_mask: a pair is two different bones in 1 .. 23, got {(i, j)!r}")
        m[_INDEX.index((i, j))] = True
    return m


def _clamp(x):
    return 0.0 if x < 0.0 else (1.0 if x > 1.0 else x)


def _seg_dist(p1, q1, p2, q2):
    """the distance of two segments by the clamped closest-point construction of include/tcdiff_group.h, float64 on the host"""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    A, E, F = dot(d1, d1), dot(d2, d2), dot(d2, r)
    if A <= _SMALL and E <= _SMALL:
        s = u = 0.0
    elif A <= _SMALL:
        s, u = 0.0, _clamp(F / E)
    else:
        Cc = dot(d1, r)
        if E <= _SMALL:
            u, s = 0.0, _clamp(-Cc / A)
        else:
            B = dot(d1, d2)
            den = A * E - B * B
            s = _clamp((B * F - Cc * E) / den) if den > 0.0 else 0.0
            u = (B * s + F) / E
            if u < 0.0:
                u, s = 0.0, _clamp(-Cc / A)
            elif u > 1.0:
                u, s = 1.0, _clamp((B - Cc) / A)
    diff = (p1 + s * d1) - (p2 + u * d2)
    return math.sqrt(dot(diff, diff))


def rest_pose(parents=None) -> np.ndarray:
    """SMPL's rest joints (24, 3) float64: the offsets of tcdiff_amd/fk.py summed down the tree"""
    parents = list(SMPL_PARENTS if parents is None else parents)
    off = np.asarray(SMPL_OFFSETS, np.float64)
    J = np.zeros((24, 3), np.float64)
    for j in range(1, 24):
        J[j] = J[parents[j]] + off[j]
    return J


def _radii(radii, who):
    radii = capsule_radii() if radii is None else np.asarray(radii, np.float64)
    if radii.shape != (24,) or not np.isfinite(radii[1:]).all() or (radii[1:] < 0).any():
        raise L.TcdiffError(f"{who}: radii must be 24 finite numbers >= 0 (entry 0 is unused)")
    return radii


def _parents(parents, who):
    parents = list(SMPL_PARENTS if parents is None else parents)
    if len(parents) != 24 or any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) for p in parents) or \
            any(not 0 <= parents[j] < j for j in range(1, 24)):
        raise L.TcdiffError(f"{who}: parents must be 24 ints, every parent before its child")
    return [int(p) for p in parents]


def self_pairs(*, radii=None, parents=None, rest_joints=None, hops=2, rest_margin=0.05) -> np.ndarray:
    """The default list of bone pairs, (253,) bool in ``pair_index()``'s order, built on the host in float64, once.

    Two bones are neighbours if they share a joint (one's parent joint is the other's, or one ends where the other starts).  A pair
    is left out if its distance in that neighbour graph is at most ``hops``, or if its gap in the rest pose,
    (dist - radii[i]) - radii[j] by the header's formula, is below ``rest_margin`` (metres).  ``rest_joints`` (24, 3) is the rest
    pose (default: SMPL's offsets summed down the tree; a user with a body passes ``body.J``, and ``radii_from_body(body)`` for the
    radii).  ``hops``, ``rest_margin`` and the radii are choices, not measurements."""
    radii, parents = _radii(radii, "self_pairs"), _parents(parents, "self_pairs")
    if isinstance(hops, bool) or not isinstance(hops, (int, np.integer)) or hops < 0:
        raise L.TcdiffError(f"self_pairs: hops must be an int >= 0, got {hops!r}")
    if isinstance(rest_margin, bool) or not isinstance(rest_margin, (int, float)) or not math.isfinite(rest_margin):
        raise L.TcdiffError(f"self_pairs: rest_margin must be a finite number, got {rest_margin!r}")
    if rest_joints is None:
        rest = rest_pose(parents)
    else:
        rest = np.asarray(rest_joints.detach().cpu() if isinstance(rest_joints, torch.Tensor) else rest_joints, np.float64)
        if rest.shape != (24, 3) or not np.isfinite(rest).all():
            raise L.TcdiffError("self_pairs: rest_joints must be (24, 3) finite numbers")
    ends = [None] + [{parents[i], i} for i in range(1, 24)]
    far = 24
    hop = np.full((24, 24), far, np.int64)
    for i in range(1, 24):                                   # breadth first from every bone
        hop[i, i] = 0
        front = [i]
        while front:
            nxt = []
            for a in front:
                for c in range(1, 24):
                    if hop[i, c] == far and ends[a] & ends[c]:
                        hop[i, c] = hop[i, a] + 1
                        nxt.append(c)
            front = nxt
    m = np.zeros(PAIRS, bool)
    for k, (i, j) in enumerate(_INDEX):
        if hop[i, j] <= hops:
            continue
        gap = (_seg_dist(rest[parents[i]], rest[i], rest[parents[j]], rest[j]) - radii[i]) - radii[j]
        m[k] = not gap < rest_margin
    return m


def _check_joints(joints):
    if not isinstance(joints, torch.Tensor) or joints.dim() != 5 or tuple(joints.shape[3:]) != (24, 3):
        raise L.TcdiffError(f"self_contact: joints must be (b, dn, T, 24, 3), got "
                            f"{tuple(joints.shape) if isinstance(joints, torch.Tensor) else type(joints)}")
    if joints.dtype != torch.float32:
        raise L.TcdiffError(f"self_contact: joints must be float32, got {joints.dtype}")
    if min(joints.shape[:3]) < 1:
        raise L.TcdiffError(f"self_contact: joints {tuple(joints.shape)} has an empty dimension")
    if joints.stride(-1) != 1 or joints.stride(-2) != 3:
        raise L.TcdiffError(f"self_contact: the trailing 2 dimension(s) of joints must be contiguous (strides {tuple(joints.stride())})")


def self_contact(joints, *, radii=None, parents=None, mask=None, rest_joints=None, hops=2, rest_margin=0.05, tolerance=0.03,
                 return_frames=False) -> dict:
    """joints (b, dn, T, 24, 3) float32 on the device, in metres, read in place through its strides (only the trailing 24 x 3 must
    be contiguous: the permuted view of a frame-major buffer is read without a copy); one dancer is enough.

    Returns device tensors per clip and dancer: float64 (b, dn) ``self_contact_rate``, ``self_gap_min`` (metres, negative = the
    penetration depth), ``self_depth_mean``; int64 (b, dn) ``self_contact_episodes``, (b, dn, 3) ``self_closest`` (frame and the two
    bones of the smallest gap) and (b, dn, 253) ``self_pair_frames`` (``pair_index()`` gives the order).  With ``return_frames`` also
    ``gap`` float64 and ``closest`` int32 (= 24 i + j), both (b, dn, T).  Nothing is copied to the host; ``metrics.summarize`` does that.

    ``mask`` (253,) bool lists the bone pairs that are measured (``pair_mask`` makes one from pairs); None: ``self_pairs(radii=...,
    parents=..., rest_joints=..., hops=..., rest_margin=...)``, which are otherwise unused.  ``radii`` (24,) capsule radii by bone
    (default ``capsule_radii()``), ``parents`` the skeleton (default SMPL's), ``tolerance`` the depth in metres a contact must exceed:
    choices, not measurements.  The definitions: include/tcdiff_selfcontact.h."""
    _check_joints(joints)
    b, dn, T = joints.shape[:3]
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or not (0 <= tolerance < math.inf):
        raise L.TcdiffError(f"self_contact: tolerance must be a finite number >= 0, got {tolerance!r}")
    radii, parents = _radii(radii, "self_contact"), _parents(parents, "self_contact")
    if mask is None:
        try:
            mask = self_pairs(radii=radii, parents=parents, rest_joints=rest_joints, hops=hops, rest_margin=rest_margin)
        except L.TcdiffError as e:
            raise L.TcdiffError(f"self_contact: {e}") from None
    else:
        mask = np.asarray(mask.detach().cpu() if isinstance(mask, torch.Tensor) else mask)
        if mask.shape != (PAIRS,) or mask.dtype != np.bool_:
            raise L.TcdiffError(f"self_contact: mask must be ({PAIRS},) bool (pair_mask makes one), got {mask.dtype} {mask.shape}")
    if not mask.any():
        raise L.TcdiffError("self_contact: no bone pair is listed (an empty mask)")
    if not joints.is_cuda:
        raise L.TcdiffError("self_contact runs on MI355X only (no CPU fallback)")
    words = [0, 0, 0, 0]
    for k in np.flatnonzero(mask):
        words[int(k) >> 6] |= 1 << (int(k) & 63)
    dev = joints.device
    joints = joints.detach()
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)
    out = {"self_contact_rate": f64(b, dn), "self_gap_min": f64(b, dn), "self_contact_episodes": i64(b, dn), "self_closest": i64(b, dn, 3),
           "self_depth_mean": f64(b, dn), "self_pair_frames": i64(b, dn, PAIRS)}
    if return_frames:
        out.update(gap=f64(b, dn, T), closest=torch.empty(b, dn, T, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        workspace = torch.empty(K.self_contact_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        K.self_contact(joints, [-1 if j == 0 else p for j, p in enumerate(parents)], radii.tolist(), words, float(tolerance), workspace,
                       out.get("gap"), out.get("closest"), out["self_contact_rate"], out["self_gap_min"], out["self_contact_episodes"],
                       out["self_closest"], out["self_depth_mean"], out["self_pair_frames"])
    return out


def evaluate_self_contact(samples, normalizer, dn, mode="normal", **kw) -> dict:
    """The sampler's normalised samples (b, S * dn, 151) -> ``self_contact`` of the exported poses: ``export_poses``, then
    ``self_contact``, everything on the device.  In "long" mode the b windows are one song, so the result has one row."""
    _, _, poses, _ = export_poses(samples, normalizer, mode, dn)
    return self_contact(poses, **kw)
