"""The foot lock: a post-process on what ``export_poses`` returns, on the device.  While the model declares a foot planted (its four
contact channels), the foot is held at the mean of where it stood, hip and knee are re-solved by analytic two-bone inverse
kinematics, the foot keeps its world orientation, and the correction is eased in and out around the contact.
include/tcdiff_footlock.h is the definition; ``tck_foot_lock`` (csrc/footlock.hip) runs it in three launches for any number of clips.

The reference has no counterpart: it renders the raw poses, planted feet sliding.  The construction is the textbook one, restated;
parity with any other tool is unpinned.  Not built: smoothing the shift where two runs touch, floor penetration and the height of the
anchor, toe-joint articulation, hands, correcting the root, locking inside the sampler.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import _lib as L
from . import kernels as K
from .fk import SMPL_OFFSETS, SMPL_PARENTS


class FootLock(NamedTuple):
    q: torch.Tensor                  # (b, T dn, 24, 3) float32: the poses, joints 1, 4, 7 and 2, 5, 8 re-solved where a shift applies
    joints: torch.Tensor | None      # (b, dn, T, 24, 3) float32: fk_forward of q, in place of export_poses' third result
    planted: torch.Tensor            # (b, dn, 2) int32: frames pinned, per leg (left, right)
    clamped: torch.Tensor            # (b, dn, 2) int32: frames whose target was out of reach
    max_shift: torch.Tensor          # (b, dn, 2) float64: the largest shift, in metres


def _number(v, what, ok):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not ok(v):
        raise L.TcdiffError(f"foot_lock: {what}, got {v!r}")
    return float(v)


def foot_lock(q, pos, contacts=None, *, dn, contact_threshold=0.95, still=0.01, blend=5, reach=1e-3, parents=None, offsets=None,
              return_joints=True) -> FootLock:
    """``q`` (b, T dn, 24, 3) float32 axis-angle and ``pos`` (b, T dn, 3) on the device, row = frame dn + dancer: ``export_poses``'
    first two results, in long mode too (b = 1).  ``contacts`` (b, dn, T, 4) float32 in the order of joints 7, 8, 10, 11, read in place
    through its strides (``export_poses``' permuted copy and a frame-major buffer alike); None, which is what long mode gives, labels
    the planted frames from the motion by the dataset's rule: a joint that moves less than ``still`` metres to the next frame.

    A foot is pinned by its ankle where the ankle's channel exceeds ``contact_threshold``, else by its toe where the toe's does; over
    each run of such frames the pin joint is moved to its mean position; outside the runs the shift fades over ``blend`` frames (two
    runs at most ``2 blend`` frames apart are bridged linearly).  A target further than ``(1 - reach)`` of the leg's length is clamped
    to that distance (and no nearer than ``reach`` of it).  ``blend = 5`` and ``reach = 1e-3`` are choices, not measurements:
    a sixth of a second at 30 frames a second, and a knee that never locks out completely.

    ``pos`` is never changed, nothing synchronises, nothing is copied to the host; ``parents`` / ``offsets`` default to the SMPL
    skeleton and must have SMPL's legs.  With ``return_joints=False`` the FK is skipped and ``joints`` is None."""
    if not isinstance(q, torch.Tensor) or not isinstance(pos, torch.Tensor):
        raise L.TcdiffError("foot_lock: q and pos must be tensors")
    if q.dim() != 4 or tuple(q.shape[2:]) != (24, 3) or q.dtype != torch.float32:
        raise L.TcdiffError(f"foot_lock: q must be (b, frames * dancers, 24, 3) float32, got {tuple(q.shape)} {q.dtype}")
    b, n = q.shape[:2]
    if tuple(pos.shape) != (b, n, 3) or pos.dtype != torch.float32:
        raise L.TcdiffError(f"foot_lock: pos must be ({b}, {n}, 3) float32, got {tuple(pos.shape)} {pos.dtype}")
    if isinstance(dn, bool) or not isinstance(dn, int) or dn < 1 or b < 1 or n < 1 or n % dn:
        raise L.TcdiffError(f"foot_lock: {n} rows are not a whole number of frames of {dn!r} dancers")
    T = n // dn
    if contacts is not None and (not isinstance(contacts, torch.Tensor) or tuple(contacts.shape) != (b, dn, T, 4) or contacts.dtype != torch.float32):
        raise L.TcdiffError(f"foot_lock: contacts must be ({b}, {dn}, {T}, 4) float32 or None")
    thr = _number(contact_threshold, "contact_threshold must be a finite number", lambda v: True)
    still = _number(still, "still must be a distance >= 0", lambda v: v >= 0)
    reach = _number(reach, "reach must lie in (0, 0.5)", lambda v: 0 < v < 0.5)
    if isinstance(blend, bool) or not isinstance(blend, int) or blend < 0:
        raise L.TcdiffError(f"foot_lock: blend must be an int >= 0, got {blend!r}")
    parents = SMPL_PARENTS if parents is None else parents
    offsets = SMPL_OFFSETS if offsets is None else offsets
    if len(parents) != 24 or len(offsets) != 24:
        raise L.TcdiffError("foot_lock: the skeleton has 24 joints")
    if not q.is_cuda or pos.device != q.device or (contacts is not None and contacts.device != q.device):
        raise L.TcdiffError("foot_lock runs on MI355X only (no CPU fallback): q, pos and contacts must be on one device")
    dev = q.device
    q, pos = q.detach().contiguous(), pos.detach().contiguous()
    workspace = torch.empty(K.foot_lock_workspace(b, dn, T), dtype=torch.uint8, device=dev)
    q_out = torch.empty_like(q)
    joints = torch.empty(b, dn, T, 24, 3, device=dev) if return_joints else None
    planted = torch.empty(b, dn, 2, dtype=torch.int32, device=dev)
    clamped = torch.empty(b, dn, 2, dtype=torch.int32, device=dev)
    max_shift = torch.empty(b, dn, 2, dtype=torch.float64, device=dev)
    K.foot_lock(q, pos, None if contacts is None else contacts.detach(), b, dn, T, thr, still, blend, reach, parents, offsets, workspace,
                q_out, joints, planted, clamped, max_shift)
    return FootLock(q_out, joints, planted, clamped, max_shift)
