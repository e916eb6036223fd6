"""Keeping the dancers' bodies apart: a post-process on what ``export_poses`` returns, on the device.  Where the capsule bodies of
``group_metrics`` come closer than ``margin``, the two roots are shifted apart HORIZONTALLY along the line between them, as little as
the bodies require, and the shift is eased in and out over ``blend`` frames; rotations are untouched, so every limb keeps its pose.
include/tcdiff_apart.h is the definition; ``tcp_keep_apart`` (csrc/apart.hip) runs it in 2 ``rounds`` + 3 launches for any number of
clips and reports what it did (``pushed``, ``max_shift``, ``max_step``) and what it could not do (``capped``, ``contact_after``).

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)
    apart = keep_apart(pos, poses, dn=dn)
    locked = foot_lock(q, apart.pos, contacts, dn=dn)          # afterwards: a shifted root slides a planted foot, this re-pins it

The reference has no counterpart: it renders the raw poses.  The construction is the project's own; parity with any other tool is
unpinned.  ``margin``, ``iterations``, ``rounds``, ``blend`` and ``max_push`` are choices, not measurements.  Not promised: with three
or more dancers a push that clears one pair can close another; rounds reduce that but need not end it.  Not built: vertical moves,
changing a pose to dodge, resolving inside the sampler, mesh-level contact, resolving a contact between parts of one dancer
(``self_contact``, tcdiff_amd/self_contact.py, measures it), smoothing beyond the envelope.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .fk import SMPL_PARENTS
from .group_metrics import capsule_radii

MAX_DANCERS = L.APART.constants["TC_APART_MAX_DANCERS"]
MAX_BLEND = L.APART.constants["TC_APART_MAX_BLEND"]
MAX_ROUNDS = L.APART.constants["TC_APART_MAX_ROUNDS"]


class Apart(NamedTuple):
    pos: torch.Tensor                  # (b, T dn, 3) float32: the shifted root positions
    joints: torch.Tensor               # (b, dn, T, 24, 3) float32, contiguous: the shifted joints
    contact_before: torch.Tensor       # (b, P) int64: frames with gap < 0, on the input
    contact_after: torch.Tensor        # (b, P) int64: the same on the joints returned
    gap_min_before: torch.Tensor       # (b, P) float64: the smallest finite gap, NaN if none
    gap_min_after: torch.Tensor        # (b, P) float64
    pushed: torch.Tensor               # (b, P) int64: frames that some round pushed
    capped: torch.Tensor               # (b, P) int64: frames that some round capped at max_push
    max_shift: torch.Tensor            # (b, dn) float64: the largest length of the final shift, metres
    max_step: torch.Tensor             # (b, dn) float64: the largest change of the shift from one frame to the next
    shift: torch.Tensor | None         # (b, dn, T, 2) float64: the final shift of the two floor components, with return_shift


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
        raise L.TcdiffError(f"keep_apart: {what} must be a finite number >= 0, got {v!r}")
    return float(v)


def _int(v, what, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v > hi:
        raise L.TcdiffError(f"keep_apart: {what} must be an int in [0, {hi}], got {v!r}")
    return int(v)


def keep_apart(pos, joints, *, dn, up=2, radii=None, parents=None, margin=0.02, iterations=8, rounds=3, blend=5, max_push=0.6,
               mobility=None, return_shift=False) -> Apart:
    """``pos`` (b, T dn, 3) float32, row = frame dn + dancer, and ``joints`` (b, dn, T, 24, 3) float32 on the device, in metres:
    ``export_poses``' second and third result (or ``foot_lock``'s joints).  The joints are read in place through their strides, as
    ``group_metrics`` reads them.  ``radii`` and ``parents`` as for ``group_metrics`` (``radii_from_body`` works too).

    Per round, every pair of dancers and frame asks for the push ``m`` along the line between the two roots that opens the gap to
    ``margin`` (at most ``iterations`` steps, at most ``max_push`` metres: a frame that reaches it is *capped*); the pushes are spread
    over ``blend`` frames to either side by a linear envelope and shared by ``mobility`` (``dn`` numbers >= 0, default all 1: a
    dancer of mobility 0 stays on the trajectory it was given; two such dancers are left alone).  ``rounds`` rounds, because with
    three or more dancers a push that clears one pair can close another.  ``margin=0.02``, ``iterations=8``, ``rounds=3``,
    ``blend=5`` and ``max_push=0.6`` are choices, not measurements.

    Returns an ``Apart``.  Where the final shift is 0 the outputs hold the input's bits; "after" is evaluated on the float32 joints
    that are returned.  Nothing synchronises, nothing is copied to the host.  One dancer: the inputs are returned as they are and the
    per-pair results are empty.  The definition: include/tcdiff_apart.h."""
    if not isinstance(pos, torch.Tensor) or not isinstance(joints, torch.Tensor):
        raise L.TcdiffError("keep_apart: pos and joints must be tensors")
    if joints.dim() != 5 or tuple(joints.shape[3:]) != (24, 3) or joints.dtype != torch.float32:
        raise L.TcdiffError(f"keep_apart: joints must be (b, dn, T, 24, 3) float32, got {tuple(joints.shape)} {joints.dtype}")
    if min(joints.shape[:3]) < 1:
        raise L.TcdiffError(f"keep_apart: joints {tuple(joints.shape)} has an empty dimension")
    if joints.stride(-1) != 1 or joints.stride(-2) != 3:
        raise L.TcdiffError(f"keep_apart: the trailing 2 dimension(s) of joints must be contiguous (strides {tuple(joints.stride())})")
    b, jdn, T = joints.shape[:3]
    if isinstance(dn, bool) or not isinstance(dn, (int, np.integer)) or dn != jdn:
        raise L.TcdiffError(f"keep_apart: dn must be the joints' number of dancers, {jdn}, got {dn!r}")
    dn = int(dn)
    if dn > MAX_DANCERS:
        raise L.TcdiffError(f"keep_apart: at most {MAX_DANCERS} dancers, got {dn}")
    if tuple(pos.shape) != (b, T * dn, 3) or pos.dtype != torch.float32:
        raise L.TcdiffError(f"keep_apart: pos must be ({b}, {T * dn}, 3) float32, got {tuple(pos.shape)} {pos.dtype}")
    if isinstance(up, bool) or up not in (0, 1, 2):
        raise L.TcdiffError(f"keep_apart: up must be 0, 1 or 2, got {up!r}")
    margin, max_push = _number(margin, "margin"), _number(max_push, "max_push")
    iterations, rounds, blend = _int(iterations, "iterations", 2 ** 31 - 1), _int(rounds, "rounds", MAX_ROUNDS), _int(blend, "blend", MAX_BLEND)
    radii = capsule_radii() if radii is None else np.asarray(radii, np.float64)
    if radii.shape != (24,) or not np.isfinite(radii[1:]).all() or (radii[1:] < 0).any():
        raise L.TcdiffError("keep_apart: radii must be 24 finite numbers >= 0 (entry 0 is unused)")
    parents = list(SMPL_PARENTS if parents is None else parents)
    if len(parents) != 24 or any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) for p in parents) or \
            any(not 0 <= parents[j] < j for j in range(1, 24)):
        raise L.TcdiffError("keep_apart: parents must be 24 ints, every parent before its child")
    try:
        mobility = np.ones(dn) if mobility is None else np.array(mobility, np.float64)
    except (TypeError, ValueError):
        mobility = np.empty(0)
    if mobility.shape != (dn,) or not np.isfinite(mobility).all() or (mobility < 0).any():
        raise L.TcdiffError(f"keep_apart: mobility must be {dn} finite numbers >= 0")
    if not joints.is_cuda or pos.device != joints.device:
        raise L.TcdiffError("keep_apart runs on MI355X only (no CPU fallback): pos and joints must be on one device")
    dev = joints.device
    P = dn * (dn - 1) // 2
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)
    if P == 0:
        zero = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
        return Apart(pos, joints, i64(b, 0), i64(b, 0), f64(b, 0), f64(b, 0), i64(b, 0), i64(b, 0), zero(b, 1), zero(b, 1),
                     zero(b, 1, T, 2) if return_shift else None)
    pos, joints = pos.detach().contiguous(), joints.detach()
    out = Apart(torch.empty_like(pos), torch.empty(b, dn, T, 24, 3, dtype=torch.float32, device=dev), i64(b, P), i64(b, P), f64(b, P), f64(b, P),
                i64(b, P), i64(b, P), f64(b, dn), f64(b, dn), f64(b, dn, T, 2) if return_shift else None)
    with torch.cuda.device(dev):
        workspace = torch.empty(K.keep_apart_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        K.keep_apart(pos, joints, int(up), [0 if j == 0 else int(p) for j, p in enumerate(parents)], radii.tolist(), mobility.tolist(), margin,
                     iterations, rounds, blend, max_push, workspace, out.pos, out.joints, out.shift, out.contact_before, out.contact_after,
                     out.gap_min_before, out.gap_min_after, out.pushed, out.capped, out.max_shift, out.max_step)
    return out
