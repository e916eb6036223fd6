"""Putting the dancers on the floor: a floor measure and a post-process on what ``export_poses`` returns, on the device.  The floor is
given or estimated (the median of the planted feet's lows); each dancer's root is shifted VERTICALLY so that its planted feet stand on
the floor and no capsule of ``group_metrics``' body sinks below it, and the shift is eased in and out over ``blend`` frames; rotations
and the two floor components are untouched.  include/tcdiff_ground.h is the definition; ``tcf_ground_metrics`` and ``tcf_ground``
(csrc/ground.hip) run it in three and five launches for any number of clips.

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)
    apart = keep_apart(pos, poses, dn=dn)
    grounded = ground(apart.pos, apart.joints, contacts, dn=dn)
    locked = foot_lock(q, grounded.pos, contacts, dn=dn)      # afterwards: it pins feet that already stand on the floor

The reference has no counterpart: it renders the raw poses.  The construction is the project's own, in the spirit of the "penetrate"
and "float" scores of the physics-plausibility literature; parity with any other tool is unpinned.  ``tolerance``, ``blend``,
``max_lift`` and the default radii are choices, not measurements.  Not built: mesh-level soles from ``skin``'s vertices, sloped or
uneven floors, a floor per dancer, bending knees to absorb a correction, correcting inside the sampler, drawing the grid at the
estimated floor.
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

MAX_DANCERS = L.GROUND.constants["TC_GROUND_MAX_DANCERS"]
MAX_BLEND = L.GROUND.constants["TC_GROUND_MAX_BLEND"]
COUNTS = ("planted_frames", "penetration_frames", "float_frames")          # int64 (b, dn)
VALUES = ("penetration_max", "penetration_mean", "float_mean")             # float64 (b, dn)
METRICS = ("floor",) + COUNTS + VALUES


class Ground(NamedTuple):
    pos: torch.Tensor                  # (b, T dn, 3) float32: the shifted root positions
    joints: torch.Tensor               # (b, dn, T, 24, 3) float32, contiguous: the shifted joints
    floor: torch.Tensor                # (b,) float64: the floor used, given or estimated
    before: dict                       # ground_metrics' keys, on the input
    after: dict                        # the same on the outputs, with the input's labels
    capped: torch.Tensor               # (b, dn) int64: frames whose lift was clamped to max_lift
    max_shift: torch.Tensor            # (b, dn) float64: the largest |shift|, metres
    max_step: torch.Tensor             # (b, dn) float64: the largest change of the shift from one frame to the next
    shift: torch.Tensor | None         # (b, dn, T) float64: the vertical shift, with return_shift


def _fail(fn, msg):
    raise L.TcdiffError(f"{fn}: {msg}")


def _number(fn, v, what, lo=None):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or (lo is not None and v < lo):
        _fail(fn, f"{what} must be a finite number{'' if lo is None else f' >= {lo}'}, got {v!r}")
    return float(v)


def _args(fn, joints, contacts, floor, up, radii, parents, contact_threshold, still, tolerance):
    """the checks both functions share; -> (b, dn, T, floor_in tensor or None, radii list, parents list, thr, still, tolerance)"""
    if not isinstance(joints, torch.Tensor):
        _fail(fn, "joints must be a tensor")
    if joints.dim() != 5 or tuple(joints.shape[3:]) != (24, 3) or joints.dtype != torch.float32:
        _fail(fn, f"joints must be (b, dn, T, 24, 3) float32, got {tuple(joints.shape)} {joints.dtype}")
    if min(joints.shape[:3]) < 1:
        _fail(fn, f"joints {tuple(joints.shape)} has an empty dimension")
    if joints.stride(-1) != 1 or joints.stride(-2) != 3:
        _fail(fn, f"the trailing 2 dimension(s) of joints must be contiguous (strides {tuple(joints.stride())})")
    b, dn, T = joints.shape[:3]
    if dn > MAX_DANCERS:
        _fail(fn, f"at most {MAX_DANCERS} dancers, got {dn}")
    if contacts is not None and (not isinstance(contacts, torch.Tensor) or tuple(contacts.shape) != (b, dn, T, 4) or
                                 contacts.dtype != torch.float32):
        _fail(fn, f"contacts must be ({b}, {dn}, {T}, 4) float32 or None")
    if isinstance(up, bool) or up not in (0, 1, 2):
        _fail(fn, f"up must be 0, 1 or 2, got {up!r}")
    thr = _number(fn, contact_threshold, "contact_threshold")
    still, tolerance = _number(fn, still, "still", 0), _number(fn, tolerance, "tolerance", 0)
    try:
        radii = capsule_radii() if radii is None else np.array(radii, np.float64)
    except (TypeError, ValueError):
        radii = np.empty(0)
    if radii.shape != (24,) or not np.isfinite(radii[1:]).all() or (radii[1:] < 0).any():
        _fail(fn, "radii must be 24 finite numbers >= 0 (entry 0 is unused)")
    parents = list(SMPL_PARENTS if parents is None else parents)
    if len(parents) != 24 or any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) for p in parents) or \
            any(not 0 <= parents[j] < j for j in range(1, 24)):
        _fail(fn, "parents must be 24 ints, every parent before its child")
    floor_in = None
    if isinstance(floor, torch.Tensor):
        if tuple(floor.shape) != (b,) or floor.dtype != torch.float64:
            _fail(fn, f"a floor tensor must be ({b},) float64, got {tuple(floor.shape)} {floor.dtype}")
        floor_in = floor
    elif floor is not None:
        floor = _number(fn, floor, "floor (None, a number or a (b,) float64 tensor)")
    return (b, dn, T, floor if floor_in is None else floor_in, radii.tolist(), [0 if j == 0 else int(p) for j, p in enumerate(parents)], thr,
            still, tolerance)


def _on_device(fn, joints, contacts, floor, pos=None):
    """the last check, then the floor as the launchers take it: None or a (b,) float64 device tensor"""
    if not joints.is_cuda or (contacts is not None and contacts.device != joints.device) or \
            (isinstance(floor, torch.Tensor) and floor.device != joints.device) or (pos is not None and pos.device != joints.device):
        _fail(fn, "runs on MI355X only (no CPU fallback): pos, joints, contacts and floor must be on one device")
    if floor is None or isinstance(floor, torch.Tensor):
        return None if floor is None else floor.detach().contiguous()
    return torch.full((joints.shape[0],), floor, dtype=torch.float64, device=joints.device)


def _metrics(floor, counts, values):
    out = {"floor": floor}
    out.update({k: counts[n] for n, k in enumerate(COUNTS)})
    out.update({k: values[n] for n, k in enumerate(VALUES)})
    return out


def ground_metrics(joints, contacts=None, *, floor=None, up=2, radii=None, parents=None, contact_threshold=0.95, still=0.01,
                   tolerance=0.005) -> dict:
    """How the dancers stand on the floor.  ``joints`` (b, dn, T, 24, 3) float32 on the device, in metres, read in place through its
    strides (only the trailing 24 x 3 must be contiguous); ``contacts`` (b, dn, T, 4) float32 for the joints 7, 8, 10, 11, as
    ``foot_lock`` takes them, or None: then a foot is planted where its ankle or toe moves less than ``still`` metres to the next
    frame.  ``floor``: None (estimated per clip: the median of the planted feet's lows, of the body's lows if nothing is planted), a
    number, or a (b,) float64 device tensor.  ``radii`` / ``parents`` as for ``group_metrics`` (``radii_from_body`` works too).

    Returns a dict of device tensors that ``metrics.summarize`` takes as it is: ``floor`` (b,) float64; ``planted_frames``,
    ``penetration_frames`` (the body more than ``tolerance`` below the floor) and ``float_frames`` (the planted feet more than
    ``tolerance`` above it), int64 (b, dn); ``penetration_max``, ``penetration_mean`` (over the frames whose joints are finite) and
    ``float_mean`` (over the planted frames, NaN without one), float64 (b, dn), metres.  ``tolerance`` = 5 mm and the default radii are
    choices, not measurements.  Nothing synchronises, nothing is copied to the host.  The definition: include/tcdiff_ground.h."""
    b, dn, T, floor_in, radii, parents, thr, still, tolerance = _args("ground_metrics", joints, contacts, floor, up, radii, parents,
                                                                      contact_threshold, still, tolerance)
    floor_in = _on_device("ground_metrics", joints, contacts, floor_in)
    dev = joints.device
    out_floor = torch.empty(b, dtype=torch.float64, device=dev)
    counts = torch.empty(3, b, dn, dtype=torch.int64, device=dev)
    values = torch.empty(3, b, dn, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        workspace = torch.empty(K.ground_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        K.ground_metrics(joints.detach(), None if contacts is None else contacts.detach(), int(up), parents, radii, floor_in, thr, still,
                         tolerance, workspace, out_floor, counts, values)
    return _metrics(out_floor, counts, values)


def ground(pos, joints, contacts=None, *, dn, floor=None, up=2, radii=None, parents=None, contact_threshold=0.95, still=0.01,
           tolerance=0.005, blend=5, max_lift=0.5, return_shift=False) -> Ground:
    """``pos`` (b, T dn, 3) float32, row = frame dn + dancer, and ``joints`` (b, dn, T, 24, 3) float32 on the device: ``export_poses``'
    second and third result (or ``keep_apart``'s).  ``contacts``, ``floor``, ``radii``, ``parents``, ``contact_threshold``, ``still``
    and ``tolerance`` as for ``ground_metrics``.

    Over each run of planted frames the root is shifted by the mean of (floor - the planted feet's low), so the run stands on the floor
    on average; between two runs at most ``2 blend`` frames apart the shift is bridged linearly, elsewhere it fades over ``blend``
    frames.  Where any capsule of the body is still below the floor, a lift is added and spread over ``blend`` frames to either side by
    a linear envelope.  The shift is clamped to ``max_lift`` metres (``capped`` counts those frames).  A jump further than ``blend``
    frames from every run is left alone.  ``blend = 5``, ``max_lift = 0.5``, ``tolerance = 0.005`` and the default radii are choices,
    not measurements.

    Returns a ``Ground``: the shifted ``pos`` and ``joints``, the ``floor`` used, ``before`` and ``after`` (``ground_metrics``' keys;
    "after" on the float32 outputs, with the labels of the input), ``capped``, ``max_shift``, ``max_step`` and, with
    ``return_shift``, the shift itself.  Frames whose shift is 0, and frames whose joints are not all finite, keep their bits.
    Nothing synchronises, nothing is copied to the host.  The definition: include/tcdiff_ground.h."""
    if not isinstance(pos, torch.Tensor):
        _fail("ground", "pos must be a tensor")
    b, jdn, T, floor_in, radii, parents, thr, still, tolerance = _args("ground", joints, contacts, floor, up, radii, parents,
                                                                       contact_threshold, still, tolerance)
    if isinstance(dn, bool) or not isinstance(dn, (int, np.integer)) or dn != jdn:
        _fail("ground", f"dn must be the joints' number of dancers, {jdn}, got {dn!r}")
    dn = int(dn)
    if tuple(pos.shape) != (b, T * dn, 3) or pos.dtype != torch.float32:
        _fail("ground", f"pos must be ({b}, {T * dn}, 3) float32, got {tuple(pos.shape)} {pos.dtype}")
    if isinstance(blend, bool) or not isinstance(blend, (int, np.integer)) or not 0 <= blend <= MAX_BLEND:
        _fail("ground", f"blend must be an int in [0, {MAX_BLEND}], got {blend!r}")
    max_lift = _number("ground", max_lift, "max_lift", 0)
    floor_in = _on_device("ground", joints, contacts, floor_in, pos)
    dev = joints.device
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)
    pos = pos.detach().contiguous()
    out_floor, cb, vb, ca, va = f64(b), i64(3, b, dn), f64(3, b, dn), i64(3, b, dn), f64(3, b, dn)
    out = Ground(torch.empty_like(pos), torch.empty(b, dn, T, 24, 3, dtype=torch.float32, device=dev), out_floor, _metrics(out_floor, cb, vb),
                 _metrics(out_floor, ca, va), i64(b, dn), f64(b, dn), f64(b, dn), f64(b, dn, T) if return_shift else None)
    with torch.cuda.device(dev):
        workspace = torch.empty(K.ground_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        K.ground(pos, joints.detach(), None if contacts is None else contacts.detach(), int(up), parents, radii, floor_in, thr, still,
                 tolerance, int(blend), max_lift, workspace, out.pos, out.joints, out.shift, out_floor, cb, vb, ca, va, out.capped,
                 out.max_shift, out.max_step)
    return out
