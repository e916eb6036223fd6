"""Does a dancer TREMBLE, and a filter against it.  A diffusion sampler predicts its frames as independent rows, and what it returns
jitters from frame to frame in the rotations and the root: the fault still visible in every clip once the feet are pinned, the bodies
apart and the soles on the floor.  Two functions, on the device, float64 throughout (include/tcdiff_smooth.h is the definition,
csrc/smooth.hip runs it):

* ``smoothness(joints)``: the scores the motion literature reports as "Accel" (m/s^2) and "Jitter" (the mean jerk, m/s^3), per clip
  and dancer, in one launch: ``accel_mean``, ``jitter``, ``jitter_local`` (root-relative), ``root_jitter``, the two maxima with their
  frame and joint, and the ``terms`` counted.
* ``smooth(q, pos, dn=...)``: a Savitzky-Golay filter of what ``export_poses`` returns, in two launches for any number of clips: the
  root positions per component, the rotations as unit quaternions -- signed to the output frame's hemisphere, filtered in R^4,
  projected back to the unit sphere -- then the joints of the filtered poses by the export's FK.

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)
    s = smooth(q, pos, dn=dn)                      # s.q, s.pos, s.joints; s.before["jitter"], s.after["jitter"]

It belongs right after the export and before ``keep_apart``, ``ground`` and ``foot_lock``: those act on the joints, and run after the
filter each keeps its promise on the output.  ``window=9, polyorder=3`` are choices, not measurements: the reference's own smoother
(``smooth_data``, TrajDecoder/utils/utils_model.py:79-86: scipy's savgol_filter, window 21, order 3, per channel on the host) lowers
the jitter further but triples the error against a clean motion, 0.7 s being long for a dance; ``root_window=21`` is that filter on
the root.  The taps are those of ``savgol_filter(..., mode="interp")`` and are held to scipy on the CPU; the quaternion form, the
sign rule and the scores are the project's own and parity with any other tool is unpinned.  Not built: contact-aware taps, a filter
inside the sampler, a one-euro or Kalman filter, frequency-domain scores, smoothing the kinks that the correctors' linear envelopes
add after it.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .export import export_poses
from .fk import SMPL_OFFSETS, SMPL_PARENTS

MAX_WINDOW = L.SMOOTH.constants["TC_SMOOTH_MAX_WINDOW"]
ALL_JOINTS = (1 << 24) - 1
_TABLES = {}          # (window, polyorder, device) -> the table on that device


class Smooth(NamedTuple):
    q: torch.Tensor                  # (b, T dn, 24, 3) float32: the filtered rotation vectors
    pos: torch.Tensor                # (b, T dn, 3) float32: the filtered root positions
    joints: torch.Tensor             # (b, dn, T, 24, 3) float32: fk_forward of q and pos, in place of export_poses' third result
    max_rot_change: torch.Tensor     # (b, dn) float64: the largest rotation between an input and its output, in radians
    max_pos_change: torch.Tensor     # (b, dn) float64: the largest root displacement, in metres
    copied: torch.Tensor             # (b, dn) int32: the outputs copied through (a non-finite or degenerate window)
    window: tuple                    # (window, root_window)
    polyorder: tuple                 # (polyorder, root_polyorder)
    before: dict | None = None       # smoothness of the input's joints (measure=True)
    after: dict | None = None        # smoothness of `joints`


def savgol_table(window, polyorder) -> np.ndarray:
    """The (window, window) float64 tap table of include/tcdiff_smooth.h: A pinv(A) for the Vandermonde matrix A of the offsets
    -R .. R.  Row R holds the interior taps, the rows before and after it the polynomial fit of the first and last ``window`` frames:
    scipy's ``savgol_filter(..., mode="interp")``, restated with numpy."""
    _window(window, polyorder, "savgol_table", "window", "polyorder")
    R = (window - 1) // 2
    A = np.vander(np.arange(-R, R + 1, dtype=np.float64), polyorder + 1, increasing=True)
    return A @ np.linalg.pinv(A)


def _window(window, polyorder, who, wname, pname):
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 3 <= window <= MAX_WINDOW or window % 2 == 0:
        raise L.TcdiffError(f"{who}: {wname} must be an odd int in [3, {MAX_WINDOW}], got {window!r}")
    if isinstance(polyorder, bool) or not isinstance(polyorder, (int, np.integer)) or not 0 <= polyorder < window:
        raise L.TcdiffError(f"{who}: {pname} must be an int in [0, {wname}) = [0, {window}), got {polyorder!r}")
    return int(window), int(polyorder)


def _table_on(window, polyorder, dev):
    key = (window, polyorder, str(dev))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(savgol_table(window, polyorder)).to(dev)
    return _TABLES[key]


def _mask(joints_mask):
    if joints_mask is None:
        return ALL_JOINTS
    if isinstance(joints_mask, (int, np.integer)) and not isinstance(joints_mask, bool):
        if not 0 <= joints_mask <= ALL_JOINTS:
            raise L.TcdiffError(f"smooth: joints_mask must be 24 bits, got {joints_mask!r}")
        return int(joints_mask)
    try:
        js = list(joints_mask)
    except TypeError:
        raise L.TcdiffError(f"smooth: joints_mask must be 24 bits as an int, or the joints to filter, got {joints_mask!r}") from None
    m = 0
    for j in js:
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= j < 24:
            raise L.TcdiffError(f"smooth: joints_mask lists joints in 0 .. 23, got {j!r}")
        m |= 1 << int(j)
    return m


def _check_joints(joints, who="smoothness"):
    if not isinstance(joints, torch.Tensor) or joints.dim() != 5 or tuple(joints.shape[3:]) != (24, 3):
        raise L.TcdiffError(f"{who}: joints must be (b, dn, T, 24, 3), got "
                            f"{tuple(joints.shape) if isinstance(joints, torch.Tensor) else type(joints)}")
    if joints.dtype != torch.float32:
        raise L.TcdiffError(f"{who}: joints must be float32, got {joints.dtype}")
    if min(joints.shape[:3]) < 1:
        raise L.TcdiffError(f"{who}: joints {tuple(joints.shape)} has an empty dimension")
    if joints.shape[2] < 4:
        raise L.TcdiffError(f"{who}: a jerk takes 4 frames, got T = {joints.shape[2]}")
    if joints.stride(-1) != 1 or joints.stride(-2) != 3:
        raise L.TcdiffError(f"{who}: the trailing 2 dimension(s) of joints must be contiguous (strides {tuple(joints.stride())})")


def _fps(fps, who):
    if isinstance(fps, bool) or not isinstance(fps, (int, float)) or not 0 < fps <= 1e6:
        raise L.TcdiffError(f"{who}: fps must be a number in (0, 1e6], got {fps!r}")
    return float(fps)


def smoothness(joints, *, fps=30) -> dict:
    """joints (b, dn, T, 24, 3) float32 on the device, in metres, T >= 4, read in place through its strides (only the trailing 24 x 3
    must be contiguous: the permuted view of a frame-major buffer is read without a copy).

    Returns device tensors per clip and dancer, a dict that ``metrics.summarize`` takes as it is: float64 (b, dn) ``accel_mean``
    (the mean second difference of the joints, m/s^2), ``jitter`` (the mean third difference, m/s^3), ``jitter_local`` (the same of
    the root-relative positions of joints 1-23), ``root_jitter`` (of joint 0), ``accel_max`` and ``jitter_max``; int32 (b, dn, 2)
    ``accel_peak`` and ``jitter_peak`` (the frame and joint of the maximum; on a tie the lower frame, then the lower joint) and
    (b, dn) ``terms`` (the jitter terms counted).  A term with a non-finite input is left out and counted out of its mean; a mean
    over nothing is NaN.  One launch, nothing is copied to the host.  The definitions: include/tcdiff_smooth.h."""
    _check_joints(joints)
    fps = _fps(fps, "smoothness")
    if not joints.is_cuda:
        raise L.TcdiffError("smoothness runs on MI355X only (no CPU fallback)")
    b, dn = joints.shape[:2]
    dev = joints.device
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    out = {"accel_mean": f64(b, dn), "jitter": f64(b, dn), "jitter_local": f64(b, dn), "root_jitter": f64(b, dn), "accel_max": f64(b, dn),
           "jitter_max": f64(b, dn), "accel_peak": i32(b, dn, 2), "jitter_peak": i32(b, dn, 2), "terms": i32(b, dn)}
    with torch.cuda.device(dev):
        K.smoothness(joints.detach(), fps, *out.values())
    return out


def evaluate_smoothness(samples, normalizer, dn, mode="normal", **kw) -> dict:
    """The sampler's normalised samples (b, S * dn, 151) -> ``smoothness`` of the exported poses: ``export_poses``, then
    ``smoothness``, everything on the device.  In "long" mode the b windows are one song, so the result has one row."""
    _, _, poses, _ = export_poses(samples, normalizer, mode, dn)
    return smoothness(poses, **kw)


def smooth(q, pos, *, dn, window=9, polyorder=3, root_window=None, root_polyorder=None, joints_mask=None, parents=None, offsets=None,
           measure=True) -> Smooth:
    """``q`` (b, T dn, 24, 3) float32 rotation vectors and ``pos`` (b, T dn, 3) on the device, row = frame dn + dancer:
    ``export_poses``' first two results, in long mode too (b = 1).

    The rotations are filtered with (``window``, ``polyorder``), the root with (``root_window``, ``root_polyorder``), which default
    to the same; a window is odd, 3 .. 63 and at most T frames, an order below its window.  9 / 3 are choices, not measurements;
    ``root_window=21`` is the reference's ``smooth_data``.  ``joints_mask``: 24 bits as an int, or the joints to filter; the others
    are copied through bit for bit, and so is every output whose window holds a non-finite float (``copied`` counts those).

    Returns ``Smooth``: ``q``, ``pos`` and ``joints`` (b, dn, T, 24, 3) -- the FK of the filtered poses, in the layout ``foot_lock``
    returns its joints -- and per clip and dancer ``max_rot_change`` (radians), ``max_pos_change`` (metres) and ``copied``.  With
    ``measure`` also ``before`` and ``after``, the ``smoothness`` (at 30 fps) of the input's joints (from the same FK launch) and of
    the output's.  Two launches, plus one per measured side; the inputs are never changed, nothing synchronises, nothing is copied to
    the host.  ``parents`` / ``offsets`` default to the SMPL skeleton.  The definitions: include/tcdiff_smooth.h."""
    if not isinstance(q, torch.Tensor) or not isinstance(pos, torch.Tensor):
        raise L.TcdiffError("smooth: q and pos must be tensors")
    if q.dim() != 4 or tuple(q.shape[2:]) != (24, 3) or q.dtype != torch.float32:
        raise L.TcdiffError(f"smooth: q must be (b, frames * dancers, 24, 3) float32, got {tuple(q.shape)} {q.dtype}")
    b, n = q.shape[:2]
    if tuple(pos.shape) != (b, n, 3) or pos.dtype != torch.float32:
        raise L.TcdiffError(f"smooth: pos must be ({b}, {n}, 3) float32, got {tuple(pos.shape)} {pos.dtype}")
    if isinstance(dn, bool) or not isinstance(dn, int) or dn < 1 or b < 1 or n < 1 or n % dn:
        raise L.TcdiffError(f"smooth: {n} rows are not a whole number of frames of {dn!r} dancers")
    T = n // dn
    window, polyorder = _window(window, polyorder, "smooth", "window", "polyorder")
    root_window, root_polyorder = _window(window if root_window is None else root_window, polyorder if root_polyorder is None else root_polyorder,
                                          "smooth", "root_window", "root_polyorder")
    if T < max(window, root_window):
        raise L.TcdiffError(f"smooth: a window of {max(window, root_window)} frames needs T >= {max(window, root_window)}, got T = {T}")
    mask = _mask(joints_mask)
    if not isinstance(measure, bool):
        raise L.TcdiffError(f"smooth: measure must be a bool, got {measure!r}")
    if measure and T < 4:
        raise L.TcdiffError(f"smooth: measure=True scores the jerk, which takes 4 frames, got T = {T}")
    parents = SMPL_PARENTS if parents is None else parents
    offsets = SMPL_OFFSETS if offsets is None else offsets
    if len(parents) != 24 or len(offsets) != 24:
        raise L.TcdiffError("smooth: the skeleton has 24 joints")
    if any(int(parents[j]) >= j for j in range(24)):
        raise L.TcdiffError(f"smooth: every parent must precede its child, got parents {list(parents)!r}")
    if math.prod((b, dn, T)) > 2 ** 31 - 1:
        raise L.TcdiffError(f"smooth: {b} x {dn} x {T} frame slots are more than 2^31 - 1")
    if not q.is_cuda or pos.device != q.device:
        raise L.TcdiffError("smooth runs on MI355X only (no CPU fallback): q and pos must be on one device")
    dev = q.device
    q, pos = q.detach().contiguous(), pos.detach().contiguous()
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        taps, root_taps = _table_on(window, polyorder, dev), _table_on(root_window, root_polyorder, dev)
        workspace = torch.empty(K.smooth_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        q_out, pos_out = torch.empty_like(q), torch.empty_like(pos)
        joints = torch.empty(b, dn, T, 24, 3, device=dev)
        joints_in = torch.empty(b, dn, T, 24, 3, device=dev) if measure else None
        max_rot, max_pos, copied = f64(b, dn), f64(b, dn), torch.empty(b, dn, dtype=torch.int32, device=dev)
        K.smooth(q, pos, b, dn, T, window, taps, root_window, root_taps, mask, parents, offsets, workspace, q_out, pos_out, joints, joints_in,
                 max_rot, max_pos, copied)
    before = after = None
    if measure:
        before, after = smoothness(joints_in), smoothness(joints)
    return Smooth(q_out, pos_out, joints, max_rot, max_pos, copied, (window, root_window), (polyorder, root_polyorder), before, after)
