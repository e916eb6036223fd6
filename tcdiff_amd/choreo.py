"""Say WHERE the dancers go, and check that they went there.  The model is a trajectory-controllable diffusion: every sampler takes
``x_0=``, the floor path of each dancer, and in-paints it into channels 4 and 5.  Until now an ``x_0`` came from a dataset clip
(``io.x0_from_motion``), from the Navigator (``navigator.rollout_x0`` / ``smooth_x0``) or from a full per-frame path that was already
normalised (``io.x0_from_trajectory``); nothing went from "line at 0 s, circle at 4 s, swap the outer two by 8 s" in metres to that
tensor, and after sampling no score said whether the dancers followed the path.  Three functions (include/tcdiff_choreo.h is the
definition, csrc/choreo.hip runs it on the device, float64 throughout):

* ``formation(name, dn)``: the floor positions of a named formation, on the host, a few lines.
* ``plan(keys, points, frames)``: waypoints in metres -> the per-frame trajectory and ``x_0``, with a report of what is wrong with the
  plan (bad keys, frames outside the normaliser's range, speeds, distances between the dancers), in two launches.
* ``trajectory_error(joints, traj)``: how far each dancer's root is from the planned path, in one launch.

    pts = np.stack([formation("line", 3), formation("circle", 3), formation("circle", 3, angle=np.pi)], 1)[None]      # (1, 3, K, 2)
    p = plan([0, 120, 240], pts, 300, normalizer=normalizer)
    samples = diffusion.ddim_sample(shape, cond, x_0=p.x_0)
    _, _, poses, _ = export_poses(samples, normalizer, "normal", 3)
    print(summarize(trajectory_error(poses, p.traj)))

The interpolant is PCHIP (Fritsch-Carlson, with the Fritsch-Butland slopes) as scipy's ``PchipInterpolator`` evaluates it, held to it
on the CPU: a choreography HOLDS formations, so two equal consecutive waypoints must give a dancer who stands still and a move must
not overshoot its target, and a natural or Catmull-Rom spline does neither.  The reference has no counterpart
(``given_trajectory_generation_loop`` only replays dataset trajectories); parity with any tool but scipy's interpolator is unpinned.
``min_distance`` and ``max_speed`` are choices, not measurements: they only set what ``too_close`` and ``too_fast`` count.
Not built: moving planned paths apart where they come too close (the report only says so; ``keep_apart`` acts after sampling),
snapping keys to the beat track, facing direction, per-dancer height, drawing the plan, waypoints at fractional frames, other
interpolants.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import kernels as K

MAX_KEYS = L.CHOREO.constants["TC_CHOREO_MAX_KEYS"]
FORMATIONS = ("line", "column", "circle", "v", "grid")


class Plan(NamedTuple):
    traj: torch.Tensor               # (b, dn, frames, 2) float32: the path in metres
    x_0: torch.Tensor                # (b, frames dn, 3) float32: what the samplers' x_0= takes, row = frame dn + dancer
    status: torch.Tensor             # (b, dn) int32: 0 fine, 1 bad keys, 2 a non-finite point (then the dancer's rows are NaN)
    clamped: torch.Tensor            # (b, dn) int32: frames with a channel outside the normaliser's [-1, 1]
    speed_max: torch.Tensor          # (b, dn) float64: the largest frame-to-frame speed, m/s
    speed_peak: torch.Tensor         # (b, dn) int32: its frame (on a tie the lower)
    too_fast: torch.Tensor           # (b, dn) int32: frames above max_speed
    path_length: torch.Tensor        # (b, dn) float64: metres
    dist_min: torch.Tensor           # (b, pairs) float64: the smallest distance of two dancers' roots, in the order of pairs(dn)
    dist_min_frame: torch.Tensor     # (b, pairs) int32: its frame (on a tie the lower)
    too_close: torch.Tensor          # (b, pairs) int32: frames closer than min_distance
    columns: tuple | None            # the normaliser's two columns, None without a normaliser


def formation(name, dn, *, spacing=1.0, center=(0, 0), angle=0.0) -> np.ndarray:
    """The floor positions (dn, 2) float32 (numpy, what ``plan`` copies up) of dancers 0 .. dn-1 in a named formation, in metres.
    Before the turn and the shift, with s = ``spacing`` and i the dancer:

    * ``"line"``: side by side along x, (i s, 0).
    * ``"column"``: one behind the other along y, (0, -i s).
    * ``"circle"``: (r cos(2 pi i / dn), r sin(2 pi i / dn)) with r = s / (2 sin(pi / dn)), so that neighbours are s apart; r = 0
      for one dancer.
    * ``"v"``: dancer 0 at the tip, the others alternately on the right and left arm, one step of s along a diagonal each:
      with k = (i + 1) // 2 and side = +1 for odd i, -1 for even i: (side k s / sqrt 2, -k s / sqrt 2).
    * ``"grid"``: rows of c = ceil(sqrt(dn)) dancers, (i % c) s, -(i // c) s.

    Then the centroid is subtracted, every position is turned counter-clockwise by ``angle`` (radians) and ``center`` is added: each
    formation is centred on ``center``."""
    if name not in FORMATIONS:
        raise L.TcdiffError(f"formation: name must be one of {FORMATIONS}, got {name!r}")
    if isinstance(dn, bool) or not isinstance(dn, (int, np.integer)) or dn < 1:
        raise L.TcdiffError(f"formation: dn must be an int >= 1, got {dn!r}")
    try:
        s, a, (cx, cy) = float(spacing), float(angle), (float(v) for v in center)
    except (TypeError, ValueError):
        raise L.TcdiffError(f"formation: spacing and angle must be numbers and center two numbers, got {spacing!r}, {angle!r}, {center!r}") from None
    if not (math.isfinite(s) and s >= 0 and math.isfinite(a) and math.isfinite(cx) and math.isfinite(cy)):
        raise L.TcdiffError(f"formation: spacing must be finite and >= 0, angle and center finite, got {spacing!r}, {angle!r}, {center!r}")
    i = np.arange(dn, dtype=np.float64)
    if name == "line":
        p = np.stack([i * s, 0 * i], 1)
    elif name == "column":
        p = np.stack([0 * i, -i * s], 1)
    elif name == "circle":
        r = s / (2 * math.sin(math.pi / dn)) if dn > 1 else 0.0
        p = np.stack([r * np.cos(2 * math.pi * i / dn), r * np.sin(2 * math.pi * i / dn)], 1)
    elif name == "v":
        k, side = (np.arange(dn) + 1) // 2, np.where(np.arange(dn) % 2 == 1, 1.0, -1.0)
        p = np.stack([side * k * s / math.sqrt(2), -k * s / math.sqrt(2)], 1)
    else:
        c = math.ceil(math.sqrt(dn))
        p = np.stack([(np.arange(dn) % c) * s, -(np.arange(dn) // c) * s], 1)
    p = p - p.mean(0)
    rot = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    return (p @ rot.T + np.array([cx, cy])).astype(np.float32)


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else type(x).__name__


def _host(x, what, kind):
    """a list or numpy array as a numpy array of the launch's dtype; a tensor stays what it is"""
    if isinstance(x, torch.Tensor):
        return x
    try:
        a = np.asarray(x)
    except (TypeError, ValueError):
        raise L.TcdiffError(f"plan: {what} must be a tensor, a numpy array or nested lists, got {type(x).__name__}") from None
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer if kind == "i" else np.number) or np.issubdtype(a.dtype, np.complexfloating):
        raise L.TcdiffError(f"plan: {what} must hold {'integers' if kind == 'i' else 'real numbers'}, got dtype {a.dtype}")
    if kind == "i" and a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise L.TcdiffError(f"plan: {what} must fit int32")
    return np.ascontiguousarray(a, np.int32 if kind == "i" else np.float32)


def _fps(fps, who):
    if isinstance(fps, bool) or not isinstance(fps, (int, float)) or not 0 < fps <= 1e6:
        raise L.TcdiffError(f"{who}: fps must be a number in (0, 1e6], got {fps!r}")
    return float(fps)


def _limit(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0:
        raise L.TcdiffError(f"plan: {name} must be a number >= 0, got {v!r}")
    return float(v)


def _columns(normalizer, columns):
    """the normaliser's numbers of the two columns, as host floats"""
    if normalizer is None:
        if columns is not None:
            raise L.TcdiffError("plan: columns without a normalizer")
        return None, None, None
    try:
        scale = normalizer.scaler.scale_.detach().to("cpu", torch.float32).reshape(-1).tolist()
        min_ = normalizer.scaler.min_.detach().to("cpu", torch.float32).reshape(-1).tolist()
    except AttributeError:
        raise L.TcdiffError("plan: normalizer must carry a fitted scaler.scale_ / scaler.min_ (io.Normalizer)") from None
    n = len(scale)
    if columns is None:
        if n != 3 and n < 6:
            raise L.TcdiffError(f"plan: a normalizer fitted on {n} columns has too few columns: 3 (x, y, z: the Navigator's) or at least 6 "
                                f"(the motion's, trajectory in 4 and 5), or give columns=")
        columns = (0, 1) if n == 3 else (4, 5)
    try:
        columns = tuple(columns)
    except TypeError:
        columns = ()
    if len(columns) != 2 or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0 for c in columns):
        raise L.TcdiffError(f"plan: columns must be two ints >= 0, got {columns!r}")
    if len(min_) != n or max(columns) >= n:
        raise L.TcdiffError(f"plan: a normalizer fitted on {n} columns has too few columns for columns={columns!r}")
    columns = (int(columns[0]), int(columns[1]))
    return [scale[c] for c in columns], [min_[c] for c in columns], columns


def _overlap(a, b):
    return a.data_ptr() < b.data_ptr() + b.numel() * b.element_size() and b.data_ptr() < a.data_ptr() + a.numel() * a.element_size()


def plan(keys, points, frames, *, counts=None, fps=30, normalizer=None, columns=None, min_distance=0.5, max_speed=3.0, out=None) -> Plan:
    """Waypoints -> the per-frame floor path of every dancer and the samplers' ``x_0``.

    ``points`` (b, dn, K, 2) float32: floor positions in metres, x and y of the data's Z-up frame (that of ``export_poses``' ``pos``
    with ``up=2``).  ``keys`` (K,) for all dancers or (b, dn, K), int32: the frames at which they hold, strictly ascending, in
    [0, frames).  ``counts`` (b, dn) int32, optional: how many of the K one dancer uses; the rest is padding and is never read.
    1 <= count <= K <= 256, ``frames`` >= 1.  Tensors on the device are read where they are; lists and numpy arrays are copied up
    once.  Between the keys the path is PCHIP per component (holds are held, targets are not overshot); before the first key it holds
    the first point, after the last key the last.

    Returns ``Plan``: ``traj`` (b, dn, frames, 2) in metres and ``x_0`` (b, frames dn, 3), row = frame dn + dancer, channels 0 and 1 the
    path in the units of ``normalizer``'s ``columns`` -- (4, 5) for one fitted on at least 6 columns, (0, 1) for one fitted on 3, the
    Navigator's -- clamped to [-1, 1], channel 2 zero: the layout of ``io.x0_from_trajectory`` and ``smooth_x0``; without a normalizer
    ``x_0`` carries metres.  ``out=`` receives ``x_0``.  The report per (clip, dancer): ``status`` (0 fine; 1 keys not strictly
    ascending or outside [0, frames), or a count outside 1 .. K; 2 a non-finite point: then the dancer's rows are NaN), ``clamped``
    (frames outside the normaliser's range: "this formation lies outside anything the model was trained on"), ``speed_max`` (m/s, of
    the stored values) with its frame ``speed_peak``, ``too_fast`` (frames above ``max_speed``), ``path_length``; per (clip, pair) in
    the order of ``group_metrics.pairs(dn)``: ``dist_min`` with ``dist_min_frame`` and ``too_close`` (frames closer than
    ``min_distance``); frames with a NaN are left out, with one dancer the three are empty.  ``min_distance=0.5`` and
    ``max_speed=3.0`` are choices, not measurements.

    Two launches (one with one dancer); the keys are checked in the kernel, nothing synchronises, nothing comes to the host.  A
    normalizer's four numbers are read on the host and travel as kernel arguments, as in ``smooth_x0``.  The definitions:
    include/tcdiff_choreo.h."""
    points, keys = _host(points, "points", "f"), _host(keys, "keys", "i")
    counts = None if counts is None else _host(counts, "counts", "i")
    if points.ndim != 4 or points.shape[-1] != 2 or min(points.shape) < 1:
        raise L.TcdiffError(f"plan: points must be (b, dn, K, 2), got {_shape(points)}")
    if isinstance(points, torch.Tensor) and points.dtype != torch.float32:
        raise L.TcdiffError(f"plan: points must be float32, got {points.dtype}")
    b, dn, nk, _ = points.shape
    if nk > MAX_KEYS:
        raise L.TcdiffError(f"plan: K = {nk} keys are more than TC_CHOREO_MAX_KEYS = {MAX_KEYS}")
    if tuple(keys.shape) not in ((nk,), (b, dn, nk)):
        raise L.TcdiffError(f"plan: keys must be ({nk},) or ({b}, {dn}, {nk}), got {_shape(keys)}")
    if isinstance(keys, torch.Tensor) and keys.dtype != torch.int32:
        raise L.TcdiffError(f"plan: keys must be int32, got {keys.dtype}")
    if counts is not None:
        if tuple(counts.shape) != (b, dn):
            raise L.TcdiffError(f"plan: counts must be ({b}, {dn}), got {_shape(counts)}")
        if isinstance(counts, torch.Tensor) and counts.dtype != torch.int32:
            raise L.TcdiffError(f"plan: counts must be int32, got {counts.dtype}")
    if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or frames < 1:
        raise L.TcdiffError(f"plan: frames must be an int >= 1, got {frames!r}")
    frames = int(frames)
    fps = _fps(fps, "plan")
    min_distance, max_speed = _limit(min_distance, "min_distance"), _limit(max_speed, "max_speed")
    scale, min_, columns = _columns(normalizer, columns)
    if math.prod((b, dn, frames)) > 2 ** 31 - 1:
        raise L.TcdiffError(f"plan: {b} x {dn} x {frames} frame slots are more than 2^31 - 1")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (b, frames * dn, 3) or out.dtype != torch.float32 or
                            not out.is_contiguous()):
        raise L.TcdiffError(f"plan: out must be a contiguous float32 ({b}, {frames * dn}, 3) tensor, got {_shape(out)} "
                            f"{getattr(out, 'dtype', '')}")
    tensors = [t for t in (points, keys, counts, out) if isinstance(t, torch.Tensor)]
    if any(not t.is_cuda for t in tensors) or (not tensors and not torch.cuda.is_available()):
        raise L.TcdiffError("plan runs on MI355X only (no CPU fallback): tensors must be on the device; lists and numpy arrays are copied up")
    dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    if any(t.device != dev for t in tensors):
        raise L.TcdiffError("plan: points, keys, counts and out must be on one device")
    up = lambda x: x.detach().contiguous() if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(dev)
    points, keys, counts = up(points), up(keys), None if counts is None else up(counts)
    if out is not None and _overlap(out, points):
        raise L.TcdiffError("plan: out overlaps the points it is computed from")
    n_pairs = dn * (dn - 1) // 2
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        traj = torch.empty(b, dn, frames, 2, dtype=torch.float32, device=dev)
        x_0 = torch.empty(b, frames * dn, 3, dtype=torch.float32, device=dev) if out is None else out
        p = Plan(traj, x_0, i32(b, dn), i32(b, dn), f64(b, dn), i32(b, dn), i32(b, dn), f64(b, dn), f64(b, n_pairs), i32(b, n_pairs),
                 i32(b, n_pairs), columns)
        pair_out = (p.dist_min, p.dist_min_frame, p.too_close) if n_pairs else (None, None, None)
        K.choreo_plan(points, keys, counts, frames, fps, scale, min_, min_distance, max_speed, traj, x_0, p.status, p.clamped, p.speed_max,
                      p.speed_peak, p.too_fast, p.path_length, *pair_out)
    return p


def trajectory_error(joints, traj, *, up=2) -> dict:
    """Did the dance follow the plan?  ``joints`` (b, dn, T, 24, 3) float32 on the device, in metres, read in place through its
    strides (only the trailing 24 x 3 must be contiguous: the permuted view of a frame-major buffer is read without a copy); the root
    is joint 0.  ``traj`` (b, dn, T, 2) float32: ``Plan.traj``, or any trajectory in metres.  In long mode b = 1.

    Returns device tensors per clip and dancer, a dict that ``metrics.summarize`` takes as it is: float64 (b, dn) ``traj_err_mean``,
    ``traj_err_max`` and ``traj_err_final`` (the last counted frame), the floor distance sqrt(dx dx + dy dy) over the two components
    that are not ``up`` between the root and the path, in metres; int32 ``traj_err_peak`` (the frame of the maximum; on a tie the
    lower) and ``traj_frames`` (the frames counted).  A frame with a non-finite input is counted out; a mean over nothing is NaN.
    One launch, nothing is copied to the host.  The definitions: include/tcdiff_choreo.h."""
    if not isinstance(joints, torch.Tensor) or joints.dim() != 5 or tuple(joints.shape[3:]) != (24, 3) or min(joints.shape) < 1:
        raise L.TcdiffError(f"trajectory_error: joints must be (b, dn, T, 24, 3), got {_shape(joints)}")
    if joints.dtype != torch.float32:
        raise L.TcdiffError(f"trajectory_error: joints must be float32, got {joints.dtype}")
    if joints.stride(-1) != 1 or joints.stride(-2) != 3:
        raise L.TcdiffError(f"trajectory_error: the trailing 2 dimension(s) of joints must be contiguous (strides {tuple(joints.stride())})")
    b, dn, T = joints.shape[:3]
    if not isinstance(traj, torch.Tensor) or tuple(traj.shape) != (b, dn, T, 2):
        raise L.TcdiffError(f"trajectory_error: traj must be ({b}, {dn}, {T}, 2), got {_shape(traj)}")
    if traj.dtype != torch.float32:
        raise L.TcdiffError(f"trajectory_error: traj must be float32, got {traj.dtype}")
    if isinstance(up, bool) or not isinstance(up, (int, np.integer)) or not 0 <= up <= 2:
        raise L.TcdiffError(f"trajectory_error: up must be 0, 1 or 2, got {up!r}")
    if math.prod((b, dn, T)) > 2 ** 31 - 1:
        raise L.TcdiffError(f"trajectory_error: {b} x {dn} x {T} frame slots are more than 2^31 - 1")
    if not joints.is_cuda or traj.device != joints.device:
        raise L.TcdiffError("trajectory_error runs on MI355X only (no CPU fallback): joints and traj must be on one device")
    dev = joints.device
    f64 = lambda: torch.empty(b, dn, dtype=torch.float64, device=dev)
    i32 = lambda: torch.empty(b, dn, dtype=torch.int32, device=dev)
    out = {"traj_err_mean": f64(), "traj_err_max": f64(), "traj_err_final": f64(), "traj_err_peak": i32(), "traj_frames": i32()}
    with torch.cuda.device(dev):
        K.trajectory_error(joints.detach(), traj.detach().contiguous(), int(up), *out.values())
    return out
