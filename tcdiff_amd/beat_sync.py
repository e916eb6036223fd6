"""Is the dance ON the music, and a time warp that brings it there.  ``beat_align`` of ``motion_metrics`` (Bailando's beat alignment, the
number every dance paper leads with) says in one float per dancer how far the kinematic beats -- the minima of the smoothed joint
speed -- lie from the music's; nothing returned where they are, and nothing acted on them: a dance whose accents land three frames
after the drum played that way in every pickle, .glb, frame and AVI with sound.  Two functions, on the device, float64 throughout
(include/tcdiff_beatsync.h is the definition, csrc/beatsync.hip runs it):

* ``motion_beats(joints)``: the smoothed speed curve, the kinematic beats as a per-frame flag and their count, per dancer or, with
  ``share``, pooled over a clip's dancers, in two launches.
* ``beat_sync(q, pos, beats, dn=...)``: a monotone time warp of what ``export_poses`` returns, in three launches for any number of
  clips: every music beat is matched to its nearest kinematic beat within ``max_shift`` frames, the matches that keep the local
  playback rate within [1 / max_rate, max_rate] become the anchors of a PCHIP warp (the interpolant of ``plan``, so ascending anchors
  give a monotone warp), and the poses are resampled along it: the root linearly, the rotations by slerp, the contacts from the
  nearer frame; then the joints of the retimed poses by the export's FK.

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)
    beats = beats_from_cond(cond, poses.shape[2], long=False)
    s = beat_sync(q, pos, beats, dn=dn, contacts=contacts)          # s.q, s.pos, s.joints, s.contacts; s.before / s.after["beat_align"]

It belongs right after the export and before ``smooth``, ``keep_apart``, ``ground`` and ``foot_lock``: those then act on the retimed
motion, and the filter takes out the kinks of the resampling.  ``max_shift=7`` (under half a beat at 120 bpm and 30 fps),
``max_rate=1.5``, ``strength=1``, ``sigma_smooth=5`` (``motion_metrics``' default), the linear root interpolation and the
nearest-frame contacts are choices, not measurements.  The reference has no counterpart (it renders the raw poses): the speed curve is
``beat_align``'s own, the rest is the project's own and parity with any other tool is unpinned.  Not promised: that the speed minimum
of the warped motion lands exactly on its beat (the warp's own rate modulates the speed); that ``trajectory_error`` stays (a warp
shifts the root path in time, by up to ``max_shift`` frames of travel); with ``share=False``, that the contacts between dancers stay
(``keep_apart`` runs later).  Not built: snapping choreography keys to beats, retiming inside the sampler, changing the clip length,
cubic root interpolation, a musical-phrase or downbeat model, warping ``cond``.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .fk import SMPL_OFFSETS, SMPL_PARENTS

MAX_FRAMES = L.BEATSYNC.constants["TC_BEATSYNC_MAX_FRAMES"]
MAX_RADIUS = L.BEATSYNC.constants["TC_BEATSYNC_MAX_RADIUS"]
_TABLES = {}          # (sigma, device) -> the weights on that device


class BeatSync(NamedTuple):
    q: torch.Tensor                  # (b, T dn, 24, 3) float32: the retimed rotation vectors
    pos: torch.Tensor                # (b, T dn, 3) float32: the retimed root positions
    joints: torch.Tensor             # (b, dn, T, 24, 3) float32: fk_forward of q and pos, in place of export_poses' third result
    contacts: torch.Tensor | None    # (b, dn, T, 4) float32: the contacts of the nearer source frame, or None
    warp: torch.Tensor               # (b, W, T) float64: the source time of every output frame
    status: torch.Tensor             # (b, W) int32: 1: a non-finite speed, the warp is the identity
    kin_count: torch.Tensor          # (b, W) int32: the kinematic beats
    music_count: torch.Tensor        # (b, W) int32: the music beats (the end frames are pinned and do not count)
    matched: torch.Tensor            # (b, W) int32: the music beats that keep a kinematic beat within max_shift
    dropped: torch.Tensor            # (b, W) int32: of those, the ones the rate bound refused
    anchors: torch.Tensor            # (b, W) int32: of those, the ones the warp passes through
    shift_max: torch.Tensor          # (b, W) float64: the largest |warp[t] - t|, in frames
    rate_min: torch.Tensor           # (b, W) float64: the smallest warp[t + 1] - warp[t]
    rate_min_frame: torch.Tensor     # (b, W) int32
    rate_max: torch.Tensor           # (b, W) float64: the largest
    rate_max_frame: torch.Tensor     # (b, W) int32
    moved: torch.Tensor              # (b, dn) int32: the frames whose source time is not their own
    copied: torch.Tensor             # (b, dn) int32: the outputs copied through for want of finite source frames
    speed: torch.Tensor              # (b, W, T - 1) float64: the smoothed speed curve of the input
    kin: torch.Tensor                # (b, W, T) uint8: 1 marks a kinematic beat of the input
    before: dict | None = None       # motion_metrics(joints of the input, beats=beats) (measure=True)
    after: dict | None = None        # motion_metrics(joints, beats=beats)


def gaussian_table(sigma) -> np.ndarray:
    """The 2 rad + 1 normalised float64 weights of ``scipy.ndimage.gaussian_filter1d(..., sigma)``, rad = int(4 sigma + 0.5), built on
    the host as scipy builds them: the kernel and the restatement multiply the same doubles in the same order."""
    sigma = _sigma(sigma, "gaussian_table")
    rad = int(4.0 * sigma + 0.5)
    x = np.arange(-rad, rad + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def _sigma(sigma, who):
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not sigma > 0 or not math.isfinite(sigma):
        raise L.TcdiffError(f"{who}: sigma_smooth must be a positive number, got {sigma!r}")
    if 4.0 * float(sigma) + 0.5 > MAX_RADIUS:
        raise L.TcdiffError(f"{who}: sigma_smooth {sigma} needs a filter radius above TC_BEATSYNC_MAX_RADIUS = {MAX_RADIUS}")
    return float(sigma)


def _table_on(sigma, dev):
    key = (sigma, str(dev))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(gaussian_table(sigma)).to(dev)
    return _TABLES[key]


def _fps(fps, who):
    if isinstance(fps, bool) or not isinstance(fps, (int, float)) or not 0 < fps <= 1e6:
        raise L.TcdiffError(f"{who}: fps must be a number in (0, 1e6], got {fps!r}")
    return float(fps)


def _frames(T, who):
    if T > MAX_FRAMES:
        raise L.TcdiffError(f"{who}: {T} frames are more than TC_BEATSYNC_MAX_FRAMES = {MAX_FRAMES}")


def motion_beats(joints, *, fps=30, sigma_smooth=5.0, share=False) -> dict:
    """joints (b, dn, T, 24, 3) float32 on the device, in metres, read in place through its strides (only the trailing 24 x 3 must be
    contiguous), as ``motion_metrics`` reads it.

    Returns device tensors, with W = 1 if ``share`` (the clip's dancers pooled) else dn: ``speed`` (b, W, T - 1) float64, the mean
    joint speed per frame smoothed exactly as ``beat_align`` smooths it; ``kin`` (b, W, T) uint8, 1 on its strict interior local
    minima, the kinematic beats; ``kin_count`` (b, W) int32 -- with ``share=False`` the ``motion_beats`` of ``motion_metrics``.  A
    curve with a non-finite speed has no beats and a ``speed`` of NaN.  ``fps`` is checked and otherwise unused: the curve is per
    frame, as Bailando's.  Two launches, nothing is copied to the host.  The definitions: include/tcdiff_beatsync.h."""
    if not isinstance(joints, torch.Tensor) or joints.dim() != 5 or tuple(joints.shape[3:]) != (24, 3):
        raise L.TcdiffError(f"motion_beats: joints must be (b, dn, T, 24, 3), got "
                            f"{tuple(joints.shape) if isinstance(joints, torch.Tensor) else type(joints)}")
    if joints.dtype != torch.float32:
        raise L.TcdiffError(f"motion_beats: joints must be float32, got {joints.dtype}")
    if min(joints.shape[:3]) < 1:
        raise L.TcdiffError(f"motion_beats: joints {tuple(joints.shape)} has an empty dimension")
    if joints.stride(-1) != 1 or joints.stride(-2) != 3:
        raise L.TcdiffError(f"motion_beats: the trailing 2 dimension(s) of joints must be contiguous (strides {tuple(joints.stride())})")
    _fps(fps, "motion_beats")
    sigma = _sigma(sigma_smooth, "motion_beats")
    if not isinstance(share, bool):
        raise L.TcdiffError(f"motion_beats: share must be a bool, got {share!r}")
    b, dn, T = joints.shape[:3]
    _frames(T, "motion_beats")
    if not joints.is_cuda:
        raise L.TcdiffError("motion_beats runs on MI355X only (no CPU fallback)")
    dev, W = joints.device, 1 if share else dn
    with torch.cuda.device(dev):
        weights = _table_on(sigma, dev)
        workspace = torch.empty(K.beat_sync_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        out = {"speed": torch.empty(b, W, T - 1, dtype=torch.float64, device=dev), "kin": torch.empty(b, W, T, dtype=torch.uint8, device=dev),
               "kin_count": torch.empty(b, W, dtype=torch.int32, device=dev)}
        K.motion_beats(joints.detach(), share, (weights.numel() - 1) // 2, weights, workspace, *out.values())
    return out


def beat_sync(q, pos, beats, *, dn, contacts=None, share=True, max_shift=7, max_rate=1.5, strength=1.0, sigma_smooth=5.0, fps=30,
              parents=None, offsets=None, measure=True) -> BeatSync:
    """``q`` (b, T dn, 24, 3) float32 rotation vectors and ``pos`` (b, T dn, 3) on the device, row = frame dn + dancer:
    ``export_poses``' first two results, in long mode too (b = 1).  ``beats`` (b, T) uint8 as ``beats_from_cond`` returns it;
    ``contacts`` (b, dn, T, 4) float32 or None.

    With ``share`` the dancers of a clip are retimed together by the beats of their pooled speed (W = 1 warp per clip), without it
    each by its own (W = dn).  A music beat is matched to its nearest kinematic beat at most ``max_shift`` frames away; a match is
    kept while the warp's rate between neighbouring anchors stays within [1 / max_rate, max_rate]; ``strength`` in [0, 1] is the
    share of the distance that is closed.  7, 1.5, 1 and ``sigma_smooth=5`` are choices, not measurements, and so are the linear
    root interpolation and the nearest-frame contacts.

    Returns ``BeatSync``: the retimed ``q``, ``pos``, ``joints`` (b, dn, T, 24, 3) and ``contacts``; ``warp`` (b, W, T), the source
    time of every output frame, nondecreasing from 0 to T - 1; what became of the beats per warp (``status``, ``kin_count``,
    ``music_count``, ``matched``, ``dropped``, ``anchors``, ``shift_max``, ``rate_min`` / ``rate_max`` with their frames); per clip
    and dancer ``moved`` and ``copied``; ``speed`` and ``kin`` of the input as ``motion_beats`` returns them.  With ``measure`` also
    ``before`` and ``after``: ``motion_metrics(joints, beats=beats)`` of the input's joints and of the output's, by the existing
    kernel on both sides.  A warp whose speed curve holds a non-finite value is the identity (``status`` 1) and its dancers' outputs
    are the input's words; an output whose two source frames hold a non-finite float is input frame t's word (``copied``).  Three
    launches, plus the two metric calls; the inputs are never changed, nothing synchronises, nothing is copied to the host.
    ``parents`` / ``offsets`` default to the SMPL skeleton.  The definitions: include/tcdiff_beatsync.h."""
    if not isinstance(q, torch.Tensor) or not isinstance(pos, torch.Tensor) or not isinstance(beats, torch.Tensor):
        raise L.TcdiffError("beat_sync: q, pos and beats must be tensors")
    if q.dim() != 4 or tuple(q.shape[2:]) != (24, 3) or q.dtype != torch.float32:
        raise L.TcdiffError(f"beat_sync: q must be (b, frames * dancers, 24, 3) float32, got {tuple(q.shape)} {q.dtype}")
    b, n = q.shape[:2]
    if tuple(pos.shape) != (b, n, 3) or pos.dtype != torch.float32:
        raise L.TcdiffError(f"beat_sync: pos must be ({b}, {n}, 3) float32, got {tuple(pos.shape)} {pos.dtype}")
    if isinstance(dn, bool) or not isinstance(dn, int) or dn < 1 or b < 1 or n < 1 or n % dn:
        raise L.TcdiffError(f"beat_sync: {n} rows are not a whole number of frames of {dn!r} dancers")
    T = n // dn
    if tuple(beats.shape) != (b, T) or beats.dtype != torch.uint8:
        raise L.TcdiffError(f"beat_sync: beats must be ({b}, {T}) uint8, got {tuple(beats.shape)} {beats.dtype}")
    if contacts is not None and (not isinstance(contacts, torch.Tensor) or tuple(contacts.shape) != (b, dn, T, 4) or contacts.dtype != torch.float32):
        raise L.TcdiffError(f"beat_sync: contacts must be ({b}, {dn}, {T}, 4) float32 or None, got "
                            f"{tuple(contacts.shape) if isinstance(contacts, torch.Tensor) else type(contacts)}")
    if not isinstance(share, bool):
        raise L.TcdiffError(f"beat_sync: share must be a bool, got {share!r}")
    if isinstance(max_shift, bool) or not isinstance(max_shift, (int, np.integer)) or not 0 <= max_shift <= MAX_FRAMES:
        raise L.TcdiffError(f"beat_sync: max_shift must be an int in [0, {MAX_FRAMES}], got {max_shift!r}")
    if isinstance(max_rate, bool) or not isinstance(max_rate, (int, float)) or not 1 <= max_rate <= 1e6:
        raise L.TcdiffError(f"beat_sync: max_rate must be a number in [1, 1e6], got {max_rate!r}")
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0 <= strength <= 1:
        raise L.TcdiffError(f"beat_sync: strength must be a number in [0, 1], got {strength!r}")
    sigma = _sigma(sigma_smooth, "beat_sync")
    fps = _fps(fps, "beat_sync")
    if not isinstance(measure, bool):
        raise L.TcdiffError(f"beat_sync: measure must be a bool, got {measure!r}")
    parents = SMPL_PARENTS if parents is None else parents
    offsets = SMPL_OFFSETS if offsets is None else offsets
    if len(parents) != 24 or len(offsets) != 24:
        raise L.TcdiffError("beat_sync: the skeleton has 24 joints")
    if any(int(parents[j]) >= j for j in range(24)):
        raise L.TcdiffError(f"beat_sync: every parent must precede its child, got parents {list(parents)!r}")
    _frames(T, "beat_sync")
    if math.prod((b, dn, T)) > 2 ** 31 - 1:
        raise L.TcdiffError(f"beat_sync: {b} x {dn} x {T} frame slots are more than 2^31 - 1")
    if not q.is_cuda or pos.device != q.device or beats.device != q.device or (contacts is not None and contacts.device != q.device):
        raise L.TcdiffError("beat_sync runs on MI355X only (no CPU fallback): q, pos, beats and contacts must be on one device")
    dev, W = q.device, 1 if share else dn
    q, pos, beats = q.detach().contiguous(), pos.detach().contiguous(), beats.contiguous()
    contacts = None if contacts is None else contacts.detach().contiguous()
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        weights = _table_on(sigma, dev)
        workspace = torch.empty(K.beat_sync_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        q_out, pos_out = torch.empty_like(q), torch.empty_like(pos)
        contacts_out = None if contacts is None else torch.empty_like(contacts)
        joints = torch.empty(b, dn, T, 24, 3, device=dev)
        joints_in = torch.empty(b, dn, T, 24, 3, device=dev) if measure else None
        warp, speed, kin = f64(b, W, T), f64(b, W, T - 1), torch.empty(b, W, T, dtype=torch.uint8, device=dev)
        status, kin_count, music_count, matched, dropped, anchors = (i32(b, W) for _ in range(6))
        shift_max, rate_min, rate_max, rate_min_frame, rate_max_frame = f64(b, W), f64(b, W), f64(b, W), i32(b, W), i32(b, W)
        moved, copied = i32(b, dn), i32(b, dn)
        K.beat_sync(q, pos, contacts, beats, b, dn, T, share, int(max_shift), float(max_rate), float(strength), (weights.numel() - 1) // 2,
                    weights, parents, offsets, workspace, q_out, pos_out, contacts_out, joints, joints_in, warp, speed, kin, status, kin_count,
                    music_count, matched, dropped, anchors, shift_max, rate_min, rate_max, rate_min_frame, rate_max_frame, moved, copied)
    before = after = None
    if measure:
        from .metrics import motion_metrics
        before = motion_metrics(joints_in, beats=beats, fps=fps, sigma_smooth=sigma)
        after = motion_metrics(joints, beats=beats, fps=fps, sigma_smooth=sigma)
    return BeatSync(q_out, pos_out, joints, contacts_out, warp, status, kin_count, music_count, matched, dropped, anchors, shift_max, rate_min,
                    rate_min_frame, rate_max, rate_max_frame, moved, copied, speed, kin, before, after)
