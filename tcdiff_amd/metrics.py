"""Are the generated dances any good?  Sample-level physical metrics of the joint positions ``export_poses`` leaves on the
device, in two launches (``tcdiff_motion_metrics``, csrc/metrics.hip), float64 throughout:

* ``pfc``: EDGE's physical foot contact score (do the feet slide while the body does not accelerate?),
* ``contact_slide`` / ``contact_break`` / ``contact_frames``: the model's own contact channels against the 0.01 m displacement
  the dataset labels them from (reference dataset/group_dataset.py:204-207, model/diffusion.py:719-733),
* ``collision_rate``: do the dancers walk through each other?
* ``beat_align`` / ``motion_beats``: Bailando's beat alignment against the ``onset_beat`` column of the 438-d music features.

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)        # what evaluate_samples does
    result = motion_metrics(poses, contacts, beats_from_cond(cond, poses.shape[2]))
    print(summarize(result))
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import kernels as K
from .export import _is_long, export_poses

ONSET_BEAT = 53          # 20 mfcc + 20 mfcc delta + 12 chroma + onset_env, then onset_beat (data/data_preprocess/dataset_utils.py:75-82)


def _check_view(name, t, shape, inner):
    if not isinstance(t, torch.Tensor) or t.dim() != len(shape) or any(w is not None and s != w for s, w in zip(t.shape, shape)):
        want = ", ".join("*" if w is None else str(w) for w in shape)
        raise L.TcdiffError(f"motion_metrics: {name} must be ({want}), got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if t.dtype != torch.float32:
        raise L.TcdiffError(f"motion_metrics: {name} must be float32, got {t.dtype}")
    want = 1
    for k in range(1, inner + 1):                  # the trailing dimensions are read as one contiguous run
        if t.shape[-k] != 1 and t.stride(-k) != want:
            raise L.TcdiffError(f"motion_metrics: the trailing {inner} dimension(s) of {name} must be contiguous "
                                f"(strides {tuple(t.stride())})")
        want *= t.shape[-k]
    if not t.is_cuda:
        raise L.TcdiffError("motion_metrics runs on MI355X only (no CPU fallback)")


def motion_metrics(joints, contacts=None, beats=None, *, fps=30, up=2, contact_threshold=0.95, still=0.01, radius=0.3,
                   sigma_smooth=5.0, sigma_beat=3.0) -> dict:
    """joints (b, dn, T, 24, 3) float32 on the device, in metres, read in place through its strides (only the trailing 24 x 3
    must be contiguous: the permuted view of a frame-major buffer is read without a copy); contacts (optional)
    (b, dn, T, 4) float32, feet 7, 8, 10, 11; beats (optional) (b, T) uint8, non-zero = a music beat on that motion frame.

    Returns float64 device tensors ``pfc`` (b, dn) (unscaled; ``summarize`` applies EDGE's 1e4) and ``collision_rate`` (b,);
    with contacts ``contact_slide``, ``contact_break`` (b, dn) and ``contact_frames`` (int64); with beats ``beat_align``
    (b, dn) and ``motion_beats`` (int64).  The definitions: include/tcdiff_hip.h.  ``radius`` is a choice, not a measured value."""
    _check_view("joints", joints, (None, None, None, 24, 3), 2)
    b, dn, T = joints.shape[:3]
    if min(b, dn, T) < 1:
        raise L.TcdiffError(f"motion_metrics: joints {tuple(joints.shape)} has an empty dimension")
    dev = joints.device
    if contacts is not None:
        _check_view("contacts", contacts, (b, dn, T, 4), 1)
    if beats is not None:
        if not isinstance(beats, torch.Tensor) or tuple(beats.shape) != (b, T):
            raise L.TcdiffError(f"motion_metrics: beats must be ({b}, {T}), got {tuple(getattr(beats, 'shape', ()))}")
        if beats.dtype != torch.uint8:
            raise L.TcdiffError(f"motion_metrics: beats must be uint8, got {beats.dtype}")
        if not beats.is_cuda:
            raise L.TcdiffError("motion_metrics runs on MI355X only (no CPU fallback)")
        beats = beats.contiguous()
    for t in (contacts, beats):
        if t is not None and t.device != dev:
            raise L.TcdiffError("motion_metrics: joints, contacts and beats must be on one device")
    if up not in (0, 1, 2):
        raise L.TcdiffError(f"motion_metrics: up must be 0, 1 or 2, got {up!r}")
    fps, sigma_smooth, sigma_beat = float(fps), float(sigma_smooth), float(sigma_beat)
    if not (fps > 0 and sigma_smooth > 0 and sigma_beat > 0):
        raise L.TcdiffError("motion_metrics: fps, sigma_smooth and sigma_beat must be positive")
    if 4.0 * sigma_smooth + 0.5 > L.METRICS_MAX_RADIUS:
        raise L.TcdiffError(f"motion_metrics: sigma_smooth {sigma_smooth} needs a filter radius above {L.METRICS_MAX_RADIUS}")
    n = b * dn * T
    ws = torch.empty(L.METRICS_WS_PLANES * n, dtype=torch.float64, device=dev)
    iws = torch.empty(L.METRICS_IWS_PLANES * n, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)
    out = {"pfc": f64(b, dn)}
    if contacts is not None:
        out.update(contact_slide=f64(b, dn), contact_break=f64(b, dn), contact_frames=i64(b, dn))
    out["collision_rate"] = f64(b)
    if beats is not None:
        out.update(beat_align=f64(b, dn), motion_beats=i64(b, dn))
    with torch.cuda.device(dev):
        K.motion_metrics(joints, contacts, beats, int(up), fps, float(contact_threshold), float(still), float(radius), sigma_smooth,
                         sigma_beat, ws, iws, out["pfc"], out.get("contact_slide"), out.get("contact_break"),
                         out.get("contact_frames"), out["collision_rate"], out.get("beat_align"), out.get("motion_beats"))
    return out


def beats_from_cond(cond: torch.Tensor, frames: int, *, long: bool = False) -> torch.Tensor:
    """The music's beats on the motion's frames, (b, frames) uint8, from the 438-d music features cond (b, n, 438): music runs
    at two frames per motion frame, ``beats[t] = cond[:, 2t, 53] > 0.5 or cond[:, 2t + 1, 53] > 0.5``.

    long=True: the b windows are half-overlapping windows of one song of ``frames`` = S + (b - 1) S / 2 motion frames; song frame
    t is read from window k = min(t // h, b - 1) at its local frame t - k h, h = S // 2; the result is (1, frames)."""
    if cond.dim() != 3 or cond.shape[-1] <= ONSET_BEAT:
        raise L.TcdiffError(f"beats_from_cond: cond must be (b, music frames, 438), got {tuple(cond.shape)}")
    b, n, _ = cond.shape
    frames = int(frames)
    on = cond[..., ONSET_BEAT] > 0.5
    if not long:
        if frames < 1 or 2 * frames > n:
            raise L.TcdiffError(f"beats_from_cond: {frames} motion frames need {2 * frames} music frames, cond has {n}")
        return on[:, :2 * frames].reshape(b, frames, 2).any(-1).to(torch.uint8)
    if frames < 1 or (2 * frames) % (b + 1) or (2 * frames // (b + 1)) % 2:
        raise L.TcdiffError(f"beats_from_cond: {frames} frames are not {b} half-overlapping windows of an even length")
    S = 2 * frames // (b + 1)
    h = S // 2
    if 2 * S > n:
        raise L.TcdiffError(f"beats_from_cond: windows of {S} motion frames need {2 * S} music frames, cond has {n}")
    t = torch.arange(frames, device=cond.device)
    k = torch.clamp(t // h, max=b - 1)
    loc = t - k * h
    return (on[k, 2 * loc] | on[k, 2 * loc + 1]).to(torch.uint8).reshape(1, frames)


def evaluate_samples(samples, normalizer, cond, dn, mode="normal", **kw) -> dict:
    """The sampler's normalised samples (b, S * dn, 151) and their music features -> ``motion_metrics`` of the exported poses:
    ``export_poses``, ``beats_from_cond``, ``motion_metrics``, everything on the device.  In "long" mode the b windows are one
    song and the export drops the contact channels, so the contact keys are absent.  ``export_poses`` returns contiguous
    device-side copies of its frame-major buffers, and those copies are what is scored here; ``motion_metrics`` reading a permuted
    view in place is for callers that hold such a buffer themselves."""
    _, _, poses, contacts = export_poses(samples, normalizer, mode, dn)
    beats = beats_from_cond(cond.to(poses.device), poses.shape[2], long=_is_long(mode))
    return motion_metrics(poses, contacts, beats, **kw)


def summarize(result: dict) -> dict:
    """One float per metric: the mean over clips and dancers that ignores NaN (NaN if nothing is left), PFC in EDGE's unit
    (x 1e4).  This is where the numbers come to the host."""
    out = {}
    for k, v in result.items():
        m = float(torch.nanmean(v.to(torch.float64))) if v.numel() else float("nan")
        out[k] = m * 1e4 if k == "pfc" else m
    return out
