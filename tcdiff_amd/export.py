"""The pose export of ``GaussianDiffusion.render_sample`` (reference model/diffusion.py:811-988): the sampler's normalized
samples -> un-normalised SMPL axis-angle poses, root translations, FK joint positions and contacts, in ONE launch
(``tcdiff_pose_export``, csrc/export.hip), and the ``fk_out`` pickles the reference writes from them.

* ``export_poses`` runs the launch and shapes its outputs the way the reference builds its tensors.
* ``write_fk_out`` writes the reference's files: one ``{epoch}_{num}_{clip}.pkl`` per clip (model/diffusion.py:971-987) or one
  ``{epoch}_{song}.pkl`` per song in long mode (:930-939), each ``{"smpl_poses": (., 72), "smpl_trans": (., 3),
  "full_pose": (dn, frames, 24, 3)}`` of float32 numpy arrays.
The stick-figure drawing of ``skeleton_render`` is tcdiff_amd/draw.py, which draws these joints on the device.
"""
from __future__ import annotations

import os
import pickle
from pathlib import Path

import torch

from . import _lib as L
from . import kernels as K
from .fk import SMPL_OFFSETS, SMPL_PARENTS

_NFEAT = 151
_fade_cache: dict = {}


def _fade(half: int, device) -> torch.Tensor:
    """torch.linspace(0, 1, half) then torch.linspace(1, 0, half), float32, evaluated on the host as the reference evaluates
    them (model/diffusion.py:857-862,875), then copied to the device once per (half, device)."""
    key = (half, str(device))
    t = _fade_cache.get(key)
    if t is None:
        t = torch.cat([torch.linspace(0, 1, half), torch.linspace(1, 0, half)]).to(device)
        _fade_cache[key] = t
    return t


def _is_long(mode: str) -> bool:
    # the reference stitches in "long" mode only; "normal", "inpaint", "ctrl" (and any other mode) treat clips on their own
    return mode == "long"


def export_poses(samples: torch.Tensor, normalizer, mode: str, dn: int, *, parents=None, offsets=None):
    """samples (b, S * dn, 151) on the device, as the samplers return them (row = frame * dn + dancer); ``normalizer`` with a
    fitted ``scaler.scale_`` / ``scaler.min_`` of 151 columns (``io.Normalizer`` or the reference's class).

    mode != "long" -> (q (b, S dn, 24, 3), pos (b, S dn, 3), poses (b, dn, S, 24, 3), contacts (b, dn, S, 4)).
    mode == "long" (b half-overlapping windows of one song, T = S + (b - 1) S / 2) ->
                      (full_q (1, T dn, 24, 3), full_pos (1, T dn, 3), full_pose (1, dn, T, 24, 3), None).
    ``parents`` / ``offsets`` default to the SMPL skeleton of vis.py:48-101."""
    if samples.dim() != 3 or samples.shape[-1] != _NFEAT:
        raise L.TcdiffError(f"export_poses: samples must be (b, frames * dancers, {_NFEAT}), got {tuple(samples.shape)}")
    if not samples.is_cuda:
        raise L.TcdiffError("export_poses runs on MI355X only (no CPU fallback)")
    b, n, _ = samples.shape
    dn = int(dn)
    if dn < 1 or n % dn:
        raise L.TcdiffError(f"export_poses: {n} rows are not a whole number of frames of {dn} dancers")
    S = n // dn
    dev = samples.device
    x = samples.detach().float().contiguous()
    scale = normalizer.scaler.scale_.detach().to(dev, torch.float32).contiguous()
    min_ = normalizer.scaler.min_.detach().to(dev, torch.float32).contiguous()
    if scale.numel() != _NFEAT or min_.numel() != _NFEAT:
        raise L.TcdiffError(f"export_poses: the normalizer must be fitted on {_NFEAT} columns")
    parents = SMPL_PARENTS if parents is None else parents
    offsets = SMPL_OFFSETS if offsets is None else offsets
    long = _is_long(mode)
    P = (S + (S // 2) * (b - 1)) * dn if long else b * S * dn
    trans = torch.empty(P, 3, device=dev)
    poses = torch.empty(P, 24, 3, device=dev)
    joints = torch.empty(P, 24, 3, device=dev)
    contact = None if long else torch.empty(P, 4, device=dev)
    fade = _fade(S // 2, dev) if long and S % 2 == 0 else None
    K.pose_export(x, b, S, dn, L.EXPORT_LONG if long else L.EXPORT_NORMAL, scale, min_, fade, parents, offsets, trans,
                  poses, joints, contact)
    if long:
        T = P // dn
        return (poses.view(1, T * dn, 24, 3), trans.view(1, T * dn, 3),
                joints.view(1, T, dn, 24, 3).permute(0, 2, 1, 3, 4).contiguous(), None)
    return (poses.view(b, S * dn, 24, 3), trans.view(b, S * dn, 3),
            joints.view(b, S, dn, 24, 3).permute(0, 2, 1, 3, 4).contiguous(),
            contact.view(b, S, dn, 4).permute(0, 2, 1, 3).contiguous())


def fk_out_names(mode: str, epoch, name) -> list:
    """The file names ``render_sample`` writes under ``fk_out``: model/diffusion.py:930 (long) and :971-978 (every other
    mode; only the first min(b, len(name)) clips, as the reference's zip)."""
    if _is_long(mode):
        return [f'{epoch}_{"_".join(os.path.splitext(os.path.basename(name[0]))[0].split("_")[:-1])}.pkl']
    out = []
    for num, filename in enumerate(name):
        last = os.path.normpath(filename).split(os.sep)[-1].replace("npy", "wav")
        out.append(f"{epoch}_{num}_{last[:-4]}.pkl")
    return out


def write_fk_out(fk_out, mode: str, epoch, name, q, pos, poses) -> list:
    """Writes the reference's pickles from ``export_poses``' first three results (device or host tensors / arrays);
    returns the paths written."""
    as_np = lambda t: (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    Path(fk_out).mkdir(parents=True, exist_ok=True)
    names = fk_out_names(mode, epoch, name)
    written = []
    if _is_long(mode):
        q, pos, poses = as_np(q), as_np(pos), as_np(poses)
        path = os.path.join(fk_out, names[0])
        with open(path, "wb") as f:
            pickle.dump({"smpl_poses": q[0].reshape((-1, 72)), "smpl_trans": pos[0], "full_pose": poses[0]}, f)
        return [path]
    q, pos, poses = as_np(q), as_np(pos), as_np(poses)
    for outname, qq, pos_, pose in zip(names, q, pos, poses):
        path = f"{fk_out}/{outname}"
        with open(path, "wb") as f:
            pickle.dump({"smpl_poses": qq.reshape((-1, 72)), "smpl_trans": pos_, "full_pose": pose}, f)
        written.append(path)
    return written
