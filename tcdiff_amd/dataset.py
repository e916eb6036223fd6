"""The motion side of the reference's ``AIOZDataset`` (dataset/group_dataset.py:23-238) on MI355X: raw SMPL motion (root
positions and 24 axis-angle rotations per pose, Y-up) -> the normalised (dancers, frames, 151) features ``diffusion(x, cond)``
trains on, in two launches for any number of clips (``tcdiff_motion_ingest``, csrc/ingest.hip).  The inverse of
``export.export_poses``.

* ``process_motion`` is ``AIOZDataset.process_dataset`` (:167-238) for a batch of clips.
* ``AIOZDataset`` has the reference's constructor, attributes and items; its file logic (``load_aioz``, :99-165) runs on the
  host.
The reference goes through pytorch3d (absent here: arithmetic restated from its published definitions -- "parity unpinned").
The music features (``feats438``) are read from disk as the reference reads them; ``tcdiff_amd.music`` computes 425 of their 438
columns from a waveform on the GPU (the chroma and the beat track are the caller's), and ``assemble_cond`` lays the row out.
"""
from __future__ import annotations

import glob
import os
import pickle
from pathlib import Path
from typing import Any

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _lib as L
from . import io as tio
from . import kernels as K
from .fk import SMPL_OFFSETS, SMPL_PARENTS

_NFEAT = 151
STAT_NAMES = ("data_min_", "data_max_", "scale_", "min_")


def _device_f32(a, device) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _fitted_normalizer(data_min, data_max, scale, min_, n_rows: int) -> tio.Normalizer:
    """an ``io.Normalizer`` holding one clip's statistics, on the host like the reference's (dataset/scaler.py:58-70)"""
    n = tio.Normalizer.__new__(tio.Normalizer)
    s = tio.MinMaxScaler((-1, 1), clip=True)
    s.data_min_, s.data_max_, s.scale_, s.min_ = (t.detach().cpu().clone() for t in (data_min, data_max, scale, min_))
    s.data_range_ = s.data_max_ - s.data_min_
    s.n_samples_seen_ = n_rows
    n.scaler = s
    return n


def process_motion(pos, q, *, train: bool, normalizer=None, data_len: int = -1, return_raw: bool = False,
                   parents=None, offsets=None):
    """pos (clips, dn, sq, 3) root positions and q (clips, dn, sq, 72) axis-angle rotations (numpy arrays or tensors, on the
    host or the device; never modified) -> ``(features, normalizer, stats)`` and, with ``return_raw``, the un-normalised
    features as a fourth result.

    features: (clips, dn, sq, 151) float32 on the device, [contacts 4 | root 3 | 6-D 24 x 6], normalised to [-1, 1].
    train=True:  a Normalizer is fitted on every clip on its own, as the reference's loop does (group_dataset.py:217-218);
                 the returned ``io.Normalizer`` is the LAST clip's, and stats holds every clip's ``data_min_``,
                 ``data_max_``, ``scale_`` and ``min_`` as (clips, 151) device tensors.
    train=False: ``normalizer`` (an ``io.Normalizer`` or the reference's class, fitted on 151 columns) is used for every clip
                 and returned; None raises, as the reference asserts (:220).  stats holds its ``scale_`` / ``min_`` (1, 151).
    data_len > 0 keeps the first ``data_len`` dancers of every clip (the reference slices that axis, :227-228)."""
    if not train and normalizer is None:
        raise AssertionError("process_motion(train=False) needs a fitted normalizer")
    on_dev = [t.device for t in (pos, q) if isinstance(t, torch.Tensor) and t.is_cuda]
    if not on_dev and not torch.cuda.is_available():
        raise L.TcdiffError("process_motion runs on MI355X only (no CPU fallback)")
    L.load()
    dev = on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device())
    pos_d, q_d = _device_f32(pos, dev), _device_f32(q, dev)
    if pos_d.dim() != 4 or q_d.dim() != 4 or pos_d.shape[-1] != 3 or q_d.shape[-1] != 72 or pos_d.shape[:3] != q_d.shape[:3]:
        raise L.TcdiffError(f"process_motion: pos must be (clips, dn, sq, 3) and q (clips, dn, sq, 72), got "
                            f"{tuple(pos_d.shape)} and {tuple(q_d.shape)}")
    clips, dn, sq, _ = pos_d.shape
    if clips < 1 or dn < 1 or sq < 1:
        raise L.TcdiffError(f"process_motion: empty input {tuple(pos_d.shape)}")
    scale = min_ = stats = None
    if train:
        stats = torch.empty(clips, 4, _NFEAT, device=dev)
    else:
        scale = normalizer.scaler.scale_.detach().to(dev, torch.float32).contiguous()
        min_ = normalizer.scaler.min_.detach().to(dev, torch.float32).contiguous()
        if scale.numel() != _NFEAT or min_.numel() != _NFEAT:
            raise L.TcdiffError(f"process_motion: the normalizer must be fitted on {_NFEAT} columns")
    with torch.cuda.device(dev):
        feats = torch.empty(clips, dn, sq, _NFEAT, device=dev)
        raw = torch.empty_like(feats) if return_raw else None
        feet = torch.empty(clips * dn * sq, 12, device=dev)
        K.motion_ingest(pos_d, q_d, clips, dn, sq, SMPL_PARENTS if parents is None else parents,
                        SMPL_OFFSETS if offsets is None else offsets, train, scale, min_, feats, raw, feet, stats)
    if train:
        st = {name: stats[:, k] for k, name in enumerate(STAT_NAMES)}
        normalizer = _fitted_normalizer(*(st[name][-1] for name in STAT_NAMES), dn * sq)
    else:
        st = {"scale_": scale.view(1, _NFEAT), "min_": min_.view(1, _NFEAT)}
    if data_len > 0:
        feats = feats[:, :data_len]
        raw = raw[:, :data_len] if raw is not None else None
    return (feats, normalizer, st, raw) if return_raw else (feats, normalizer, st)


class AIOZDataset(Dataset):
    """The reference's ``dataset.group_dataset.AIOZDataset`` (:23-238): same constructor arguments, ``.normalizer``,
    ``.data`` ({"pose": host numpy (clips, dn, sq, 151), "filenames", "wavs"}), ``.length`` and items
    ``(pose, feature, filename, wav)``; the motion features come from ``process_motion``."""

    def __init__(self, data_path: str, backup_path: str, train: bool, feature_type: str = "438feat", normalizer: Any = None,
                 data_len: int = -1, required_dancer_num=3, include_contacts: bool = True, force_reload: bool = False,
                 split_file=None):
        self.data_path = data_path
        self.raw_fps = 30
        self.data_fps = 30
        assert self.data_fps <= self.raw_fps
        self.data_stride = self.raw_fps // self.data_fps
        self.train = train
        self.name = "Train" if self.train else "Test"
        self.feature_type = feature_type
        self.normalizer = normalizer
        self.data_len = data_len
        self.required_dancer_num = required_dancer_num
        self.split_file = split_file

        backup_path = Path(backup_path)
        backup_path.mkdir(parents=True, exist_ok=True)
        if not train:
            # under the reference's class paths, so that its plain pickle.load reads the file (group_dataset.py:59-62)
            with open(os.path.join(backup_path, "normalizer.pkl"), "wb") as f:
                tio._RefPickle.dump(normalizer, f)
        # the reference's cache branch (:65-68) loads nothing and then fails on `data`; the raw data is always loaded here
        data = self.load_aioz(required_dancer_num)
        pose_input = self.process_dataset(data["pos"], data["q"])
        self.data = {"pose": pose_input, "filenames": data["filenames"], "wavs": data["wavs"]}
        assert len(pose_input) == len(data["filenames"])
        self.length = len(pose_input)

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        filename_ = self.data["filenames"][idx]
        feature = torch.from_numpy(np.load(filename_))
        return self.data["pose"][idx], feature, filename_, self.data["wavs"][idx]

    def load_aioz(self, required_dancer_num=3):
        """group_dataset.py:99-165: ``<data_path>/<train|test>/motions_sliced/*.pkl`` sorted; a clip is kept when its name
        without the slice suffix is in ``split_file``, ``feats438/<name>.npy`` exists and it has ``required_dancer_num``
        dancers."""
        split_data_path = os.path.join(self.data_path, "train" if self.train else "test")
        motion_path = os.path.join(split_data_path, "motions_sliced")
        sound_path = os.path.join(split_data_path, "feats438")
        wav_path = os.path.join(split_data_path, "wavs_sliced")
        all_pos, all_q, all_names, all_wavs = [], [], [], []
        for motion_p in sorted(glob.glob(os.path.join(motion_path, "*.pkl"))):
            file_name = os.path.splitext(os.path.basename(motion_p))[0]
            file_name_origin = "_".join(file_name.split("_")[:-1])
            if file_name_origin not in self.split_file:
                continue
            if not os.path.exists(os.path.join(sound_path, file_name + ".npy")):
                continue
            with open(motion_p, "rb") as f:
                data = pickle.load(f)
            pos, q = data["pos"], data["q"]
            if pos.shape[0] == required_dancer_num:
                all_pos.append(pos)
                all_q.append(q)
                all_names.append(os.path.join(sound_path, file_name + ".npy"))
                all_wavs.append(os.path.join(wav_path, file_name + ".wav"))
        return {"pos": np.array(all_pos), "q": np.array(all_q), "filenames": all_names, "wavs": all_wavs}

    def process_dataset(self, root_pos_all, local_q_all):
        """group_dataset.py:167-238 -> host numpy (clips, dn, sq, 151) float32; in train mode ``self.normalizer`` ends as the
        last clip's."""
        if len(root_pos_all) == 0:
            return np.array([])
        feats, self.normalizer, _ = process_motion(root_pos_all, local_q_all, train=self.train, normalizer=self.normalizer,
                                                   data_len=self.data_len)
        return feats.cpu().numpy()
