"""render_export.npz: what the REAL reference's GaussianDiffusion.render_sample (model/diffusion.py:765-988) writes under
``fk_out`` and hands to ``skeleton_render``, for a tensor ``shape`` (the samples themselves: no sampling runs).

  normal: 2 clips x 2 dancers x 150 frames, names "data/test/features/<clip>.npy"   -> two {epoch}_{num}_{clip}.pkl
  long:   3 half-overlapping windows x 2 dancers of one song (T = 300 frames)      -> one {epoch}_{song}.pkl
The normalizer is a reference dataset.preprocess.Normalizer fitted on synthetic motion (contacts, a root walk, the 6-D of
random rotations).  The long windows overlap as the long sampler leaves them: each window's first half is the previous
window's second half, perturbed per frame from not at all (slerp's linear branch) to strongly (negative dots).  The sample
values are multiples of 2^-10, stored as int16.

pytorch3d is absent: its six functions are bound to the oracle's restatements in model.diffusion, dataset.quaternion and vis.
skeleton_render is a recorder, p_map a plain map, and the skeleton is the reference's vis.SMPLSkeleton.
Stored (data only): the int16 inputs, the scaler's scale_ / min_, every pickle's file name and arrays, and the recorder's
contacts and arguments.  Build container only (needs the reference checkout)."""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import refload  # noqa: E402
from oracle import tcdiff_oracle as O  # noqa: E402

_, GaussianDiffusion = refload.load()
import dataset.quaternion as RQ  # noqa: E402
import model.diffusion as RD  # noqa: E402
import vis as RV  # noqa: E402
from dataset.preprocess import Normalizer  # noqa: E402

for mod in (RD, RQ, RV):
    for fn in ("rotation_6d_to_matrix", "matrix_to_axis_angle", "axis_angle_to_quaternion", "quaternion_to_axis_angle",
               "quaternion_apply", "quaternion_multiply"):
        if hasattr(mod, fn):
            setattr(mod, fn, getattr(O, fn))

calls = []


def recorder(poses, **kw):
    calls.append((np.array(poses), kw))


RD.skeleton_render = recorder
RD.p_map = lambda f, it: list(map(f, it))

SCALE = 2.0 ** -10
g = torch.Generator().manual_seed(2024)


def random_6d(n):
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    r0 = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1)
    r1 = torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1)
    return torch.cat([r0, r1], -1).float()


# synthetic motion (8 sequences x 150 frames) the normalizer is fitted on
n_fit = 8 * 150
motion = torch.empty(n_fit, 151)
motion[:, :4] = (torch.rand(n_fit, 4, generator=g) > 0.5).float()
motion[:, 4:7] = torch.cumsum(torch.randn(n_fit, 3, generator=g) * 0.05, 0)
motion[:, 7:] = random_6d(n_fit * 24).reshape(n_fit, 144)
norm = Normalizer(motion.reshape(8, 150, 151).clone())


def quantize(x):
    return torch.round(x / SCALE).clamp(-32767, 32767).to(torch.int16)


# normal: values mostly inside [-1, 1]; some outside (the clamp)
normal_q = quantize(torch.randn(2, 300, 151, generator=g) * 0.45)
# long: window k + 1's first half = window k's second half + per-frame noise of scale 0, 1e-3 .. 0.5
lw = torch.randn(3, 150, 2, 151, generator=g) * 0.45
amp = torch.tensor([0.0, 0.0, 1e-3, 1e-2, 0.1, 0.5]).repeat(13)[:75]
for k in range(2):
    lw[k + 1, :75] = lw[k, 75:] + torch.randn(75, 2, 151, generator=g) * amp[:, None, None]
long_q = quantize(lw.reshape(3, 300, 151))


def run(xq, mode, names, epoch):
    calls.clear()
    diff = GaussianDiffusion.__new__(GaussianDiffusion)
    torch.nn.Module.__init__(diff)
    diff.smpl = RV.SMPLSkeleton("cpu")
    x = xq.float() * SCALE
    with tempfile.TemporaryDirectory() as d:
        diff.render_sample(x.clone(), torch.zeros(1), norm, epoch, os.path.join(d, "render"), fk_out=os.path.join(d, "fk"),
                           name=names, mode=mode, required_dancer_num=2)
        files = sorted(os.listdir(os.path.join(d, "fk")))
        data = []
        for f in files:
            with open(os.path.join(d, "fk", f), "rb") as fh:
                data.append(pickle.load(fh))
    return files, data, list(calls)


out = {"normal_x": normal_q.numpy(), "long_x": long_q.numpy(), "sample_scale": np.float64(SCALE),
       "scale_": norm.scaler.scale_.numpy(), "min_": norm.scaler.min_.numpy()}
normal_names = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]
files, data, rec = run(normal_q, "normal", normal_names, 7)
assert len(files) == 2 and len(rec) == 2
out["normal_files"] = np.array(files)
for i, (f, dct) in enumerate(zip(files, data)):
    assert list(dct) == ["smpl_poses", "smpl_trans", "full_pose"]
    num = int(f.split("_")[1])
    for key, v in dct.items():
        assert v.dtype == np.float32, (key, v.dtype)
        out[f"normal_{num}_{key}"] = v
for num, (pose, kw) in enumerate(rec):
    assert np.array_equal(pose, out[f"normal_{num}_full_pose"])
    out[f"normal_render_contact_{num}"] = np.asarray(kw["contact"], dtype=np.float32)
    out[f"normal_render_epoch_{num}"] = np.array(kw["epoch"])
    out[f"normal_render_name_{num}"] = np.array(kw["name"])

long_names = ["data/test/features/gLH_sBM_c01_d16_mLH2_ch04_slice0.npy"]
files, data, rec = run(long_q, "long", long_names, 3)
assert len(files) == 1 and len(rec) == 1
out["long_files"] = np.array(files)
for key, v in data[0].items():
    assert v.dtype == np.float32, (key, v.dtype)
    out[f"long_{key}"] = v
pose, kw = rec[0]
assert np.array_equal(pose, out["long_full_pose"])          # render_len 512 > 300 frames: the whole song
out["long_render_epoch"] = np.array(kw["epoch"])
out["long_render_stitch"] = np.array(bool(kw["stitch"]))
path = os.path.join(HERE, "render_export.npz")
np.savez_compressed(path, **out)
print(files, {k: v.shape for k, v in out.items()}, os.path.getsize(path))
