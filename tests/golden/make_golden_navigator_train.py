"""navigator_train.npz: the REAL reference's TrajDecoder(..., dropout=0.0) in .train() mode and float64, on the seeded weights /
inputs of tests/navigator_ref.py at case A of tests/navigator_train_ref.py and a seeded target: the loss of
TrajDecoder/train_traj.py:183-196, and of the output and of every parameter's gradient a fixed sample of elements
(navigator_ref.sample_idx) with the top magnitude.  Parameters autograd leaves without a gradient are listed in `none`.  Data only.
Build container only (needs the reference checkout; REF_ROOT overrides its place)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "TrajDecoder"))
import navigator_ref as R  # noqa: E402
import navigator_train_ref as TR  # noqa: E402
from model.traj_model import TrajDecoder  # noqa: E402

torch.set_num_threads(8)
name, layers, window, dn, b, frames, _ = TR.CASES[0]
model = TrajDecoder(nfeats=2, trans_layer=layers, window_size=window, dropout=0.0)
model.load_state_dict(R.synth_state_dict(model), strict=True)
model = model.double().train()
x, cond = R.synth_inputs("train." + name, window, dn, b, frames)
x_target = TR.synth_target(name, b, dn, window).double()
pre_traj = model(x.double(), cond.double())

# the loss of train_traj.py:183-196, written independently of the helper under test: squared error of the positions, and twice
# each of the dancer-to-dancer and frame-to-frame differences
sq = lambda t: t.pow(2).mean()
err = pre_traj - x_target
loss = sq(err) + 2 * sq(torch.diff(err, dim=1)) + 2 * sq(torch.diff(err, dim=2))
loss.backward()

out = {"loss": np.float64(loss.item())}
flat = pre_traj.detach().reshape(-1).numpy()
out["out.sample"], out["out.top"], out["out.shape"] = flat[R.sample_idx(flat.size)], np.float64(np.abs(flat).max()), \
    np.array(pre_traj.shape)
none = []
for k, p in model.named_parameters():
    if p.grad is None:
        none.append(k)
        continue
    flat = p.grad.reshape(-1).numpy()
    out[f"grad.{k}.sample"], out[f"grad.{k}.top"] = flat[R.sample_idx(flat.size)], np.float64(np.abs(flat).max())
out["none"] = np.array(none)
np.savez_compressed(os.path.join(HERE, "navigator_train.npz"), **out)
print("loss", loss.item(), "none", none, "wrote", os.path.getsize(os.path.join(HERE, "navigator_train.npz")), "bytes")
