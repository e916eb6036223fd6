"""navigator.npz: the REAL reference's TrajDecoder (TrajDecoder/model/traj_model.py) and the rollout of TCDiff.py:526-547 on the
seeded weights / inputs of tests/navigator_ref.py, run twice -- in fp32 and after .double().

Per case of navigator_ref.CASES: both rollouts (or forward outputs) in full; for the FIRST window, via forward hooks, the LSTM
output, music_projection's output and every block's output -- of the float64 run a fixed sample of elements
(navigator_ref.sample_idx) and the top magnitude, and the yardstick max|fp32 - f64| / max|f64| of the whole tensor.  Also the 133
state_dict keys and shapes of TrajDecoder(nfeats=2, trans_layer=6, window_size=100).  Data only.  Build container only (needs the
reference checkout; REF_ROOT overrides its place)."""
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
from model.traj_model import TrajDecoder  # noqa: E402

torch.set_num_threads(8)
out = {}


def run(model, x, cond, window, step, forward_only):
    stages = {"blocks": []}
    n_layers = len(model.trans_extractor.blocks)

    def keep(key, pick):                      # first window only; a hook that returns a value would replace the output
        def hook(m, i, o):
            if key == "blocks":
                if len(stages["blocks"]) < n_layers:
                    stages["blocks"].append(o.detach())
            elif key not in stages:
                stages[key] = pick(o).detach()
        return hook
    hooks = [model.lstm.register_forward_hook(keep("lstm", lambda o: o[0])),
             model.music_projection.register_forward_hook(keep("music", lambda o: o))]
    for blk in model.trans_extractor.blocks:
        hooks.append(blk.register_forward_hook(keep("blocks", None)))
    with torch.no_grad():
        if forward_only:
            res = model(x, cond)
        else:
            cur = x[:, :, :window]
            pieces = [cur]
            for start in range(0, cond.shape[1] + 1 - (window + step) * 2, step * 2):      # TCDiff.py:540-544
                cur = model(cur, cond[:, start:start + (window + step) * 2])
                pieces.append(cur[:, :, -step:])
            res = torch.cat(pieces, dim=2)
    for h in hooks:
        h.remove()
    stages["blocks"] = torch.stack(stages["blocks"])
    return res, stages


for name, layers, window, step, dn, b, cond_len in R.CASES:
    model = TrajDecoder(nfeats=2, trans_layer=layers, window_size=window).eval()
    model.load_state_dict(R.synth_state_dict(model), strict=True)
    x, cond = R.synth_inputs(name, window, dn, b, cond_len)
    fwd = name.startswith("forward")
    r32, s32 = run(model, x, cond, window, step, fwd)
    model = model.double()
    r64, s64 = run(model, x.double(), cond.double(), window, step, fwd)
    out[f"{name}.out32"] = r32.numpy()
    out[f"{name}.out64"] = r64.numpy()
    pred32, pred64 = (r32, r64) if fwd else (r32[:, :, window:], r64[:, :, window:])
    out[f"{name}.out_yardstick"] = np.float64(R.rel_err(pred32, pred64))
    for st in ("lstm", "music", "blocks"):
        flat = s64[st].reshape(-1).numpy()
        out[f"{name}.{st}.sample64"] = flat[R.sample_idx(flat.size)]
        out[f"{name}.{st}.shape"] = np.array(s64[st].shape)
        out[f"{name}.{st}.top"] = np.float64(np.abs(flat).max())
        out[f"{name}.{st}.yardstick"] = np.float64(R.rel_err(s32[st], s64[st]))
    print(name, "frames", r64.shape[2], "max", float(r64.abs().max()), "std", float(pred64.std()),
          "yardsticks: out %.2e" % out[f"{name}.out_yardstick"],
          " ".join("%s %.2e" % (st, out[f"{name}.{st}.yardstick"]) for st in ("lstm", "music", "blocks")))

model = TrajDecoder(nfeats=2, trans_layer=6, window_size=100)
sd = model.state_dict()
out["keys"] = np.array(list(sd.keys()))
out["shapes"] = np.array([str(tuple(v.shape)) for v in sd.values()])
out["n_params"] = np.int64(sum(p.numel() for p in model.parameters()))
np.savez_compressed(os.path.join(HERE, "navigator.npz"), **out)
print("wrote navigator.npz", os.path.getsize(os.path.join(HERE, "navigator.npz")), "bytes")
