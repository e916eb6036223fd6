"""Time the Dance-Beat Navigator rollout on the GPU: tcdiff_amd.navigator.rollout against the float32 torch evaluation of
tests/navigator_ref.py (nn.LSTM + aten ops, the baseline a user has without the kernels) on the same device.

    python tools/navigator_bench.py [--runs 20] [--out profiles/navigator_rollout.txt]
    python tools/navigator_bench.py --once 301        # a single warm rollout (for a kernel trace)

Shape: trans_layer 6, window 100, step 25, 3 dancers, 30 clips, 301 and 1801 music frames.  Warm; median of --runs rollouts, each
timed with a host clock around a device synchronise; the two implementations alternate."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import navigator_ref as R  # noqa: E402
from tcdiff_amd import TrajDecoder  # noqa: E402
from tcdiff_amd import navigator as N  # noqa: E402

LAYERS, WINDOW, STEP, DN, B = 6, 100, 25, 3, 30


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("navigator_bench needs the GPU")
    dev = "cuda"
    m = TrajDecoder(nfeats=2, trans_layer=LAYERS, window_size=WINDOW)
    sd = R.synth_state_dict(m)
    m.load_state_dict(sd)
    m.to(dev).eval()
    sd32 = R.to(sd, torch.float32, dev)
    lstm = torch.nn.LSTM(2, 64, 3).to(dev).eval()
    lstm.load_state_dict({k[5:]: v for k, v in sd32.items() if k.startswith("lstm.")})
    lines = []
    for frames in ([a.once] if a.once else [301, 1801]):
        x, cond = R.synth_inputs(f"bench{frames}", WINDOW, DN, B, frames)
        x, cond = x.to(dev), cond.to(dev)
        hip = lambda: N.rollout(m, x, cond, step=STEP)
        if a.once:
            hip()
            ms, _ = timed(hip)
            print(f"{frames} frames: one warm rollout {ms:.3f} ms")
            return
        with torch.no_grad():
            ref = lambda: R.rollout(sd32, x, cond, LAYERS, WINDOW, STEP, lstm=lstm)
            for _ in range(3):
                got, want = hip(), ref()
            th, tr = [], []
            for _ in range(max(20, a.runs)):
                th.append(timed(hip)[0])
                tr.append(timed(ref)[0])
        want64 = R.rollout(R.to(sd, torch.float64), x.cpu().double(), cond.cpu().double(), LAYERS, WINDOW, STEP)
        nw = len(N.window_starts(frames, WINDOW, STEP))
        lines.append(f"{frames} music frames, b {B}, dn {DN}, {nw} windows: HIP rollout median {statistics.median(th):.3f} ms "
                     f"(min {min(th):.3f}, max {max(th):.3f}); torch float32 restatement median {statistics.median(tr):.3f} ms "
                     f"(min {min(tr):.3f}, max {max(tr):.3f}); ratio {statistics.median(tr) / statistics.median(th):.2f}x; "
                     f"{len(th)} runs each, alternating")
        lines.append(f"    predicted frames vs float64: HIP {R.rel_err(got[:, :, WINDOW:], want64[:, :, WINDOW:]):.3e}, "
                     f"torch float32 on the GPU {R.rel_err(want[:, :, WINDOW:], want64[:, :, WINDOW:]):.3e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
