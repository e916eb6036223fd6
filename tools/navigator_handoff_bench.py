"""Time the Navigator -> sampler hand-off on the GPU: `rollout` + `io.x0_from_navigator` (device -> host copy, the numpy Kalman
loop, host -> device copy, zero-pad and permute in torch) against `navigator.rollout_x0` (the rollout's launches followed by one
launch of csrc/handoff.hip), and the hand-off alone on a finished rollout.

    python tools/navigator_handoff_bench.py [--runs 20] [--out FILE]

Shape as tools/navigator_bench.py: trans_layer 6, window 100, step 25, 3 dancers, 30 clips, 301 and 1801 music frames.  Warm;
median of --runs calls, each timed with a host clock around a device synchronise, the forms alternating in one process; the
kernel's own time from device events around the one launch.  --out appends."""
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
from tcdiff_amd import io as IO  # noqa: E402
from tcdiff_amd import navigator as N  # noqa: E402

LAYERS, WINDOW, STEP, DN, B = 6, 100, 25, 3, 30


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("navigator_handoff_bench needs the GPU")
    dev = "cuda"
    m = TrajDecoder(nfeats=2, trans_layer=LAYERS, window_size=WINDOW)
    m.load_state_dict(R.synth_state_dict(m))
    m.to(dev).eval()
    lines = []
    for music in (301, 1801):
        x, cond = R.synth_inputs(f"bench{music}", WINDOW, DN, B, music)
        x, cond = x.to(dev), cond.to(dev)
        host = lambda: IO.x0_from_navigator(N.rollout(m, x, cond, step=STEP))
        fused = lambda: N.rollout_x0(m, x, cond, step=STEP)
        roll = lambda: N.rollout(m, x, cond, step=STEP)
        for _ in range(3):
            want, got, traj = host(), fused(), roll()
        out = torch.empty_like(got)
        alone = lambda: N.smooth_x0(traj, out=out)
        host_alone = lambda: IO.x0_from_navigator(traj)
        alone(), host_alone()
        th, tf, tr, ta, tk, tha = [], [], [], [], [], []
        for _ in range(max(1, a.runs)):
            th.append(timed(host)[0])
            tf.append(timed(fused)[0])
            tr.append(timed(roll)[0])
            tha.append(timed(host_alone)[0])
            ta.append(timed(alone)[0])
            tk.append(event_ms(alone))
        frames = traj.shape[2]
        diff = float((got - want).abs().max())
        lines += [f"{music} music frames, b {B}, dn {DN}, {frames} trajectory frames, {len(th)} runs each, alternating:",
                  f"    rollout + io.x0_from_navigator : {med(th)}",
                  f"    rollout_x0                     : {med(tf)}   ratio {statistics.median(th) / statistics.median(tf):.3f}x",
                  f"    rollout alone                  : {med(tr)}",
                  f"    io.x0_from_navigator alone     : {med(tha)}",
                  f"    smooth_x0 alone, host clock    : {med(ta)}",
                  f"    smooth_x0 alone, device events : {med(tk)}",
                  f"    max |rollout_x0 - io.x0_from_navigator(rollout)| = {diff:.3e}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
