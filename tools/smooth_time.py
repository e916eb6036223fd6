"""Workload for timing the jitter scores and the rotation filter (profiles/smooth.txt):

    python tools/smooth_time.py [repeats] [out.txt] [time limit in seconds]

Two workloads a user would run: 16 clips x 3 dancers x 150 frames, and one long song of 1 x 3 x 1200 frames, each with the default
window 9 and with the largest, 63 (order 3).  Seeded noisy dances (tests/smooth_ref.py ``noisy_case``).  After one warm-up per shape,
each repeat times the two launches of ``tcw_smooth`` as a whole with device events (both FK outputs asked for, as ``smooth`` does with
``measure=True``), and in the same run the one launch of ``tcw_smoothness`` and the three of ``tck_foot_lock`` on the same poses;
then a window of 200 calls back to back is timed as a whole, which is what a caller in a loop pays per call.  The two launches one by
one are a matter for rocprofv3 (``--kernel-trace --stats``), not for this tool.  Each result is also held to the numpy restatement
and the largest error per output is printed.
Prints one line per measurement and, with a second argument, also writes them there.  The whole run is ended by an alarm after the
time limit (300 s unless given)."""
import importlib
import os
import signal
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smooth_ref as R  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS  # noqa: E402
from tcdiff_amd.footlock import foot_lock  # noqa: E402

S = importlib.import_module("tcdiff_amd.smooth")


def timed(call, repeats):
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def line(what, t):
    return f"  {what}: median {statistics.median(t) * 1e3:.1f} us, min {min(t) * 1e3:.1f} us, max {max(t) * 1e3:.1f} us"


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"smooth_time: not finished after {limit} s"))
    signal.alarm(limit)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    for what, (b, dn, T) in (("16 clips x 3 dancers x 150 frames", (16, 3, 150)), ("one long song, 1 x 3 x 1200 frames", (1, 3, 1200))):
        _, _, qh, ph = R.noisy_case(b=b, dn=dn, T=T, seed=100)
        q, pos = torch.from_numpy(np.array(qh)).to(dev), torch.from_numpy(np.array(ph)).to(dev)          # copies: the cases are read-only
        ws = torch.empty(K.smooth_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        q_out, pos_out = torch.empty_like(q), torch.empty_like(pos)
        joints, joints_in = torch.empty(b, dn, T, 24, 3, device=dev), torch.empty(b, dn, T, 24, 3, device=dev)
        f64 = [torch.empty(b, dn, dtype=torch.float64, device=dev) for _ in range(8)]
        i32 = [torch.empty(b, dn, 2, dtype=torch.int32, device=dev) for _ in range(2)] + [torch.empty(b, dn, dtype=torch.int32, device=dev) for _ in range(2)]

        def score():
            K.smoothness(joints, 30.0, *f64[:6], i32[0], i32[1], i32[2])

        def lock():
            foot_lock(q, pos, None, dn=dn)

        for W in (9, 63):
            taps = S._table_on(W, 3, dev)

            def call():
                K.smooth(q, pos, b, dn, T, W, taps, W, taps, R.ALL, SMPL_PARENTS, SMPL_OFFSETS, ws, q_out, pos_out, joints, joints_in, f64[6],
                         f64[7], i32[3])

            call()                                                         # the warm-ups
            score()
            lock()
            torch.cuda.synchronize()
            mine, scores, theirs = timed(call, repeats), timed(score, repeats), timed(lock, repeats)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                call()
            e1.record()
            torch.cuda.synchronize()
            got = S.smooth(q, pos, dn=dn, window=W)
            ref = R.smooth(qh, ph, dn, window=W)
            gq, gp = got.q.cpu().numpy(), got.pos.cpu().numpy()
            rot = float(R.angles(gq.astype(np.float64), ref["q64"]).max())
            st = R.stats(qh, ph, gq, gp, dn)
            rel = lambda a, w: float((np.abs(a - w) / np.maximum(np.abs(w), 1e-300)).max())          # a statistic that is exactly 0 stays 0
            after = R.smoothness(got.joints.cpu().numpy())
            worst = max(rel(got.after[k].cpu().numpy(), after[k]) for k in R.FLOATS)
            same = all(np.array_equal(got.after[k].cpu().numpy(), after[k]) for k in R.INTS)
            moved = 4 * (2 * q.numel() + 2 * pos.numel() + 2 * joints.numel()) / 2 ** 20
            say(f"{what}, window {W} / order 3: {b * dn} dancers, workspace {ws.numel() / 2 ** 10:.1f} KiB, {moved:.1f} MiB in and out; jitter "
                f"{float(got.before['jitter'].mean()):.0f} -> {float(got.after['jitter'].mean()):.0f} m/s^3, accel "
                f"{float(got.before['accel_mean'].mean()):.1f} -> {float(got.after['accel_mean'].mean()):.1f} m/s^2")
            say(line(f"tcw_smooth, two launches with both FK outputs, device events, {repeats} repeats after one warm-up", mine))
            say(line("tcw_smoothness on the output's joints, one launch, the same run", scores))
            say(line("foot_lock on the same poses (labels from the motion), three launches, the same run", theirs))
            say(f"  200 calls of tcw_smooth back to back: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per call, "
                f"{e0.elapsed_time(e1) / 200 * 1e6 / (b * dn * T):.1f} ns per dancer and frame")
            say(f"  against the float64 restatement: pos {'equal bits' if np.array_equal(gp.view(np.int32), ref['pos'].view(np.int32)) else 'DIFFERENT'}, "
                f"rotations {rot:.2e} rad, max_rot_change {rel(got.max_rot_change.cpu().numpy(), st['max_rot_change']):.1e}, max_pos_change "
                f"{rel(got.max_pos_change.cpu().numpy(), st['max_pos_change']):.1e}, scores {worst:.1e} (relative), integers "
                f"{'equal' if same and np.array_equal(got.copied.cpu().numpy(), ref['copied']) else 'DIFFERENT'}")
    signal.alarm(0)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
