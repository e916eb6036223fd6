"""Workload for timing the choreography planner and its closing check (profiles/choreo.txt):

    python tools/choreo_time.py [repeats] [out.txt] [time limit in seconds]

Two workloads a user would run: 16 clips x 3 dancers x 150 frames with 6 keys, and one long song of 1 x 3 x 1200 frames with 40 keys,
seeded waypoints (tests/choreo_ref.py ``case``) with a 151-column normaliser's numbers.  After one warm-up per shape, each repeat times
the two launches of ``tcc_plan`` as a whole with device events, and in the same run the one launch of ``tcc_trajectory_error`` on
joints of the same shape and the one launch of ``smooth_x0`` (csrc/handoff.hip) on the planned trajectories, the yardstick for a
launch-bound hand-off; then a window of 200 calls back to back is timed as a whole, which is what a caller in a loop pays per call.
The launches one by one are a matter for rocprofv3 (``--kernel-trace --stats``), not for this tool.  Each plan is also held to the
numpy restatement.
Prints one line per measurement and, with a second argument, also writes them there.  The whole run is ended by an alarm after the
time limit (300 s unless given)."""
import os
import signal
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import choreo_ref as R  # noqa: E402
from tcdiff_amd import choreo as CH  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd.navigator import smooth_x0  # noqa: E402

SCALE, MIN = [0.4, 0.55], [0.1, -0.2]


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
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"choreo_time: not finished after {limit} s"))
    signal.alarm(limit)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    for what, (b, dn, T, nk) in (("16 clips x 3 dancers x 150 frames, 6 keys", (16, 3, 150, 6)), ("one long song, 1 x 3 x 1200 frames, 40 keys", (1, 3, 1200, 40))):
        keys_h, points_h, counts_h = R.case(b, dn, T, nk, seed=100, per_dancer=True)
        keys, points, counts = (torch.from_numpy(a).to(dev) for a in (keys_h, points_h, counts_h))
        P = dn * (dn - 1) // 2
        f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
        traj, x0 = torch.empty(b, dn, T, 2, device=dev), torch.empty(b, T * dn, 3, device=dev)
        rep = [i32(b, dn), i32(b, dn), f64(b, dn), i32(b, dn), i32(b, dn), f64(b, dn), f64(b, P), i32(b, P), i32(b, P)]
        joints = torch.randn(b, T, dn, 24, 3, device=dev).permute(0, 2, 1, 3, 4)          # the permuted view of a frame-major buffer
        err = [f64(b, dn), f64(b, dn), f64(b, dn), i32(b, dn), i32(b, dn)]
        x0_nav = torch.empty(b, T * dn, 3, device=dev)

        def call():
            K.choreo_plan(points, keys, counts, T, 30.0, SCALE, MIN, 0.5, 3.0, traj, x0, *rep)

        def check():
            K.trajectory_error(joints, traj, 2, *err)

        def handoff():
            smooth_x0(traj, out=x0_nav)

        call()                                                             # the warm-ups
        check()
        handoff()
        torch.cuda.synchronize()
        mine, checks, theirs = timed(call, repeats), timed(check, repeats), timed(handoff, repeats)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            call()
        e1.record()
        torch.cuda.synchronize()
        ref = R.plan(keys_h, points_h, T, counts_h, 30.0, SCALE, MIN, 0.5, 3.0)
        got = dict(zip(("status", "clamped", "speed_max", "speed_peak", "too_fast", "path_length", "dist_min", "dist_min_frame", "too_close"),
                       (r.cpu().numpy() for r in rep)), traj=traj.cpu().numpy(), x_0=x0.cpu().numpy())
        same = all(np.array_equal(got[k].view(np.int32) if got[k].dtype == np.float32 else got[k], ref[k].view(np.int32) if ref[k].dtype == np.float32 else ref[k])
                   for k in got)
        moved = (points.numel() * 4 + keys.numel() * 4 + 2 * traj.numel() * 4 + x0.numel() * 4) / 2 ** 10
        say(f"{what}: {b * dn} dancers, {b * P} pairs, {moved:.1f} KiB in and out; {int(got['clamped'].sum())} frames clamped, "
            f"{int(got['too_fast'].sum())} too fast, {int(got['too_close'].sum())} too close")
        say(line(f"tcc_plan, two launches, device events, {repeats} repeats after one warm-up", mine))
        say(line("tcc_trajectory_error on joints of the same shape (a permuted view), one launch, the same run", checks))
        say(line("smooth_x0 on the planned trajectories, one launch, the same run", theirs))
        say(f"  200 calls of tcc_plan back to back: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per call, "
            f"{e0.elapsed_time(e1) / 200 * 1e6 / (b * dn * T):.1f} ns per dancer and frame")
        say(f"  against the float64 restatement: every output {'equal' if same else 'DIFFERENT'}")
    signal.alarm(0)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
