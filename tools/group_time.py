"""Workload for timing the group metrics (profiles/group.txt):

    python tools/group_time.py [repeats] [out.txt] [time limit in seconds]

Two workloads a user would run: 16 clips x 3 dancers x 150 frames, and one long song of 1 x 3 x 1200 frames, with the default
parameters (window 30 frames, 15 lags either way).  Seeded synthetic dancers (tests/group_ref.py ``synth``).  After one warm-up per
shape, each repeat times the three launches of ``tcg_group_metrics`` with device events; then a window of 200 calls back to back is
timed as a whole, which is what a caller in a loop pays per call.  The kernels one by one are a matter for rocprofv3, not for this
tool.  Prints one line per measurement and, with a second argument, also writes them there.  The whole run is ended by an alarm
after the time limit (300 s unless given)."""
import os
import signal
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import group_ref as R  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd import metrics as M  # noqa: E402
from tcdiff_amd.fk import SMPL_PARENTS  # noqa: E402
from tcdiff_amd.group_metrics import capsule_radii, group_metrics  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"group_time: not finished after {limit} s"))
    signal.alarm(limit)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = "cuda:0"
    parents, radii = [-1] + list(SMPL_PARENTS[1:]), capsule_radii().tolist()
    for what, (b, dn, T) in (("16 clips x 3 dancers x 150 frames", (16, 3, 150)), ("one long song, 1 x 3 x 1200 frames", (1, 3, 1200))):
        J = torch.from_numpy(np.array(R.synth(b, dn, T, seed=100))).to(dev)          # a copy: synth's arrays are read-only
        P = dn * (dn - 1) // 2
        ws = torch.empty(K.group_workspace(b, dn, T, 15), dtype=torch.uint8, device=dev)
        f64 = [torch.empty(b, P, dtype=torch.float64, device=dev) for _ in range(5)]
        i64 = [torch.empty(b, P, dtype=torch.int64, device=dev) for _ in range(3)]
        closest = torch.empty(b, P, 3, dtype=torch.int64, device=dev)

        def call():
            K.group_metrics(J, 2, 30.0, parents, radii, 30, 15, 1e-6, ws, None, None, f64[0], f64[1], i64[0], closest, i64[1], f64[2], f64[3],
                            i64[2], f64[4])
        call()                                                             # the warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            call()
        e1.record()
        torch.cuda.synchronize()
        s = M.summarize(group_metrics(J))
        say(f"{what}: {b * P} pairs, workspace {ws.numel() / 2 ** 20:.2f} MiB; contact rate {s['body_contact_rate']:.3f}, "
            f"crossings {s['path_crossings']:.2f} a pair, sync {s['sync']:.3f}")
        say(f"  three launches, device events, {repeats} repeats after one warm-up: median {statistics.median(times) * 1e3:.1f} us, "
            f"min {min(times) * 1e3:.1f} us, max {max(times) * 1e3:.1f} us")
        say(f"  200 calls back to back: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per call, "
            f"{e0.elapsed_time(e1) / 200 * 1e6 / (b * P * T):.1f} ns per pair and frame")
    signal.alarm(0)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
