"""Workload for timing ground and ground_metrics (profiles/ground.txt):

    python tools/ground_time.py [repeats] [out.txt] [time limit in seconds]

Two workloads a user would run: 16 clips x 3 dancers x 150 frames, and one long song of 1 x 3 x 1200 frames, on tests/ground_ref.py's
seeded inputs at the default parameters, each with the contacts given and with the still rule.  After one warm-up per case the five
launches of ``tcf_ground`` are timed as a whole with device events, then the four with the floor given (no median), then the three of
``tcf_ground_metrics`` and its two with the floor given; the differences price the median launch and the walk + apply launches.  The
kernels one by one are a matter for rocprofv3, not for this tool.  Prints one line per measurement and, with a second argument, also
writes them there.  The whole run is ended by an alarm after the time limit (300 s unless given)."""
import os
import signal
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ground_ref as R  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd.fk import SMPL_PARENTS  # noqa: E402
from tcdiff_amd.group_metrics import capsule_radii  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"ground_time: not finished after {limit} s"))
    signal.alarm(limit)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = "cuda:0"
    parents, radii = [0] + list(SMPL_PARENTS[1:]), capsule_radii().tolist()
    for what, (b, dn, T) in (("16 clips x 3 dancers x 150 frames", (16, 3, 150)), ("one long song, 1 x 3 x 1200 frames", (1, 3, 1200))):
        pos, J, Cn = (torch.from_numpy(np.array(a)).to(dev) for a in R.seeded(b, dn, T))
        ws = torch.empty(K.ground_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        pos_out, joints_out = torch.empty_like(pos), torch.empty_like(J)
        f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
        i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)
        floor, given = f64(b), torch.zeros(b, dtype=torch.float64, device=dev)
        cb, vb, ca, va, capped, ms, mt = i64(3, b, dn), f64(3, b, dn), i64(3, b, dn), f64(3, b, dn), i64(b, dn), f64(b, dn), f64(b, dn)
        for kind, c in (("contacts", Cn), ("still rule", None)):
            def full(floor_in):
                K.ground(pos, J, c, 2, parents, radii, floor_in, 0.95, 0.01, 0.005, 5, 0.5, ws, pos_out, joints_out, None, floor, cb, vb, ca, va,
                         capped, ms, mt)

            def measure(floor_in):
                K.ground_metrics(J, c, 2, parents, radii, floor_in, 0.95, 0.01, 0.005, ws, floor, cb, vb)

            def timed(fn, *args):
                fn(*args)                                                  # the warm-up
                torch.cuda.synchronize()
                times = []
                for _ in range(repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(*args)
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e3)
                return statistics.median(times), min(times), max(times)

            full(None)
            torch.cuda.synchronize()
            say(f"{what}, {kind}: workspace {ws.numel() / 2 ** 20:.2f} MiB; floor {float(floor.min()):.4f} .. {float(floor.max()):.4f} m; "
                f"planted frames {int(cb[0].sum())}; penetration frames {int(cb[1].sum())} -> {int(ca[1].sum())}; float frames "
                f"{int(cb[2].sum())} -> {int(ca[2].sum())}; capped {int(capped.sum())}; largest shift {float(ms.max()):.4f} m, largest step "
                f"{float(mt.max()):.4f} m a frame")
            med = {}
            for name, fn, arg, n in (("ground, floor estimated", full, None, 5), ("ground, floor given", full, given, 4),
                                     ("ground_metrics, floor estimated", measure, None, 3), ("ground_metrics, floor given", measure, given, 2)):
                med[name], lo, hi = timed(fn, arg)
                say(f"  {name}: {n} launches, device events, {repeats} repeats after one warm-up: median {med[name]:.1f} us, min {lo:.1f} us, "
                    f"max {hi:.1f} us")
            say(f"  the median launch: {med['ground, floor estimated'] - med['ground, floor given']:.1f} us (from ground), "
                f"{med['ground_metrics, floor estimated'] - med['ground_metrics, floor given']:.1f} us (from ground_metrics); walk + apply + the "
                f"second evaluation: {med['ground, floor given'] - med['ground_metrics, floor given']:.1f} us")
    signal.alarm(0)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
