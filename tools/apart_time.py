"""Workload for timing keep_apart (profiles/apart.txt):

    python tools/apart_time.py [repeats] [out.txt] [time limit in seconds]

Two workloads a user would run: 16 clips x 3 dancers x 150 frames, and one long song of 1 x 3 x 1200 frames, at the default
parameters.  Each is timed twice: on inputs without contact (tests/apart_ref.py ``spread`` by 3 m: every frame costs one evaluation of
the gap per round) and on the spread seeded inputs (0.8 m: dancers that meet now and then).  After one warm-up per case the 2 rounds
+ 3 launches of ``tcp_keep_apart`` are timed as a whole with device events for rounds = 0, 1, 2, 3: rounds = 0 is apply + verify +
stats, and each further round adds one demand and one combine launch, so the differences are the cost of a round.  The demand launch
alone is timed as the difference of iterations = 8 and iterations = 0 at one round (the latter evaluates every gap once and pushes
nothing).  The kernels one by one are a matter for rocprofv3, not for this tool.  Prints one line per measurement and, with a second
argument, also writes them there.  The whole run is ended by an alarm after the time limit (300 s unless given)."""
import os
import signal
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import apart_ref as A  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd.apart import keep_apart  # noqa: E402
from tcdiff_amd.fk import SMPL_PARENTS  # noqa: E402
from tcdiff_amd.group_metrics import capsule_radii  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"apart_time: not finished after {limit} s"))
    signal.alarm(limit)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = "cuda:0"
    parents, radii = [0] + list(SMPL_PARENTS[1:]), capsule_radii().tolist()
    for what, (b, dn, T) in (("16 clips x 3 dancers x 150 frames", (16, 3, 150)), ("one long song, 1 x 3 x 1200 frames", (1, 3, 1200))):
        for kind, by in (("without contact", 3.0), ("spread seeded input", A.SPREAD)):
            pos, J = (torch.from_numpy(np.array(a)).to(dev) for a in A.spread(b, dn, T, seed=100, by=by))
            P = dn * (dn - 1) // 2
            ws = torch.empty(K.keep_apart_workspace(b, dn, T), dtype=torch.uint8, device=dev)
            pos_out, joints_out = torch.empty_like(pos), torch.empty_like(J)
            i64 = [torch.empty(b, P, dtype=torch.int64, device=dev) for _ in range(4)]
            f64 = [torch.empty(b, P, dtype=torch.float64, device=dev) for _ in range(2)] + \
                  [torch.empty(b, dn, dtype=torch.float64, device=dev) for _ in range(2)]

            def call(rounds, iterations=8):
                K.keep_apart(pos, J, 2, parents, radii, [1.0] * dn, 0.02, iterations, rounds, 5, 0.6, ws, pos_out, joints_out, None, i64[0], i64[1],
                             f64[0], f64[1], i64[2], i64[3], f64[2], f64[3])

            def timed(rounds, iterations=8):
                call(rounds, iterations)                                   # the warm-up
                torch.cuda.synchronize()
                times = []
                for _ in range(repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(rounds, iterations)
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e3)
                return statistics.median(times), min(times), max(times)

            out = keep_apart(pos, J, dn=dn)
            say(f"{what}, {kind}: {b * P} pairs, workspace {ws.numel() / 2 ** 20:.2f} MiB; contact frames "
                f"{int(out.contact_before.sum())} -> {int(out.contact_after.sum())}, pushed {int(out.pushed.sum())}, capped {int(out.capped.sum())}, "
                f"deepest gap {float(out.gap_min_before.min()):.4f} -> {float(out.gap_min_after.min()):.4f} m, largest shift "
                f"{float(out.max_shift.max()):.4f} m, largest step {float(out.max_step.max()):.4f} m a frame")
            med = {}
            for rounds in (0, 1, 2, 3):
                med[rounds], lo, hi = timed(rounds)
                say(f"  rounds = {rounds}, {2 * rounds + 3} launches, device events, {repeats} repeats after one warm-up: median {med[rounds]:.1f} us, "
                    f"min {lo:.1f} us, max {hi:.1f} us")
            once = timed(1, 0)[0]
            say(f"  apply + verify + stats: {med[0]:.1f} us; a round (demand + combine): {(med[3] - med[0]) / 3:.1f} us on average, the first "
                f"{med[1] - med[0]:.1f} us; one round with iterations = 0 (one evaluation a frame): {once - med[0]:.1f} us, so the iteration "
                f"costs {med[1] - once:.1f} us of the first round")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                call(3)
            e1.record()
            torch.cuda.synchronize()
            say(f"  100 calls back to back at the defaults: {e0.elapsed_time(e1) / 100 * 1e3:.1f} us per call, "
                f"{e0.elapsed_time(e1) / 100 * 1e6 / (b * P * T):.1f} ns per pair and frame")
    signal.alarm(0)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
