"""Workload for timing the self-contact metric (profiles/selfcontact.txt):

    python tools/selfcontact_time.py [repeats] [out.txt] [time limit in seconds]

Two workloads a user would run: 16 clips x 3 dancers x 150 frames, and one long song of 1 x 3 x 1200 frames, with the default
parameters (183 listed bone pairs, tolerance 3 cm).  Seeded FK scenes (tests/selfcontact_ref.py ``synth``).  After one warm-up per
shape, each repeat times the two launches of ``tci_self_contact`` as a whole with device events, and in the same run the three
launches of ``tcg_group_metrics`` on the same joints; then a window of 200 calls back to back is timed as a whole, which is what a
caller in a loop pays per call.  The two launches one by one are a matter for rocprofv3 (``--kernel-trace --stats``), not for this
tool.  Each result is also held to the numpy restatement and the largest error per output is printed.
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
import selfcontact_ref as R  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd import metrics as M  # noqa: E402
from tcdiff_amd.fk import SMPL_PARENTS  # noqa: E402
from tcdiff_amd.group_metrics import capsule_radii  # noqa: E402
from tcdiff_amd.self_contact import self_contact, self_pairs  # noqa: E402


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


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"selfcontact_time: not finished after {limit} s"))
    signal.alarm(limit)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = "cuda:0"
    parents, radii = [-1] + list(SMPL_PARENTS[1:]), capsule_radii().tolist()
    mask = self_pairs()
    words = [sum(1 << int(k - 64 * w) for k in np.flatnonzero(mask) if k // 64 == w) for w in range(4)]
    for what, (b, dn, T) in (("16 clips x 3 dancers x 150 frames", (16, 3, 150)), ("one long song, 1 x 3 x 1200 frames", (1, 3, 1200))):
        Jh = R.synth(b, dn, T, seed=100)
        J = torch.from_numpy(np.array(Jh)).to(dev)          # a copy: synth's arrays are read-only
        ws = torch.empty(K.self_contact_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        f64 = [torch.empty(b, dn, dtype=torch.float64, device=dev) for _ in range(3)]
        episodes = torch.empty(b, dn, dtype=torch.int64, device=dev)
        closest = torch.empty(b, dn, 3, dtype=torch.int64, device=dev)
        frames = torch.empty(b, dn, 253, dtype=torch.int64, device=dev)

        def call():
            K.self_contact(J, parents, radii, words, 0.03, ws, None, None, f64[0], f64[1], episodes, closest, f64[2], frames)

        P = dn * (dn - 1) // 2
        gws = torch.empty(K.group_workspace(b, dn, T, 15), dtype=torch.uint8, device=dev)
        g64 = [torch.empty(b, P, dtype=torch.float64, device=dev) for _ in range(5)]
        gi64 = [torch.empty(b, P, dtype=torch.int64, device=dev) for _ in range(3)]
        gclosest = torch.empty(b, P, 3, dtype=torch.int64, device=dev)

        def group():
            K.group_metrics(J, 2, 30.0, parents, radii, 30, 15, 1e-6, gws, None, None, g64[0], g64[1], gi64[0], gclosest, gi64[1], g64[2], g64[3],
                            gi64[2], g64[4])

        call()                                                             # the warm-ups
        group()
        torch.cuda.synchronize()
        mine, theirs = timed(call, repeats), timed(group, repeats)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            call()
        e1.record()
        torch.cuda.synchronize()
        got = self_contact(J, return_frames=True)
        s = M.summarize({k: v for k, v in got.items() if k not in ("gap", "closest")})
        ref = R.self_contact(Jh)
        worst = {}
        for k in R.FLOATS:
            g, w = got[k].cpu().numpy(), ref[k]
            ok = ~np.isnan(w)
            assert np.array_equal(np.isnan(g), ~ok), k
            worst[k] = float(np.abs(g - w)[ok].max()) if ok.any() else 0.0
        same = {k: bool(np.array_equal(got[k].cpu().numpy(), ref[k])) for k in R.INTS}
        say(f"{what}: {b * dn} dancers, {int(mask.sum())} of 253 bone pairs listed, workspace {ws.numel() / 2 ** 20:.2f} MiB; contact rate "
            f"{s['self_contact_rate']:.3f}, episodes {s['self_contact_episodes']:.2f} a dancer, mean depth {s['self_depth_mean'] * 100:.2f} cm")
        say(f"  self_contact, two launches, device events, {repeats} repeats after one warm-up: median {statistics.median(mine) * 1e3:.1f} us, "
            f"min {min(mine) * 1e3:.1f} us, max {max(mine) * 1e3:.1f} us")
        say(f"  group_metrics on the same joints, three launches, the same run: median {statistics.median(theirs) * 1e3:.1f} us, "
            f"min {min(theirs) * 1e3:.1f} us, max {max(theirs) * 1e3:.1f} us")
        say(f"  200 calls back to back: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per call, "
            f"{e0.elapsed_time(e1) / 200 * 1e6 / (b * dn * T):.1f} ns per dancer and frame")
        say("  against the float64 restatement: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + "; " +
            ", ".join(f"{k} {'equal' if v else 'DIFFERENT'}" for k, v in same.items()) + " (closest: exact ties of the default radii aside)")
    signal.alarm(0)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
