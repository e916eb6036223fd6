"""Workload for timing mesh_contact (profiles/meshcontact.txt):

    python tools/meshcontact_time.py [repeats] [out.txt] [time limit in seconds]

A closed synthetic mesh of SMPL's size (tests/meshcontact_ref.py's closed_lattice with nu = nv = 83: V = 6891, F = 13778), posed on
the device as balls of 0.55 m around the dancers' centres, in three workloads a user would run: 16 clips x 3 dancers x 150 frames with
the dancers apart (the boxes are disjoint, so the call should cost about one read of the vertices: the achieved bytes per second are
reported against that), the same clips with dancers that meet now and then, and one song of 3 x 1200 frames of the same motion.  After
one warm-up per case the three launches of ``tcm_mesh_contact`` are timed as a whole with device events; then the heaviest contact
frame of the case (the most inside vertices) is timed alone, as one clip of one frame of its two dancers.  The kernels one by one are
a matter for rocprofv3, not for this tool.  Prints one line per measurement and, with a second argument, also writes them there.  The
whole run is ended by an alarm after the time limit (300 s unless given)."""
import os
import signal
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meshcontact_ref as R  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402


def centres(b, T, dn, gap, pull, dev):
    """(b, T dn, 3): dancers in a row along x, `gap` apart, drawn to the middle by `pull` metres and back every 60 frames, a little
    differently in every clip"""
    c, t, d = torch.meshgrid(torch.arange(b, device=dev), torch.arange(T, device=dev), torch.arange(dn, device=dev), indexing="ij")
    wave = (30 - ((t + 7 * c) % 60 - 30).abs()).double() / 30.0          # 0 .. 1 .. 0
    x = d * gap - (d - (dn - 1) / 2) * pull * wave
    return torch.stack([x, 0.1 * d + 0.0 * x, 1.0 + 0.05 * d + 0.0 * x], -1).reshape(b, T * dn, 3).float()


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"meshcontact_time: not finished after {limit} s"))
    signal.alarm(limit)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = "cuda:0"
    ball, faces = R.closed_lattice(83, 83, 1, (0.0, 0.0, 0.0))
    V, F = ball.shape[0], faces.shape[0]
    ball_d, faces_d = torch.from_numpy(ball).to(dev), torch.from_numpy(faces).to(dev)
    say(f"closed lattice nu = nv = 83: V = {V}, F = {F}")

    def timed(fn):
        fn()                                                  # the warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(times), min(times), max(times)

    def run(x, dn):
        b, rows = x.shape[:2]
        T, P = rows // dn, dn * (dn - 1) // 2
        ws = torch.empty(K.mesh_contact_workspace(b, dn, T, V, F), dtype=torch.uint8, device=dev)
        f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
        i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)
        inside, depth = torch.empty(b, P, T, 2, dtype=torch.int32, device=dev), f64(b, P, T)
        outs = (f64(b, P), i64(b, P), f64(b, P), i64(b, P, 3), f64(b, P))
        return (lambda: K.mesh_contact(x, faces_d, faces, dn, 2, ws, inside, depth, *outs)), inside, depth, outs, ws

    for what, (b, dn, T), gap, pull in (("16 clips x 3 dancers x 150 frames, dancers apart", (16, 3, 150), 1.5, 0.0),
                                        ("16 clips x 3 dancers x 150 frames, dancers that meet now and then", (16, 3, 150), 1.3, 0.4),
                                        ("one long song, 1 x 3 x 1200 frames, dancers that meet now and then", (1, 3, 1200), 1.3, 0.4)):
        x = ball_d[None, None] + centres(b, T, dn, gap, pull, dev)[:, :, None]
        fn, inside, depth, outs, ws = run(x, dn)
        med, lo, hi = timed(fn)
        torch.cuda.synchronize()
        contact = int((inside.sum(-1) > 0).sum())
        nbytes = x.numel() * 4
        say(f"{what}: vertices {nbytes / 2 ** 20:.1f} MiB, workspace {ws.numel() / 2 ** 20:.2f} MiB; contact frames {contact} of "
            f"{inside.shape[0] * inside.shape[1] * T} (pair, frame)s, episodes {int(outs[1].sum())}, deepest {float(outs[2].max()):.4f} m, "
            f"most inside vertices in a frame {int(inside.sum(-1).max())}")
        say(f"  mesh_contact: 3 launches, device events, {repeats} repeats after one warm-up: median {med:.1f} us, min {lo:.1f} us, "
            f"max {hi:.1f} us; one read of the vertices in that time: {nbytes / med / 1e6:.3f} TB/s")
        if contact:
            flat = int(inside.sum(-1).reshape(-1).argmax())
            c, rest = divmod(flat, inside.shape[1] * T)
            p, t = divmod(rest, T)
            a, bb = R.pairs(dn)[p]
            one = torch.stack([x[c, t * dn + a], x[c, t * dn + bb]])[None].contiguous()
            fn1, inside1, _, _, _ = run(one, 2)
            med, lo, hi = timed(fn1)
            say(f"  the heaviest contact frame alone (clip {c}, frame {t}, dancers {a} and {bb}; inside vertices "
                f"{inside1[0, 0, 0].tolist()}): median {med:.1f} us, min {lo:.1f} us, max {hi:.1f} us")
    signal.alarm(0)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
