"""Workload for timing the stick-figure frames (profiles/draw.txt):

    python tools/draw_time.py [repeats] [out.txt]

30 clips x 3 dancers x 150 frames at 480 x 480, the poses exported from seeded random samples.  Each repeat (after one warm-up)
times, with device events, the two launches of ``draw_dance`` on all 30 clips at once; then the copy of the frames to the host;
then, for ONE clip of 150 frames, what ``render_sample(draw_out=...)`` does per clip: draw, copy, ``write_apng`` (zlib, host).
Prints one line per measurement and, with a second argument, also writes them there."""
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcdiff_amd import draw as D  # noqa: E402
from tcdiff_amd import export as E  # noqa: E402
from tcdiff_amd import io as tio  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd.fk import SMPL_PARENTS  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    dn, S, b, W, H = 3, 150, 30, 480, 480
    norm = tio.Normalizer(torch.randn(2000, 151, generator=g))
    x = (torch.rand(b, S * dn, 151, generator=g) * 2 - 1).to(dev)
    _, _, poses, contacts = E.export_poses(x, norm, "normal", dn)
    view = D.camera(W, H)
    segs = torch.from_numpy(D.floor_grid(view)).to(dev)
    pal = torch.tensor(D.PALETTE, dtype=torch.uint8, device=dev)
    style = D.make_style()
    pts = torch.empty(b, S, dn, 24, 3, device=dev)
    trail = torch.empty(b, S, dn, 2, device=dev)
    order = torch.empty(b, S, dn, dtype=torch.int32, device=dev)
    planted = torch.empty(b, S, dn, 4, dtype=torch.uint8, device=dev)
    frames = torch.empty(b, S, H, W, 3, dtype=torch.uint8, device=dev)
    say(f"{b} clips x {dn} dancers x {S} frames at {W} x {H}: frames {frames.numel() / 2 ** 20:.0f} MiB")
    for it in range(repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        K.draw_project(poses, contacts, view.reshape(-1).tolist(), 0.0, 2, 0.95, 0.01, pts, trail, order, planted)
        ev[1].record()
        K.draw_raster(pts, trail, order, planted, b, dn, S, W, H, SMPL_PARENTS, segs, segs.shape[0], pal, pal.shape[0], style, frames)
        ev[2].record()
        torch.cuda.synchronize()
        if it:
            say(f"repeat {it}: tcdiff_draw_project {ev[0].elapsed_time(ev[1]):.3f} ms, tcdiff_draw_raster {ev[1].elapsed_time(ev[2]):.3f} ms")
    assert torch.equal(frames, D.draw_dance(poses, contacts))
    t0 = time.perf_counter()
    host = frames.cpu()
    say(f"copy of all {b} clips to the host (pageable): {(time.perf_counter() - t0) * 1e3:.1f} ms")
    del host
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(2):
            t0 = time.perf_counter()
            one = D.draw_dance(poses[:1], contacts[:1])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            h = one[0].cpu()
            t2 = time.perf_counter()
            path = D.write_apng(os.path.join(tmp, "clip.png"), h)
            t3 = time.perf_counter()
            if it:
                say(f"one clip ({S} frames): draw_dance {(t1 - t0) * 1e3:.2f} ms, copy {(t2 - t1) * 1e3:.2f} ms, "
                    f"write_apng (zlib level 6, one host thread) {(t3 - t2) * 1e3:.0f} ms, file {os.path.getsize(path) / 2 ** 20:.2f} MiB")
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
