"""Workload for timing the Motion-JPEG path (profiles/mjpeg.txt):

    python tools/mjpeg_time.py [repeats] [out.txt]

The one-clip workload of tools/draw_time.py: 3 dancers x 150 frames at 480 x 480, the poses exported from the same seeded random
samples.  Each repeat (after one warm-up) times, with device events, the four launches of ``encode_jpeg`` on the clip's frames
(launches 1 - 3 are ``tcj_mjpeg_plan``, launch 4 ``tcj_mjpeg_write``; the kernels of the plan are timed one by one through
rocprofv3 when that is wanted, not here); then, end to end, what ``render_sample(draw_out=...)`` with ``draw_format = "avi"`` does
per clip: draw, encode, copy of the compressed bytes, ``write_avi`` with 5 s of sound.  Prints one line per measurement and, with a
second argument, also writes them there."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcdiff_amd import draw as D  # noqa: E402
from tcdiff_amd import export as E  # noqa: E402
from tcdiff_amd import io as tio  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd import video as V  # noqa: E402


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
    frames = D.draw_dance(poses[:1], contacts[:1])[0]
    sound = 0.5 * np.sin(2 * np.pi * 440 * np.arange(5 * 30720) / 30720.0)
    for quality, subsampling in ((90, "420"), (90, "444"), (75, "420")):
        sub = V.SUBSAMPLING[subsampling]
        workspace = torch.empty(K.mjpeg_workspace(S, H, W, sub), dtype=torch.uint8, device=dev)
        offsets = torch.empty(S + 1, dtype=torch.int64, device=dev)
        say(f"one clip, {S} frames at {W} x {H}, quality {quality}, {subsampling}: frames {frames.numel() / 2 ** 20:.0f} MiB, "
            f"workspace {workspace.numel() / 2 ** 20:.0f} MiB")
        for it in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            K.mjpeg_plan(frames, quality, sub, workspace, offsets)
            ev[1].record()
            total = int(offsets[S].item())
            data = torch.empty(total, dtype=torch.uint8, device=dev)
            ev[2].record()
            K.mjpeg_write(S, H, W, quality, sub, workspace, data)
            ev[3].record()
            torch.cuda.synchronize()
            if it:
                say(f"  repeat {it}: tcj_mjpeg_plan (blocks, count, offsets) {ev[0].elapsed_time(ev[1]):.3f} ms, tcj_mjpeg_write "
                    f"{ev[2].elapsed_time(ev[3]):.3f} ms, {total / 2 ** 20:.2f} MiB of JPEG")
        with tempfile.TemporaryDirectory() as tmp:
            for it in range(2):
                t0 = time.perf_counter()
                one = D.draw_dance(poses[:1], contacts[:1])
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                jpeg = V.encode_jpeg(one[0], quality, subsampling)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                host = jpeg.cpu()
                t3 = time.perf_counter()
                path = V.write_avi(os.path.join(tmp, "clip.avi"), host, fps=30, audio=sound, sample_rate=30720)
                t4 = time.perf_counter()
                if it:
                    say(f"  end to end: draw_dance {(t1 - t0) * 1e3:.2f} ms, encode_jpeg {(t2 - t1) * 1e3:.2f} ms, copy {(t3 - t2) * 1e3:.2f} ms, "
                        f"write_avi {(t4 - t3) * 1e3:.1f} ms, file {os.path.getsize(path) / 2 ** 20:.2f} MiB (of which sound "
                        f"{2 * len(sound) / 2 ** 20:.2f} MiB)")
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
