"""Workload for timing the glTF export (profiles/gltf.txt):

    python tools/gltf_time.py [repeats]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gltf_time.py [repeats]

16 clips x 150 frames x 3 dancers and one clip of 1125 frames x 3 dancers, `repeats` times after one warm-up: `export_poses` (one
pose_export launch, the yardstick) and, on its outputs, `animation_block` (one gltf_animation_kernel), timed with device events;
then the device-to-host copy of the block and `build_glb` per clip on the host's clock.  Also prints the bytes the launch moves."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcdiff_amd import export as E  # noqa: E402
from tcdiff_amd import gltf as X  # noqa: E402
from tcdiff_amd import io as tio  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    dn = 3
    norm = tio.Normalizer(torch.randn(2000, 151, generator=g))
    for b, T in ((16, 150), (1, 1125)):
        x = (torch.rand(b, T * dn, 151, generator=g) * 2 - 1).to(dev)
        for it in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            q, pos, _, _ = E.export_poses(x, norm, "normal", dn)
            ev[1].record()
            block = X.animation_block(q, pos, dn)
            ev[2].record()
            torch.cuda.synchronize()
            if it:
                print(f"{b} x {T} x {dn}: export_poses {ev[0].elapsed_time(ev[1]):.3f} ms, animation_block {ev[1].elapsed_time(ev[2]):.3f} ms",
                      flush=True)
        read, written = (q.numel() + pos.numel()) * 4, block.numel() * 4
        print(f"{b} x {T} x {dn}: the launch reads {read} bytes (each rotation vector twice: {read + q.numel() * 4}) and writes {written}",
              flush=True)
        for it in range(repeats + 1):
            t0 = time.perf_counter()
            host = block.cpu().numpy()
            t1 = time.perf_counter()
            files = [X.build_glb(one, T, dn, 30.0) for one in host]
            t2 = time.perf_counter()
            if it:
                print(f"{b} x {T} x {dn}: copy to the host {1e3 * (t1 - t0):.3f} ms, build_glb {1e3 * (t2 - t1) / b:.3f} ms per clip "
                      f"({len(files[0])} bytes per file)", flush=True)


if __name__ == "__main__":
    main()
