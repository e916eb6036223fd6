"""Workload for timing the motion metrics next to the pose export they follow (profiles/metrics.txt):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/metrics_time.py [repeats]

Two jobs, each `repeats` times after one warm-up: 30 clips x 3 dancers x 150 frames in "normal" mode, and one 2325-frame song
(30 half-overlapping windows of 150 frames) in "long" mode.  Each repeat is export_poses, beats_from_cond, motion_metrics;
the trace's pose_export_kernel / metrics_frame_kernel / metrics_sequence_kernel rows are what the profile records.  Also
prints device-event times of the two calls."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcdiff_amd import export as E  # noqa: E402
from tcdiff_amd import io as tio  # noqa: E402
from tcdiff_amd import metrics as M  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    dn, S, b = 3, 150, 30
    norm = tio.Normalizer(torch.randn(2000, 151, generator=g))
    x = (torch.rand(b, S * dn, 151, generator=g) * 2 - 1).to(dev)
    cond = torch.rand(b, 2 * S + 1, 438, generator=g)
    cond[..., 53] = (torch.rand(b, 2 * S + 1, generator=g) < 0.07).float()
    cond = cond.to(dev)
    for mode in ("normal", "long"):
        for it in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            _, _, poses, contacts = E.export_poses(x, norm, mode, dn)
            ev[1].record()
            beats = M.beats_from_cond(cond, poses.shape[2], long=mode == "long")
            res = M.motion_metrics(poses, contacts, beats)
            ev[2].record()
            torch.cuda.synchronize()
            if it:
                print(f"{mode} {tuple(poses.shape[:3])}: export_poses {ev[0].elapsed_time(ev[1]):.3f} ms, "
                      f"beats_from_cond + motion_metrics {ev[1].elapsed_time(ev[2]):.3f} ms", flush=True)
        print(mode, {k: round(v, 6) for k, v in M.summarize(res).items()}, flush=True)


if __name__ == "__main__":
    main()
