"""Workload for timing the beat tracker (profiles/beat.txt):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/beat_time.py [repeats]

Two jobs, each `repeats` times after one warm-up: 16 clips x 1800 frames (30-second slices at 60 frames / s, clicks every 25 - 40
frames) and 3 clips x 451 frames.  Each repeat is one beat_track call with the tempo estimated (both launches); the trace's
beat_* kernel rows are what the profile records.  Also prints device-event times of the calls and the beats found."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import beat_ref as R  # noqa: E402
from tcdiff_amd import music as MU  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = "cuda:0"
    jobs = {"16 clips x 1800 frames": np.stack([R.make_envelope(1800, 25 + s, seed=s) for s in range(16)]),
            "3 clips x 451 frames": np.stack([R.make_envelope(451, 27 + 3 * s, seed=s) for s in range(3)])}
    for name, o in jobs.items():
        O = torch.from_numpy(o).to(dev)
        times = []
        for it in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            tempo, beat, parts = MU.beat_track(O, return_parts=True)
            ev[1].record()
            torch.cuda.synchronize()
            if it:
                times.append(ev[0].elapsed_time(ev[1]))
        print(f"{name}: beat_track {sorted(round(t, 3) for t in times)} ms, median {np.median(times):.3f} ms; periods "
              f"{parts['period'].tolist()}, beats {parts['n_beats'].tolist()}", flush=True)


if __name__ == "__main__":
    main()
