"""Workload for timing the chroma columns (profiles/chroma.txt):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/chroma_time.py [repeats]

Two jobs, each `repeats` times after one warm-up: 16 clips x 30 seconds (921600 samples, 1801 frames) and 3 clips x 20617 samples
(41 frames), the test signals of tests/chroma_ref.py.  Each repeat is one chroma_cqt call with the tuning estimated (all four
launches); the trace's chroma_* and music_stft rows are what the profile records.  Also prints device-event times of the calls
and the tuning indices found."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chroma_ref as R  # noqa: E402
from tcdiff_amd import music as MU  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = "cuda:0"
    jobs = {"16 clips x 921600 samples": np.stack([R.make_tones(30 * R.SR, seed=s) for s in range(16)]),
            "3 clips x 20617 samples": np.stack([R.make_tones(512 * 40 + 137, seed=s) for s in (4, 5, 9)])}
    for name, y in jobs.items():
        Y = torch.from_numpy(y).to(dev)
        MU.chroma_cqt(Y[:1, :4096])                       # the tables' upload stays out of the warm-up call's time
        times = []
        for it in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            chroma, parts = MU.chroma_cqt(Y, return_parts=True)
            ev[1].record()
            torch.cuda.synchronize()
            if it:
                times.append(ev[0].elapsed_time(ev[1]))
        print(f"{name}: chroma_cqt {sorted(round(t, 3) for t in times)} ms, median {np.median(times):.3f} ms; tuning indices "
              f"{parts['tuning_index'].tolist()}", flush=True)


if __name__ == "__main__":
    main()
