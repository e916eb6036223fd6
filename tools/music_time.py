"""Workload for timing the music front end (profiles/music.txt):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/music_time.py [repeats]

Two jobs, each `repeats` times after one warm-up: 30 five-second slices (153 600 samples each at 30 720 Hz, what render_count
clips of the reference's test set are), and one 60-second song.  Each repeat is one music_features call; the trace's music_*
kernel rows are what the profile records.  Also prints device-event times of the calls, and -- as context, on the same host --
the float32 run time of the numpy / scipy restatement tests/music_ref.py on one slice and on the song."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import music_ref as R  # noqa: E402
from tcdiff_amd import music as MU  # noqa: E402

SR = 30720


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = "cuda:0"
    jobs = {"30 slices x 153600": np.stack([R.make_signal(5 * SR, SR, seed=s) for s in range(30)]),
            "1 song x 1843200": R.make_signal(60 * SR, SR, seed=99)[None]}
    for name, y in jobs.items():
        Y = torch.from_numpy(y).to(dev)
        for it in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            feats = MU.music_features(Y)
            ev[1].record()
            torch.cuda.synchronize()
            if it:
                print(f"{name}: music_features {tuple(feats.shape)} {ev[0].elapsed_time(ev[1]):.3f} ms", flush=True)
        t0 = time.perf_counter()
        R.features(y[0], SR, np.float32)
        print(f"{name}: music_ref float32 on the host, ONE clip of {y.shape[1]} samples: {1e3 * (time.perf_counter() - t0):.0f} ms", flush=True)


if __name__ == "__main__":
    main()
