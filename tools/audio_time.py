"""Workload for timing the audio front end (profiles/audio.txt):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/audio_time.py [repeats]

Two jobs, each `repeats` times after one warm-up: 16 files x 220500 s16 stereo frames at 44100 Hz (5-second slices as files), and
one 180-second s16 stereo song at 48000 Hz cut with slices=(0.5, 5) into 351 overlapping rows.  Each repeat is one load_audio
call on the parsed files (the upload, audio_decode_kernel, audio_resample_kernel); the trace's audio_* rows are what the profile
records.  Also prints device-event times of the calls and, per job, the resampler's multiply-adds and gathered table bytes."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_ref as R  # noqa: E402
from tcdiff_amd import audio as A  # noqa: E402


def pcm_file(frames, sr, seed):
    pcm = np.random.default_rng(seed).integers(-20000, 20001, (frames, 2), dtype=np.int64)
    return A.read_wav(R.wav_file(R.pack(pcm, "s16"), "s16", 2, sr))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = "cuda:0"
    jobs = {"16 files x 220500 frames, 44100 Hz": ([pcm_file(220500, 44100, s) for s in range(16)], None, 44100, 220500, 16),
            "180 s at 48000 Hz, slices (0.5, 5)": ([pcm_file(180 * 48000, 48000, 99)], (0.5, 5.0), 48000, 240000, 351)}
    for name, (wavs, slices, sr, n, rows) in jobs.items():
        A.resample(torch.zeros(4096, device=dev), sr)     # the table's upload stays out of the warm-up call's time
        times = []
        for it in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            y = A.load_audio(wavs, slices=slices, device=dev)
            ev[1].record()
            torch.cuda.synchronize()
            if it:
                times.append(ev[0].elapsed_time(ev[1]))
        assert y.shape == (rows, R.plan(n, sr)["size"]), y.shape
        ix = R.indices(n, sr)
        taps = int((ix["left"][2] + ix["right"][2]).sum()) * rows
        print(f"{name}: output {tuple(y.shape)}; load_audio with the upload {sorted(round(t, 3) for t in times)} ms, median "
              f"{np.median(times):.3f} ms; resample: {taps} multiply-adds, {8 * taps} gathered table bytes, at most "
              f"{R.max_taps(n, sr)} taps per output", flush=True)


if __name__ == "__main__":
    main()
