"""Workload for timing the beat synchroniser (profiles/beatsync.txt):

    python tools/beatsync_time.py [repeats] [out.txt] [time limit in seconds]

The two sizes the other correctors are timed at: 16 clips x 3 dancers x 150 frames, and one long song of 1 x 3 x 1200 frames, the seeded
dance of tests/beatsync_ref.py (``case``: a music beat every 7 frames).  After one warm-up per shape, each repeat times the three
launches of ``tcb_beat_sync`` as a whole with device events (pooled and per-dancer warps), the two of ``tcb_motion_beats``, and in the
same run ``smooth`` and ``foot_lock`` on the same poses for comparison; then a window of 200 calls back to back is timed as a whole,
which is what a caller in a loop pays per call.  The launches one by one are a matter for rocprofv3 (``--kernel-trace --stats``, a run of
its own), not for this tool.
Prints one line per measurement and, with a second argument, also writes them there.  The whole run is ended by an alarm after the
time limit (300 s unless given)."""
import importlib
import os
import signal
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import beatsync_ref as R  # noqa: E402
from tcdiff_amd.footlock import foot_lock  # noqa: E402

B = importlib.import_module("tcdiff_amd.beat_sync")
S = importlib.import_module("tcdiff_amd.smooth")


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


def line(what, t):
    return f"  {what}: median {statistics.median(t) * 1e3:.1f} us, min {min(t) * 1e3:.1f} us, max {max(t) * 1e3:.1f} us"


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"beatsync_time: not finished after {limit} s"))
    signal.alarm(limit)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    for what, (b, dn, T) in (("16 clips x 3 dancers x 150 frames", (16, 3, 150)), ("one long song, 1 x 3 x 1200 frames", (1, 3, 1200))):
        q, pos, contacts, beats = (torch.from_numpy(a.copy()).to(dev) for a in R.case(b, dn, T))
        calls = {"tcb_beat_sync, pooled warps, three launches": lambda: B.beat_sync(q, pos, beats, dn=dn, contacts=contacts, share=True, measure=False),
                 "tcb_beat_sync, a warp per dancer, three launches": lambda: B.beat_sync(q, pos, beats, dn=dn, contacts=contacts, share=False, measure=False),
                 "smooth on the same poses, two launches": lambda: S.smooth(q, pos, dn=dn, measure=False),
                 "foot_lock on the same poses": lambda: foot_lock(q, pos, contacts, dn=dn)}
        out = B.beat_sync(q, pos, beats, dn=dn, contacts=contacts, share=True)
        joints = out.joints
        calls["tcb_motion_beats on joints of the same shape, two launches"] = lambda: B.motion_beats(joints)
        for call in calls.values():                                        # the warm-ups
            call()
        torch.cuda.synchronize()
        say(f"{what}: {b * dn} dancers; pooled: {int(out.music_count.sum())} music beats, {int(out.kin_count.sum())} kinematic, {int(out.matched.sum())} matched, "
            f"{int(out.anchors.sum())} anchors, {int(out.moved.sum())} of {b * dn * T} frames moved; beat_align "
            f"{float(out.before['beat_align'].mean()):.3f} -> {float(out.after['beat_align'].mean()):.3f}")
        for name, call in calls.items():
            say(line(f"{name}, device events, {repeats} repeats after one warm-up (with the Python wrapper's allocations)", timed(call, repeats)))
        for name in list(calls)[:2]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                calls[name]()
            e1.record()
            torch.cuda.synchronize()
            say(f"  200 calls of {name.split(',')[0]} ({name.split(',')[1].strip()}) back to back: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per call")
    signal.alarm(0)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
