"""Workload for timing the foot lock (profiles/footlock.txt):

    python tools/footlock_time.py [repeats] [out.txt] [time limit in seconds]

Two workloads a user would run: 16 clips x 3 dancers x 150 frames with the model's contact channels (planted in blocks of 10 frames,
half of them), and one long song of 1 x 3 x 1200 frames without contacts, the planted frames labelled from the motion.  Seeded
synthetic motion (tests/footlock_ref.py ``motion``).  After one warm-up per shape, each repeat times the three launches of
``tck_foot_lock`` with device events; then a window of 50 calls back to back is timed as a whole, which is what a caller in a loop
pays per call.  The kernels one by one are a matter for rocprofv3, not for this tool.  Then the error maxima of the shared test
cases: the largest relative rotation angle against the float64 restatement, and the largest distance of a pinned joint from its
anchor on the float32 poses returned.  Prints one line per measurement and, with a second argument, also writes them there.  The whole
run is ended by an alarm after the time limit (300 s unless given)."""
import os
import signal
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import footlock_ref as R  # noqa: E402
from tcdiff_amd import footlock as F  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS  # noqa: E402

LEG_JOINTS = [1, 4, 7, 2, 5, 8]


def workload(b, dn, T, seed, with_contacts):
    rng = np.random.default_rng(seed)
    speed = None if with_contacts else np.where((np.arange(T) // 9) % 2 == 0, 1.0, 5.0)
    clips = [R.motion(T, seed=seed + c, dn=dn, speed=speed) for c in range(b)]
    q, pos = (np.concatenate([c[i] for c in clips]) for i in range(2))
    contacts = None
    if with_contacts:
        blocks = (rng.random((b, dn, (T + 9) // 10, 4)) > 0.5).astype(np.float32)
        contacts = np.ascontiguousarray(np.repeat(blocks, 10, axis=2)[:, :, :T])
    return q, pos, contacts


def errors(dev):
    """the shared test cases: (largest rotation error in rad, largest pinned-joint distance from the anchor in m)"""
    rot, pin = 0.0, 0.0
    todo = [(R.case(n)[:3], R.case(n)[3], R.case(n)[4]) for n in R.CASES]
    q, pos, ref = R.motion_case()
    todo.append(((q, pos, None), 5, ref))
    for (q, pos, contacts), blend, ref in todo:
        tq, tpos, tc = (None if a is None else torch.from_numpy(np.array(a)).to(dev) for a in (q, pos, contacts))          # copies: the cases are read-only
        out = F.foot_lock(tq, tpos, tc, dn=R.DN, blend=blend)
        got = out.q.cpu().numpy()
        a, b = got.astype(np.float64)[:, :, LEG_JOINTS].reshape(-1, 3), ref["q64"][:, :, LEG_JOINTS].reshape(-1, 3)
        rot = max([rot] + [R.angle_between(x, y) for x, y in zip(a, b)])
        T = q.shape[1] // R.DN
        for d in range(R.DN):
            for leg in range(2):
                for t in range(T):
                    if ref["g"][0, d, leg, t] and ref["status"][0, d, leg, t] != 2:
                        ch = R.chain(got[0, t * R.DN + d], pos[0, t * R.DN + d], leg)
                        at = ch["Pa"] if ref["g"][0, d, leg, t] == 1 else ch["Pe"]
                        pin = max(pin, R.norm(R.sub(at, tuple(ref["anchor"][0, d, leg, t]))))
    return rot, pin


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"footlock_time: not finished after {limit} s"))
    signal.alarm(limit)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = "cuda:0"
    for what, (b, dn, T), with_contacts in (("16 clips x 3 dancers x 150 frames, contacts", (16, 3, 150), True),
                                            ("one long song, 1 x 3 x 1200 frames, labels from the motion", (1, 3, 1200), False)):
        q, pos, contacts = (None if a is None else torch.from_numpy(a).to(dev) for a in workload(b, dn, T, 100, with_contacts))
        ws = torch.empty(K.foot_lock_workspace(b, dn, T), dtype=torch.uint8, device=dev)
        q_out, joints = torch.empty_like(q), torch.empty(b, dn, T, 24, 3, device=dev)
        planted, clamped = (torch.empty(b, dn, 2, dtype=torch.int32, device=dev) for _ in range(2))
        shift = torch.empty(b, dn, 2, dtype=torch.float64, device=dev)

        def call():
            K.foot_lock(q, pos, contacts, b, dn, T, 0.95, 0.01, 5, 1e-3, SMPL_PARENTS, SMPL_OFFSETS, ws, q_out, joints, planted, clamped, shift)
        call()                                                             # the warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            call()
        e1.record()
        torch.cuda.synchronize()
        frames = b * dn * T
        say(f"{what}: workspace {ws.numel() / 2 ** 20:.2f} MiB, planted {int(planted.sum())} of {2 * frames} leg frames, clamped {int(clamped.sum())}, "
            f"largest shift {float(shift.max()):.3f} m")
        say(f"  three launches, device events, {repeats} repeats after one warm-up: median {statistics.median(times) * 1e3:.1f} us, "
            f"min {min(times) * 1e3:.1f} us, max {max(times) * 1e3:.1f} us")
        say(f"  50 calls back to back: {e0.elapsed_time(e1) / 50 * 1e3:.1f} us per call, {e0.elapsed_time(e1) / 50 * 1e6 / frames:.1f} ns per frame")
    rot, pin = errors(dev)
    say(f"shared test cases ({len(R.CASES)} with contacts, 1 labelled from the motion): largest rotation error against the float64 restatement "
        f"{rot:.3e} rad (bound 1e-6), largest distance of a pinned joint from its anchor {pin:.3e} m (bound 2e-6)")
    signal.alarm(0)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
