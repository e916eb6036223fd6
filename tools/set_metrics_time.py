"""Workload for timing the set-level metrics (profiles/set_metrics.txt):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/set_metrics_time.py [repeats]

512 clips x 3 dancers x 150 frames, `repeats` times after one warm-up: `reference_from_joints` of a set of joints (one
kinetic_features_kernel, set_moments_kernel, set_pairs_kernel) and `evaluate_set` of as many samples against it (pose_export_kernel,
then the same three and set_fid_kernel).  Also prints device-event times of the two calls and the scores."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcdiff_amd import export as E  # noqa: E402
from tcdiff_amd import io as tio  # noqa: E402
from tcdiff_amd import metrics as M  # noqa: E402
from tcdiff_amd import set_metrics as S  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    dn, T, b = 3, 150, 512
    norm = tio.Normalizer(torch.randn(2000, 151, generator=g))
    real = (torch.rand(b, T * dn, 151, generator=g) * 2 - 1).to(dev)
    x = (torch.rand(b, T * dn, 151, generator=g) * 1.8 - 0.9).to(dev)
    _, _, joints, _ = E.export_poses(real, norm, "normal", dn)            # stands in for a data set's ground-truth joints
    for it in range(repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        ref = S.reference_from_joints(joints)
        ev[1].record()
        res = S.evaluate_set(x, norm, dn, ref)
        ev[2].record()
        torch.cuda.synchronize()
        if it:
            print(f"{b} x {dn} x {T}: reference_from_joints {ev[0].elapsed_time(ev[1]):.3f} ms, "
                  f"evaluate_set (with export_poses) {ev[1].elapsed_time(ev[2]):.3f} ms", flush=True)
    print({k: round(v, 6) for k, v in M.summarize(res).items()}, flush=True)


if __name__ == "__main__":
    main()
