"""Workload for timing the geometric features (profiles/geometric.txt):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/geometric_time.py [repeats]

A reference set of 1024 clips x 3 dancers x 150 frames and a single clip of 3 dancers, `repeats` times after one warm-up:
`geometric_features` (one geometric_features_kernel) and, on the same joints, `kinetic_features` (one kinetic_features_kernel) for
comparison.  Also prints device-event times of the calls and the bytes of joints each launch reads."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcdiff_amd import export as E  # noqa: E402
from tcdiff_amd import io as tio  # noqa: E402
from tcdiff_amd import set_metrics as S  # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    dn, T = 3, 150
    norm = tio.Normalizer(torch.randn(2000, 151, generator=g))
    for b in (1024, 1):
        x = (torch.rand(b, T * dn, 151, generator=g) * 2 - 1).to(dev)
        _, _, joints, _ = E.export_poses(x, norm, "normal", dn)           # stands in for a data set's ground-truth joints
        for it in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            geo = S.geometric_features(joints)
            ev[1].record()
            kin = S.kinetic_features(joints)
            ev[2].record()
            torch.cuda.synchronize()
            if it:
                print(f"{b} x {dn} x {T} ({joints.numel() * 4} bytes of joints): geometric_features {ev[0].elapsed_time(ev[1]):.3f} ms, "
                      f"kinetic_features {ev[1].elapsed_time(ev[2]):.3f} ms", flush=True)
        print("mean of the geometric features:", [round(v, 3) for v in geo.mean((0, 1)).tolist()], flush=True)
        assert bool(torch.isfinite(kin).all())


if __name__ == "__main__":
    main()
