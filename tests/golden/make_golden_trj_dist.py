"""What the REAL reference does with a `trj_dist` argument (model/model.py:71-97, 326, 332); needs a checkout of the reference
where oracle/refload.py looks for it.

    python tests/golden/make_golden_trj_dist.py

  trj_dist_reference.npz : config-1 shape (1 clip, 2 dancers x 60 frames, T = 100), eval mode, a [1, 120, 120] trj_dist at
     t = 50: `raised` (1 if the forward raised), `error_type` and `error_message` (the exception's class name and text).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import refload  # noqa: E402
from oracle import tcdiff_oracle as O  # noqa: E402


def main():
    ref, _ = refload.build_reference(O.synth_state_dict(dn=2, seq_len=60), dn=2, seq_len=60, n_timestep=100)
    ref.eval()
    raised, etype, msg = 0, "", ""
    try:
        with torch.no_grad():
            ref(torch.stack([O.synth_xT(0, 120)]), torch.stack([O.synth_cond(0, 60)]), torch.tensor([50]), cond_drop_prob=0.0,
                trj_dist=torch.randint(0, 10, (1, 120, 120), generator=torch.Generator().manual_seed(0)))
    except Exception as e:          # noqa: BLE001  (recorded, whatever it is)
        raised, etype, msg = 1, type(e).__name__, str(e)
    print(raised, etype, msg)
    np.savez_compressed(os.path.join(HERE, "trj_dist_reference.npz"), raised=np.array(raised),
                        error_type=np.array(etype), error_message=np.array(msg))


if __name__ == "__main__":
    main()
