"""Workload for timing the body skinning (profiles/skin.txt):

    python tools/skin_time.py [repeats]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/skin_time.py [repeats]

A seeded synthetic model of SMPL's size (V = 6890, four weights per vertex; the faces are a fan, skinning does not read them) and
random poses at 16 clips x 150 frames x 3 dancers and one clip of 1125 frames x 3 dancers: `skin` (one skin_pose_kernel, one
skin_vertex_kernel) `repeats` times after one first call, timed with device events, with and without the pose-corrective blend
shapes.  Also prints the bytes the vertex launch moves and the fraction of the fp32 matrix peak (157.3 TF) the product reaches."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcdiff_amd import body as B  # noqa: E402

PEAK = 157.3e12
SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]


def synthetic(V=6890, K=4, seed=0):
    g = np.random.default_rng(seed)
    jr = g.uniform(0, 1, (24, V)) ** 4
    w = np.zeros((V, 24))
    idx = np.argsort(g.uniform(0, 1, (V, 24)), 1)[:, :K]
    val = g.uniform(0.1, 1, (V, K))
    np.put_along_axis(w, idx, val / val.sum(1, keepdims=True), 1)
    kt = np.array([[p if p >= 0 else 2 ** 32 - 1 for p in SMPL_PARENTS], list(range(24))], np.uint32)
    return {"v_template": g.normal(0, 0.4, (V, 3)), "shapedirs": g.normal(0, 0.02, (V, 3, 10)), "posedirs": g.normal(0, 0.01, (V, 3, 207)),
            "J_regressor": jr / jr.sum(1, keepdims=True), "weights": w, "kintree_table": kt,
            "f": np.stack([np.zeros(V - 2, np.int64), np.arange(1, V - 1), np.arange(2, V)], 1)}


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = "cuda:0"
    body = B.load_body_model(synthetic(), device=dev)
    V, K = body.V, body.K
    g = torch.Generator().manual_seed(0)
    for clips, T, dn in ((16, 150, 3), (1, 1125, 3)):
        n = T * dn
        q = (torch.randn(clips, n, 24, 3, generator=g) * 0.5).to(dev)
        p = torch.randn(clips, n, 3, generator=g).to(dev)
        out = torch.empty(clips, n, V, 3, device=dev)
        P = clips * n
        for pose_blend in (True, False):
            for it in range(repeats + 1):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                B.skin(body, q, p, pose_blend=pose_blend, out=out)
                ev[1].record()
                torch.cuda.synchronize()
                print(f"{clips} x {T} x {dn}, pose_blend {pose_blend}: skin {'first call' if not it else 'repeat'} {ev[0].elapsed_time(ev[1]):.3f} ms",
                      flush=True)
        tiles = -(-P // B.POSE_TILE)
        flop = 2.0 * P * 208 * 3 * V
        once = 4 * (P * 208 + P * 288 + 207 * 3 * V + 3 * V + 2 * V * K)
        print(f"{clips} x {T} x {dn}: P = {P} poses, {tiles} pose tiles x {-(-V // B.VERT_TILE)} vertex tiles; the product is {flop / 1e9:.1f} GFLOP "
              f"({1e3 * flop / PEAK:.3f} ms at {PEAK / 1e12:.1f} TF); the vertex launch writes {4 * P * V * 3} bytes, reads {once} bytes if every "
              f"operand is read once and requests {4 * tiles * 207 * 3 * V} bytes of blend (its rows once per pose tile)", flush=True)


if __name__ == "__main__":
    main()
