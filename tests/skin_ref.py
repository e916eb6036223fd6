"""What tests/test_skin_cpu.py and tests/test_skin_gpu.py hold tcdiff_amd/body.py, csrc/skin.hip and build_glb(mesh=) to, written
from include/tcdiff_skin.h and the glTF 2.0 specification, not from the kernel or from tcdiff_amd:

* ``make_model``: a seeded synthetic SMPL-shaped model (nothing of a real model file is in this repository);
* ``images``: the header's "prepared once on the host in float64, rounded to float32 once" arrays of a model;
* ``pose_part``: launch 1 in float64, operation by operation as the header orders them (sin and cos from the C library);
* ``vertices``: launch 2 from those, once in float64 all the way (the truth) and once with the per-vertex part in float32 on the
  rounded feat and A (whose distance from the truth is the measure of what float32 can do, the GPU tests' bound is 32 times it);
* ``top_four``: the weights a core-glTF skin can hold;  ``skinned``: a float64 evaluator of a skinned mesh read from a .glb.
"""
import functools
import math

import numpy as np

from gltf_ref import accessor

SMALL = 1e-3
SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
_sin, _cos = np.vectorize(math.sin, otypes=[np.float64]), np.vectorize(math.cos, otypes=[np.float64])


# ---- a synthetic model ------------------------------------------------------------------------------------------------------------------
def make_model(V, K, B=4, seed=0, smpl_tree=False):
    """Random template of metre size, small shapedirs / posedirs, J_regressor rows that are convex weights, exactly K nonzero
    skinning weights per vertex summing to 1, a random valid tree (parent < child) or SMPL's, a triangle fan for faces."""
    g = np.random.default_rng(seed)
    jr = g.uniform(0.0, 1.0, (24, V)) ** 4
    jr /= jr.sum(1, keepdims=True)
    w = np.zeros((V, 24))
    for v in range(V):
        idx = g.choice(24, K, replace=False)
        val = g.uniform(0.1, 1.0, K)
        w[v, idx] = val / val.sum()
    parents = list(SMPL_PARENTS) if smpl_tree else [-1] + [int(g.integers(0, j)) for j in range(1, 24)]
    kt = np.zeros((2, 24), np.uint32)
    kt[0] = [p if p >= 0 else 2 ** 32 - 1 for p in parents]               # the root's entry as the official files have it
    kt[1] = np.arange(24)
    if V >= 3:
        f = np.stack([np.zeros(V - 2, np.int64), np.arange(1, V - 1), np.arange(2, V)], 1)
    else:
        f = np.array([[0, V - 1, V - 1]], np.int64)
    return {"v_template": g.normal(0.0, 0.4, (V, 3)), "shapedirs": g.normal(0.0, 0.02, (V, 3, B)),
            "posedirs": g.normal(0.0, 0.01, (V, 3, 207)), "J_regressor": jr, "weights": w, "kintree_table": kt, "f": f.astype(np.uint32)}


def images(model, betas=None, weights=None):
    """the header's model arrays: float64 on the host, each rounded to float32 once; ``weights``: dense (V, 24) in place of the model's"""
    vt, sd = np.asarray(model["v_template"], np.float64), np.asarray(model["shapedirs"], np.float64)
    V = vt.shape[0]
    b = np.zeros(sd.shape[2])
    if betas is not None:
        b[:len(betas)] = betas
    v_shaped = vt + sd @ b
    J = np.asarray(model["J_regressor"], np.float64) @ v_shaped
    parents = [int(p) if p < 24 else -1 for p in np.asarray(model["kintree_table"])[0].astype(np.int64)]
    offsets = np.zeros((24, 3))
    for j in range(24):
        if parents[j] >= 0:
            offsets[j] = J[j] - J[parents[j]]
    w = np.asarray(model["weights"] if weights is None else weights, np.float64)
    K = int((w != 0).sum(1).max())
    wv, wj = np.zeros((V, K)), np.zeros((V, K), np.int64)
    for v in range(V):
        nz = np.flatnonzero(w[v])
        wv[v, :len(nz)], wj[v, :len(nz)] = w[v, nz], nz
    blend = np.zeros((207, 3 * V))
    pd = np.asarray(model["posedirs"], np.float64)
    for k in range(207):
        blend[k] = pd[:, :, k].reshape(-1)                                # blend[k][3v + c] = posedirs[v][c][k]
    f32 = lambda a: a.astype(np.float32)
    return {"V": V, "K": K, "parents": parents, "v_shaped": f32(v_shaped), "blend": f32(blend), "J": f32(J), "offsets": f32(offsets),
            "wv": f32(wv), "wj": wj, "v_shaped64": v_shaped, "J64": J, "offsets64": offsets}


# ---- launch 1 ------------------------------------------------------------------------------------------------------------------------------
def rodrigues(r):
    """r (..., 3) float32 -> R (..., 3, 3) float64, the header's expressions in the header's order"""
    assert r.dtype == np.float32
    r = r.astype(np.float64)
    r0, r1, r2 = r[..., 0], r[..., 1], r[..., 2]
    x00, x11, x22 = r0 * r0, r1 * r1, r2 * r2
    theta = np.sqrt((x00 + x11) + x22)
    t2 = theta * theta
    with np.errstate(invalid="ignore", divide="ignore"):
        small = theta < SMALL
        safe = np.where(small, 1.0, theta)
        a = np.where(small, (1.0 - t2 / 6.0) + t2 * t2 / 120.0, _sin(safe) / safe)
        b = np.where(small, (0.5 - t2 / 24.0) + t2 * t2 / 720.0, (1.0 - _cos(safe)) / np.where(small, 1.0, t2))
    x01, x02, x12 = r0 * r1, r0 * r2, r1 * r2
    a0, a1, a2 = a * r0, a * r1, a * r2
    R = np.empty(r.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1.0 - b * (x11 + x22), b * x01 - a2, b * x02 + a1
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = b * x01 + a2, 1.0 - b * (x00 + x22), b * x12 - a0
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = b * x02 - a1, b * x12 + a0, 1.0 - b * (x00 + x11)
    return R


def pose_part(im, poses, trans, origin="pelvis"):
    """poses (P, 24, 3), trans (P, 3) float32 -> float64 (feat (P, 208), A (P, 24, 12), joints (P, 24, 3), shift (P, 3)), unrounded"""
    assert poses.dtype == np.float32 and trans.dtype == np.float32 and poses.shape[1:] == (24, 3)
    P = poses.shape[0]
    R = rodrigues(poses)
    J, off, parents = im["J"].astype(np.float64), im["offsets"].astype(np.float64), im["parents"]
    feat = np.zeros((P, 208))
    feat[:, :207] = (R[:, 1:] - np.eye(3)).reshape(P, 207)
    GR, Gt = np.zeros((P, 24, 3, 3)), np.zeros((P, 24, 3))
    for j in range(24):
        p = parents[j]
        if p < 0:
            GR[:, j], Gt[:, j] = R[:, j], J[j]
            continue
        assert p < j
        for a in range(3):
            for b in range(3):
                GR[:, j, a, b] = (GR[:, p, a, 0] * R[:, j, 0, b] + GR[:, p, a, 1] * R[:, j, 1, b]) + GR[:, p, a, 2] * R[:, j, 2, b]
            Gt[:, j, a] = ((GR[:, p, a, 0] * off[j, 0] + GR[:, p, a, 1] * off[j, 1]) + GR[:, p, a, 2] * off[j, 2]) + Gt[:, p, a]
    A = np.zeros((P, 24, 3, 4))
    A[..., :3] = GR
    for a in range(3):
        A[:, :, a, 3] = Gt[:, :, a] - ((GR[:, :, a, 0] * J[:, 0] + GR[:, :, a, 1] * J[:, 1]) + GR[:, :, a, 2] * J[:, 2])
    root = parents.index(-1)
    shift = trans.astype(np.float64) - J[root] if origin == "pelvis" else trans.astype(np.float64)
    assert origin in ("pelvis", "smpl")
    return feat, A.reshape(P, 24, 12), Gt + shift[:, None], shift


# ---- launch 2 ------------------------------------------------------------------------------------------------------------------------------
def vertices(im, poses, trans, pose_blend=True, origin="pelvis", dtype=np.float64):
    """-> (vertices (P, V, 3), joints (P, 24, 3)).  float64: everything in float64 from the float32 inputs, nothing rounded on the
    way.  float32: feat, A and the shift rounded once as launch 1 stores them, then every product and sum of launch 2 in float32,
    the sums in ascending index from zero (numpy rounds the product and the sum separately; the kernel fuses them)."""
    feat, A, joints, shift = pose_part(im, poses, trans, origin)
    t = dtype
    feat, A, shift = feat.astype(np.float32).astype(t) if t is np.float32 else feat, A.astype(np.float32).astype(t) if t is np.float32 else A, \
        shift.astype(np.float32).astype(t) if t is np.float32 else shift
    P, V, K = poses.shape[0], im["V"], im["K"]
    d = np.zeros((P, 3 * V), t)
    if pose_blend:
        blend = im["blend"].astype(t)
        for k in range(207):
            d = d + feat[:, k:k + 1] * blend[k][None]
    vp = im["v_shaped"].astype(t)[None] + d.reshape(P, V, 3)
    T = np.zeros((P, V, 12), t)
    for s in range(K):
        T = T + im["wv"][:, s].astype(t)[None, :, None] * A[:, im["wj"][:, s]]
    T = T.reshape(P, V, 3, 4)
    out = np.zeros((P, V, 3), t)
    for c in range(3):
        out = out + T[..., c] * vp[:, :, c:c + 1]
    out = (out + T[..., 3]) + shift[:, None]
    assert out.dtype == t
    return out, joints


def bound(im, poses, trans, pose_blend, origin):
    """-> (truth float64, the float32 restatement's own largest error, the bound the GPU tests use: 32 times that, at least one
    float32 ulp of the largest coordinate)"""
    truth, _ = vertices(im, poses, trans, pose_blend, origin, np.float64)
    low, _ = vertices(im, poses, trans, pose_blend, origin, np.float32)
    own = float(np.abs(low.astype(np.float64) - truth).max())
    ulp = float(np.spacing(np.float32(np.abs(truth).max())))
    return truth, own, max(32.0 * own, ulp)


def top_four(w):
    """dense weights (V, 24) -> the dense weights a core-glTF skin holds: each vertex's four largest (ties: the lower joint),
    renormalised to sum to 1; and the mass that was dropped per vertex"""
    out, dropped = np.zeros_like(w), np.zeros(len(w))
    for v in range(len(w)):
        order = sorted(range(24), key=lambda j: (-w[v, j], j))[:4]
        kept = sum(w[v, j] for j in order)
        dropped[v] = w[v].sum() - kept
        for j in order:
            out[v, j] = w[v, j] / kept
    return out, dropped


def to_y_up(p):
    return np.stack([p[..., 0], p[..., 2], -p[..., 1]], -1)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def poses_of(P, seed=0):
    """P seeded poses: rotations up to about 2 rad about random axes, translations of metre size; read-only float32"""
    g = np.random.default_rng(100 + 7 * P + seed)
    axis = g.standard_normal((P, 24, 3))
    axis /= np.sqrt((axis * axis).sum(-1, keepdims=True))
    poses = (axis * g.uniform(0.0, 2.0, (P, 24, 1))).astype(np.float32)
    trans = g.uniform(-2.0, 2.0, (P, 3)).astype(np.float32)
    poses.setflags(write=False)
    trans.setflags(write=False)
    return poses, trans


# ---- a skinned mesh read from a .glb -----------------------------------------------------------------------------------------------------
def _matrix(q):
    """unit quaternions (T, 4) as (x, y, z, w) -> (T, 3, 3)"""
    x, y, z, w = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def skinned(gltf, binary):
    """-> [per node with a mesh and a skin, in node order, its vertices (T, V, 3) float64 at every key frame].  glTF 2.0, section
    'Skins': a vertex is sum_i w_i (world(joint_i) . inverseBind_i) [POSITION; 1]; the transform of the node that carries the mesh
    is ignored.  Nodes' local transforms are their TRS with the animated values in place of the static ones."""
    anim, = gltf["animations"]
    moved, T = {}, None
    for ch in anim["channels"]:
        s = anim["samplers"][ch["sampler"]]
        moved[(ch["target"]["node"], ch["target"]["path"])] = accessor(gltf, binary, s["output"]).astype(np.float64)
        T = len(accessor(gltf, binary, s["input"]))
    world = {}

    def walk(n, WR, Wt):
        node = gltf["nodes"][n]
        assert "matrix" not in node and "scale" not in node and n not in world
        tr = moved.get((n, "translation"), np.broadcast_to(np.asarray(node.get("translation", [0, 0, 0]), np.float64), (T, 3)))
        q = moved.get((n, "rotation"), np.broadcast_to(np.asarray(node.get("rotation", [0, 0, 0, 1]), np.float64), (T, 4)))
        q = q / np.sqrt((q * q).sum(-1, keepdims=True))
        here_t = Wt + np.einsum("tab,tb->ta", WR, tr)
        here_R = WR @ _matrix(q)
        world[n] = (here_R, here_t)
        for k in node.get("children", []):
            walk(k, here_R, here_t)
    for n in gltf["scenes"][gltf["scene"]]["nodes"]:
        walk(n, np.broadcast_to(np.eye(3), (T, 3, 3)), np.zeros((T, 3)))
    out = []
    for node in gltf["nodes"]:
        if "mesh" not in node or "skin" not in node:
            continue
        skin = gltf["skins"][node["skin"]]
        prim, = gltf["meshes"][node["mesh"]]["primitives"]
        at = {k: accessor(gltf, binary, v) for k, v in prim["attributes"].items()}
        pos, jn, wt = at["POSITION"].astype(np.float64), at["JOINTS_0"].astype(np.int64), at["WEIGHTS_0"].astype(np.float64)
        ibm = accessor(gltf, binary, skin["inverseBindMatrices"]).astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)   # column-major
        verts = np.zeros((T, len(pos), 3))
        for i in range(4):
            for v in range(len(pos)):
                j = jn[v, i]
                WR, Wt = world[skin["joints"][j]]
                bound_v = ibm[j, :3, :3] @ pos[v] + ibm[j, :3, 3]
                verts[:, v] += wt[v, i] * (WR @ bound_v + Wt)
        out.append(verts)
    return out
