"""What tests/test_gltf_cpu.py and tests/test_gltf_gpu.py hold tcdiff_amd/gltf.py and csrc/gltf.hip to, written from
include/tcdiff_gltf.h and the glTF 2.0 specification, not from the kernel or from build_glb:

* ``block``: a numpy float64 restatement of the header's animation block, the sign rule a plain loop over the frames;
* ``read_glb`` / ``accessor``: a minimal .glb reader that checks the container and every accessor as it goes;
* ``evaluate``: walks the node tree at every key frame in float64 and returns the joint nodes' world positions;
* ``fk``: float64 forward kinematics of the same rotation vectors through rotation matrices (no quaternion in it);
* ``seeded`` / ``crafted``: the inputs, shared and read-only, each computed once.
"""
import functools
import json
import struct

import numpy as np

FW = 0.7071067811865476               # sqrt(1/2) in float64: the header's f = (-FW, 0, 0, FW)
SMALL = 1e-3
ULP = 2.0 ** -23                      # one float32 ulp at 1: the bound on a quaternion component
MIN_MARGIN = 1e-6                     # no decision of the seeded inputs is nearer a tie than this
PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
GPU_SHAPES = [(1, 1, 1), (1, 2, 1), (2, 63, 2), (1, 64, 3), (1, 65, 1), (3, 150, 3), (1, 1125, 2)]      # (clips, T, dn)
FLIPS_AT = (63, 64, 65, 127, 128)


def floats(T, dn):
    return T * (1 + 99 * dn)


# ---- the header, restated ----------------------------------------------------------------------------------------------------------
def quats(r, root=False):
    """r (..., 3) float32 -> (..., 4) float64 (x, y, z, w); root: f (x) q"""
    assert r.dtype == np.float32
    r = r.astype(np.float64)
    r0, r1, r2 = r[..., 0], r[..., 1], r[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.sqrt((r0 * r0 + r1 * r1) + r2 * r2)
        a2 = theta * theta
        k = np.where(theta < SMALL, (0.5 - a2 / 48.0) + a2 * a2 / 3840.0, np.sin(theta / 2.0) / theta)
        x, y, z, w = k * r0, k * r1, k * r2, np.cos(theta / 2.0)
    if root:
        fw, fx = FW, -FW
        x, y, z, w = fw * x + fx * w, fw * y - fx * z, fw * z + fx * y, fw * w - fx * x
    return np.stack([x, y, z, w], -1)


def block(poses, trans, fps=30.0):
    """poses (clips, T, dn, 24, 3), trans (clips, T, dn, 3) float32 -> (out (clips, F) float32, info): info["flips"] the number of
    sign changes, info["margin"] the smallest |dot| between neighbouring frames and |w_0| (NaN ones left out)"""
    clips, T, dn = poses.shape[:3]
    assert poses.shape == (clips, T, dn, 24, 3) and trans.shape == (clips, T, dn, 3) and trans.dtype == np.float32
    out = np.zeros((clips, floats(T, dn)), np.float32)
    q = np.concatenate([quats(poses[..., :1, :], True), quats(poses[..., 1:, :])], -2)          # (clips, T, dn, 24, 4) float64
    flips, margin = 0, np.inf
    sign = np.ones((clips, T, dn, 24))
    with np.errstate(invalid="ignore"):
        for t in range(T):                                                # the sequential rule, as the header states it
            if t == 0:
                s, deciding = np.where(q[:, 0, :, :, 3] < 0, -1.0, 1.0), q[:, 0, :, :, 3]
            else:
                a, b = q[:, t - 1], q[:, t]
                deciding = ((b[..., 0] * a[..., 0] + b[..., 1] * a[..., 1]) + b[..., 2] * a[..., 2]) + b[..., 3] * a[..., 3]
                flip = deciding < 0
                flips += int(flip.sum())
                s = np.where(flip, -sign[:, t - 1], sign[:, t - 1])
            sign[:, t] = s
            if np.isfinite(deciding).any():
                margin = min(margin, float(np.abs(deciding[np.isfinite(deciding)]).min()))
    q = (sign[..., None] * q).astype(np.float32)
    for c in range(clips):
        out[c, :T] = (np.arange(T, dtype=np.float64) / np.float64(fps)).astype(np.float32)
        for d in range(dn):
            base = T + 99 * T * d
            p = trans[c, :, d]
            out[c, base:base + 3 * T] = np.stack([p[:, 0], p[:, 2], -p[:, 1]], -1).reshape(-1)
            out[c, base + 3 * T:base + 99 * T] = q[c, :, d].transpose(1, 0, 2).reshape(-1)       # [24][T][4]
    return out, {"flips": flips, "margin": margin}


def split(one, T, dn):
    """one clip's F floats -> (times (T,), trans (dn, T, 3), rot (dn, 24, T, 4)) views"""
    per = one[T:].reshape(dn, 99 * T)
    return one[:T], per[:, :3 * T].reshape(dn, T, 3), per[:, 3 * T:].reshape(dn, 24, T, 4)


def compare(got, want, T, dn, what=""):
    """times and trans bit for bit, quaternion components within one float32 ulp at 1, NaN in the same places; prints the error"""
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    worst = 0.0
    for g, w in zip(got.reshape(-1, floats(T, dn)), want.reshape(-1, floats(T, dn))):
        (gt, gp, gq), (wt, wp, wq) = split(g, T, dn), split(w, T, dn)
        assert np.array_equal(gt.view(np.uint32), wt.view(np.uint32)), (what, "times")
        assert np.array_equal(gp.view(np.uint32), wp.view(np.uint32)), (what, "trans")
        assert np.array_equal(np.isnan(gq), np.isnan(wq)), (what, "NaN")
        ok = ~np.isnan(wq)
        if ok.any():
            worst = max(worst, float(np.abs(gq[ok].astype(np.float64) - wq[ok].astype(np.float64)).max()))
    print(f"{what}: largest quaternion component error {worst:.3e} (bound {ULP:.3e})")
    assert worst <= ULP, (what, worst)


# ---- float64 forward kinematics without quaternions ------------------------------------------------------------------------------
def _matrices(r):
    """Rodrigues' formula in float64: r (..., 3) -> (..., 3, 3)"""
    r = r.astype(np.float64)
    theta = np.sqrt((r * r).sum(-1))[..., None, None]
    K = np.zeros(r.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -r[..., 2], r[..., 1], r[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -r[..., 0], -r[..., 1], r[..., 0]
    small = theta < 1e-4
    safe = np.where(small, 1.0, theta)
    a = np.where(small, 1 - theta ** 2 / 6, np.sin(safe) / safe)
    b = np.where(small, 0.5 - theta ** 2 / 24, (1 - np.cos(safe)) / safe ** 2)
    return np.eye(3) + a * K + b * (K @ K)


def fk(poses, trans, offsets, parents=PARENTS):
    """poses (T, dn, 24, 3), trans (T, dn, 3) float32 -> joints (dn, T, 24, 3) float64 in the data's (Z-up) frame"""
    R = _matrices(poses)
    offsets = np.asarray(offsets, np.float64)
    T, dn = poses.shape[:2]
    world, pos = [None] * 24, np.zeros((T, dn, 24, 3))
    for j in range(24):
        p = parents[j]
        if p < 0:
            world[j], pos[:, :, j] = R[:, :, j], trans.astype(np.float64)
        else:
            world[j] = world[p] @ R[:, :, j]
            pos[:, :, j] = pos[:, :, p] + (world[p] @ offsets[j])
    return pos.transpose(1, 0, 2, 3)


def to_y_up(p):
    """(x, y, z) -> (x, z, -y)"""
    return np.stack([p[..., 0], p[..., 2], -p[..., 1]], -1)


# ---- a minimal .glb reader ------------------------------------------------------------------------------------------------------------
_COMPONENT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def read_glb(data: bytes):
    """-> (the JSON object, the BIN chunk's bytes); asserts the container's layout (glTF 2.0, section 'GLB file format')"""
    assert len(data) >= 20 and len(data) % 4 == 0
    magic, version, length = struct.unpack_from("<4sII", data, 0)
    assert magic == b"glTF" and version == 2 and length == len(data)
    n_json, kind = struct.unpack_from("<I4s", data, 12)
    assert kind == b"JSON" and n_json % 4 == 0 and 20 + n_json <= len(data)
    text = data[20:20 + n_json]
    assert text.rstrip(b" ") == text.strip() and not text.startswith(b" ")            # padded with trailing spaces only
    gltf = json.loads(text.decode("ascii"))
    at = 20 + n_json
    n_bin, kind = struct.unpack_from("<I4s", data, at)
    assert kind == b"BIN\0" and n_bin % 4 == 0 and at + 8 + n_bin == len(data)        # one BIN chunk, nothing after it
    binary = data[at + 8:]
    assert gltf["asset"]["version"] == "2.0" and len(gltf["buffers"]) == 1 and "uri" not in gltf["buffers"][0]
    declared = gltf["buffers"][0]["byteLength"]
    assert declared <= n_bin < declared + 4 and binary[declared:] == b"\0" * (n_bin - declared)
    for v in gltf["bufferViews"]:
        assert v["buffer"] == 0 and v["byteOffset"] % 4 == 0 and v["byteLength"] >= 1
        assert v["byteOffset"] + v["byteLength"] <= declared and "byteStride" not in v
    views_of_vertices = [p["attributes"][k] for m in gltf.get("meshes", []) for p in m["primitives"] for k in p["attributes"]]
    inputs = {s["input"] for a in gltf.get("animations", []) for s in a["samplers"]}
    for i, a in enumerate(gltf["accessors"]):
        size = np.dtype(_COMPONENT[a["componentType"]]).itemsize
        v = gltf["bufferViews"][a["bufferView"]]
        assert a["byteOffset"] % 4 == 0 and a["byteOffset"] % size == 0 and (v["byteOffset"] + a["byteOffset"]) % size == 0
        assert a["count"] >= 1 and a["byteOffset"] + a["count"] * size * _WIDTH[a["type"]] <= v["byteLength"], i
        values = accessor(gltf, binary, i)
        needs = i in inputs or any(i == p["attributes"].get("POSITION") for m in gltf.get("meshes", []) for p in m["primitives"])
        assert not needs or ("min" in a and "max" in a), i
        if "min" in a:
            flat = values.reshape(a["count"], -1)
            assert np.array_equal(flat.min(0), np.asarray(a["min"], flat.dtype)), i
            assert np.array_equal(flat.max(0), np.asarray(a["max"], flat.dtype)), i
        if i in views_of_vertices:
            assert (size * _WIDTH[a["type"]]) % 4 == 0                                  # vertex attributes: 4-byte elements
    return gltf, binary


def accessor(gltf, binary, i):
    a = gltf["accessors"][i]
    v = gltf["bufferViews"][a["bufferView"]]
    dt = np.dtype(_COMPONENT[a["componentType"]]).newbyteorder("<")
    w = _WIDTH[a["type"]]
    out = np.frombuffer(binary, dt, a["count"] * w, v["byteOffset"] + a["byteOffset"])
    return out if w == 1 else out.reshape(a["count"], w)


def _rotate(q, v):
    """unit quaternions q (T, 4) as (x, y, z, w) applied to vectors v (T, 3) or (3,), float64"""
    u, w = q[:, :3], q[:, 3:]
    v = np.broadcast_to(v, u.shape)
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def _product(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def evaluate(gltf, binary):
    """-> ({node index: world positions (T, 3) float64} of every node reached from the scene, the key-frame times).  A node's
    local transform is its TRS with the animated values in place of the static ones, the quaternions normalised; no scale."""
    anim, = gltf["animations"]
    times = None
    moved = {}
    for ch in anim["channels"]:
        s = anim["samplers"][ch["sampler"]]
        assert s["interpolation"] == "LINEAR"
        t = accessor(gltf, binary, s["input"])
        assert times is None or times is t or np.array_equal(times, t)
        times = t
        key = (ch["target"]["node"], ch["target"]["path"])
        assert key not in moved and ch["target"]["path"] in ("translation", "rotation")
        moved[key] = accessor(gltf, binary, s["output"]).astype(np.float64)
        assert len(moved[key]) == len(times)
    T = len(times)
    out, seen = {}, set()

    def walk(n, pos, rot):
        assert n not in seen                                                             # a tree: every node has one parent
        seen.add(n)
        node = gltf["nodes"][n]
        assert "matrix" not in node and "scale" not in node
        tr = moved.get((n, "translation"), np.broadcast_to(np.asarray(node.get("translation", [0, 0, 0]), np.float64), (T, 3)))
        q = moved.get((n, "rotation"), np.broadcast_to(np.asarray(node.get("rotation", [0, 0, 0, 1]), np.float64), (T, 4)))
        q = q / np.sqrt((q * q).sum(-1, keepdims=True))
        here = pos + _rotate(rot, tr)
        out[n] = here
        for k in node.get("children", []):
            walk(k, here, _product(rot, q))
    for n in gltf["scenes"][gltf["scene"]]["nodes"]:
        walk(n, np.zeros((T, 3)), np.broadcast_to(np.array([0.0, 0, 0, 1]), (T, 4)))
    return out, times


def joints_of(gltf, world, dn, names):
    """the evaluated joint nodes by name -> (dn, T, 24, 3)"""
    index = {node["name"]: n for n, node in enumerate(gltf["nodes"])}
    return np.stack([np.stack([world[index[f"d{d}_{name}"]] for name in names], 1) for d in range(dn)])


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _wrap(axis, angle):
    """axis (..., 3) unit, angle (...) -> the float32 rotation vector of angle <= pi the pose export would hand over: through a
    quaternion with w >= 0, so a joint that turns through pi jumps to the other side of the sphere"""
    v, w = axis * np.sin(angle / 2)[..., None], np.cos(angle / 2)
    v, w = np.where((w < 0)[..., None], -v, v), np.abs(w)
    n = np.sqrt((v * v).sum(-1))
    return (v / n[..., None] * (2 * np.arctan2(n, w))[..., None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def seeded(clips, T, dn):
    """Smooth random rotations swept through 4 pi every 150 frames and wrapped to angle <= pi, smooth root paths; returns
    (poses (clips, T, dn, 24, 3), trans (clips, T, dn, 3), block, info), read-only.  Asserts that no sign decision of its own
    is a near-tie before anyone compares against it."""
    g = np.random.default_rng(1000 * clips + 10 * T + dn)
    t = np.arange(T, dtype=np.float64).reshape(1, T, 1, 1)
    shape = (clips, 1, dn, 24)
    axis = g.standard_normal(shape + (3,)) + 0.4 * g.standard_normal(shape + (3,)) * np.sin(0.05 * t + g.uniform(0, 6, shape))[..., None]
    axis /= np.sqrt((axis * axis).sum(-1, keepdims=True))
    angle = g.uniform(0, 2 * np.pi, shape) + (4 * np.pi / 149) * t * g.uniform(0.7, 1.0, shape)
    poses = _wrap(axis, angle)
    ts = t[..., 0]
    trans = (g.uniform(-1, 1, (clips, 1, dn, 3)) + 0.3 * np.sin(0.07 * ts[..., None] + g.uniform(0, 6, (clips, 1, dn, 3)))).astype(np.float32)
    out, info = block(poses, trans)
    assert info["margin"] > MIN_MARGIN, info
    for a in (poses, trans, out):
        a.setflags(write=False)
    return poses, trans, out, info


@functools.lru_cache(maxsize=None)
def crafted():
    """One dancer, T = 130, a special case per joint (the rest small seeded rotations); returns (poses (1, T, 1, 24, 3), trans,
    block, what to expect by hand), read-only.
      0  the zero vector at the root: (-sqrt(1/2), 0, 0, sqrt(1/2));   1  the zero vector: (0, 0, 0, 1)
      2  theta = 1e-4;   3  theta straddling 1e-3: 0.999e-3, 1.001e-3 and float32(1e-3) (above 1e-3 as a double) in turn
      4  theta = float32(pi) (above pi: w_0 = -4.4e-8 < 0, the channel is negated)
      5  an unwrapped theta = 4 from frame 0 on: w < 0, every frame negated, no flip
      6  theta = 1 about x, told as 1 or as 1 - 2 pi (the same rotation, q negated), the telling changing at FLIPS_AT only: what
         is stored is one constant quaternion
      7  as 6, with a NaN at frame 50 and the other telling from frame 51 on (neither dot product with the NaN flips, so the sign
         stays and the OTHER quaternion is stored), then back at frame 100 (a flip)"""
    T = 130
    g = np.random.default_rng(7)
    poses = (0.3 * g.standard_normal((1, T, 1, 24, 3))).astype(np.float32)
    trans = g.standard_normal((1, T, 1, 3)).astype(np.float32)
    ch = poses[0, :, 0]                                                       # (T, 24, 3) view
    ch[:, 0] = ch[:, 1] = 0
    unit = np.array([2.0, -1.0, 2.0]) / 3
    ch[:, 2] = (1e-4 * unit).astype(np.float32)
    for t in range(T):
        ch[t, 3] = np.float32((0.999e-3, 1.001e-3, 1e-3)[t % 3]) * np.float32([0, 1, 0])
    ch[:, 4] = np.float32(np.pi) * np.float32([0, 0, 1])
    ch[:, 5] = np.float32(4.0) * np.float32([1, 0, 0])
    told = np.zeros(T, int)
    for f in FLIPS_AT:
        told[f:] ^= 1
    ch[:, 6] = 0
    ch[:, 6, 0] = np.where(told == 1, np.float32(1 - 2 * np.pi), np.float32(1))
    other = np.zeros(T, int)
    other[51:100] = 1
    ch[:, 7] = 0
    ch[:, 7, 0] = np.where(other == 1, np.float32(1 - 2 * np.pi), np.float32(1))
    ch[50, 7, 1] = np.nan
    out, info = block(poses, trans)
    assert info["margin"] > 1e-9, info                                        # joint 4's w_0 = -4.4e-8 is the nearest
    half = np.float32(np.sin(0.5)), np.float32(np.cos(0.5))
    expect = {"root": np.float32([-FW, 0, 0, FW]), "identity": np.float32([0, 0, 0, 1]), "one": np.float32([half[0], 0, 0, half[1]])}
    for a in (poses, trans, out):
        a.setflags(write=False)
    return poses, trans, out, expect


def check_crafted(got):
    """the special cases, checked by hand (not through the restatement): got (1, F) float32"""
    _, _, _, expect = crafted()
    T = 130
    _, _, rot = split(got[0], T, 1)
    rot = rot[0]                                                          # (24, T, 4)
    assert np.array_equal(rot[0], np.tile(expect["root"], (T, 1))) and np.array_equal(rot[1], np.tile(expect["identity"], (T, 1)))
    unit = np.array([2.0, -1.0, 2.0]) / 3
    assert np.abs(rot[2] - np.append(0.5e-4 * unit, 1.0)).max() < 1e-10 + ULP / 2 and (rot[2, :, 3] == 1).all()
    for t in range(T):                                                    # sin(theta / 2) on either side of the series' threshold
        th = np.float64(np.float32((0.999e-3, 1.001e-3, 1e-3)[t % 3]))
        assert abs(rot[3, t, 1] - np.sin(th / 2)) < 3e-11 and rot[3, t, 0] == rot[3, t, 2] == 0 and abs(rot[3, t, 3] - np.cos(th / 2)) < 6e-8
    # float32(pi) is above pi: w_0 < 0, the channel is negated, so z = -sin(theta / 2) = -1 and w = +4.4e-8
    assert (rot[4, :, 2] == -1).all() and (np.abs(rot[4, :, 3] - 4.371139e-8) < 1e-13).all() and (rot[4, :, :2] == 0).all()
    assert np.abs(rot[5] - np.float32([-np.sin(2.0), 0, 0, -np.cos(2.0)])).max() <= ULP      # theta = 4: negated from frame 0 on
    assert np.abs(rot[6] - expect["one"]).max() < 3e-7                    # one constant quaternion through five flips
    assert np.isnan(rot[7, 50]).all() and not np.isnan(np.delete(rot[7], 50, 0)).any()
    assert np.abs(rot[7, :50] - expect["one"]).max() < 3e-7 and np.abs(rot[7, 51:] + expect["one"]).max() < 3e-7
