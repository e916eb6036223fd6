"""Generated dances as animated glTF 2.0 binary files (.glb), the open counterpart of the reference's ``Blender_Visulization/``
(pickles split by dancer, then FBX through Autodesk's SDK and an SMPL template .fbx): one self-contained file per clip with all
its dancers, which Blender, three.js, Godot and the web viewers open as they are.

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)
    write_glb(["clip0.glb", "clip1.glb"], q, pos, dn)                         # one launch, one copy, host packing per clip

The numbers of a file -- key-frame times, the root's translation and rotation turned from the data's Z-up to Y-up, every joint's
local rotation as a quaternion whose sign is continuous in time -- are made on the device in one launch (``tcx_gltf_animation``,
csrc/gltf.hip; defined in include/tcdiff_gltf.h) as one block per clip, and that block IS the head of the file's binary chunk:
``build_glb`` only writes the JSON that points into it and appends the static data (a stick body of one octahedron per bone,
rigidly skinned -- or, with ``mesh=`` a ``BodyModel`` (tcdiff_amd/body.py: the user's own SMPL model file, none is shipped), the
model's surface as a skinned mesh).  Not built: shipping a model, FBX, per-frame normals, the pose-corrective blend shapes inside
the file and more than four weights per vertex (core glTF has neither), one body shape per dancer, audio (glTF has none), key-frame
reduction, cameras and lights.  Parity with the Khronos validator and with Blender's importer is unpinned: neither is
a dependency, conformance rests on the glTF 2.0 specification as the tests' reader restates it.
"""
from __future__ import annotations

import json
import os
import pickle
import struct
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .draw import PALETTE
from .export import _is_long, fk_out_names
from .fk import SMPL_OFFSETS, SMPL_PARENTS

# the joints' names in the reference's FBX template (Blender_Visulization/src/SmplObject.py), restated as data
JOINT_NAMES = ("m_avg_Pelvis", "m_avg_L_Hip", "m_avg_R_Hip", "m_avg_Spine1", "m_avg_L_Knee", "m_avg_R_Knee", "m_avg_Spine2",
               "m_avg_L_Ankle", "m_avg_R_Ankle", "m_avg_Spine3", "m_avg_L_Foot", "m_avg_R_Foot", "m_avg_Neck", "m_avg_L_Collar",
               "m_avg_R_Collar", "m_avg_Head", "m_avg_L_Shoulder", "m_avg_R_Shoulder", "m_avg_L_Elbow", "m_avg_R_Elbow",
               "m_avg_L_Wrist", "m_avg_R_Wrist", "m_avg_L_Hand", "m_avg_R_Hand")
BONE_RADIUS = 0.12            # the octahedron's half-width as a fraction of the bone's length ...
BONE_RADIUS_MAX = 0.03        # ... capped, in metres
BONE_WAIST = 0.2              # where along the bone its widest ring sits

_FLOAT, _UBYTE, _USHORT, _UINT = 5126, 5121, 5123, 5125     # glTF componentType
_ARRAY_BUFFER, _ELEMENT_ARRAY_BUFFER = 34962, 34963   # glTF bufferView.target


def block_floats(T: int, dn: int) -> int:
    """TC_GLTF_FLOATS(T, dn): the floats of one clip's block"""
    return T * (1 + 99 * dn)


def animation_block(smpl_poses, smpl_trans, dn, fps=30.0) -> torch.Tensor:
    """smpl_poses (clips, T * dn, 24, 3) and smpl_trans (clips, T * dn, 3) as ``export_poses`` returns them (row = frame * dn +
    dancer), or the pickles' (T * dn, 72) and (T * dn, 3) as one clip; float32 on the device.  Returns the (clips, F) float32
    block of include/tcdiff_gltf.h, F = T (1 + 99 dn), on the device: one launch, no synchronisation."""
    if not isinstance(smpl_poses, torch.Tensor) or not isinstance(smpl_trans, torch.Tensor):
        raise L.TcdiffError("animation_block: smpl_poses and smpl_trans must be tensors")
    if smpl_poses.dim() == 2 and smpl_poses.shape[-1] == 72:          # the pickles' layout: one clip
        smpl_poses, smpl_trans = smpl_poses.reshape(1, -1, 24, 3), smpl_trans.unsqueeze(0) if smpl_trans.dim() == 2 else smpl_trans
    if smpl_poses.dim() != 4 or tuple(smpl_poses.shape[2:]) != (24, 3):
        raise L.TcdiffError(f"animation_block: smpl_poses must be (clips, frames * dancers, 24, 3) or (frames * dancers, 72), "
                            f"got {tuple(smpl_poses.shape)}")
    clips, n = smpl_poses.shape[:2]
    if tuple(smpl_trans.shape) != (clips, n, 3):
        raise L.TcdiffError(f"animation_block: smpl_trans must be ({clips}, {n}, 3) beside these poses, got {tuple(smpl_trans.shape)}")
    dn = int(dn)
    if dn < 1 or clips < 1 or n < 1 or n % dn:
        raise L.TcdiffError(f"animation_block: {clips} clip(s) of {n} rows are not a whole number of frames of {dn} dancers")
    fps = float(fps)
    if not (0 < fps < float("inf")):
        raise L.TcdiffError(f"animation_block: fps must be positive and finite, got {fps!r}")
    if not smpl_poses.is_cuda or not smpl_trans.is_cuda:
        raise L.TcdiffError("animation_block runs on MI355X only (no CPU fallback)")
    if smpl_trans.device != smpl_poses.device:
        raise L.TcdiffError("animation_block: smpl_poses and smpl_trans must be on one device")
    T = n // dn
    if clips * block_floats(T, dn) > 2 ** 31 - 1:
        raise L.TcdiffError(f"animation_block: {clips} x {T} frames x {dn} dancers is more than 2^31 - 1 floats of output")
    q = smpl_poses.detach().float().contiguous()
    p = smpl_trans.detach().float().contiguous()
    with torch.cuda.device(q.device):
        out = torch.empty(clips, block_floats(T, dn), dtype=torch.float32, device=q.device)
        K.gltf_animation(q, p, clips, T, dn, fps, out)
    return out


def _srgb_to_linear(v) -> float:
    c = float(v) / 255.0
    return c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4


def _rest(parents, offsets) -> np.ndarray:
    """rest positions of the 24 joints in float64: the root at the origin (its node carries no static translation)"""
    rest = np.zeros((24, 3), np.float64)
    for j in range(24):
        if parents[j] >= 0:
            if parents[j] >= j:
                raise L.TcdiffError("build_glb: a joint's parent must come before it")
            rest[j] = rest[parents[j]] + offsets[j]
    return rest


def _bones(parents, rest):
    """One flat-shaded elongated octahedron per bone, from the parent's rest position to the child's, rigidly skinned to the
    parent: (positions (V, 3) f32, normals (V, 3) f32, joints (V, 4) u8, weights (V, 4) f32, indices (V,) u16) with unshared
    vertices, three per face, counter-clockwise seen from outside.  A bone of no length has no solid."""
    pos, nrm, jnt = [], [], []
    for j in range(24):
        p = parents[j]
        if p < 0:
            continue
        a, b = rest[p], rest[j]
        axis = b - a
        length = float(np.linalg.norm(axis))
        if not length > 1e-9:
            continue
        axis = axis / length
        side = np.zeros(3)
        side[int(np.argmin(np.abs(axis)))] = 1.0                      # the world axis the bone is least along
        u = np.cross(axis, side)
        u /= np.linalg.norm(u)
        v = np.cross(axis, u)
        r = min(BONE_RADIUS * length, BONE_RADIUS_MAX)
        mid = a + BONE_WAIST * (b - a)
        ring = [mid + r * u, mid + r * v, mid - r * u, mid - r * v]
        centre = (a + b) / 2
        for tip in (a, b):
            for k in range(4):
                tri = [tip, ring[k], ring[(k + 1) % 4]]
                n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
                if n @ (sum(tri) / 3 - centre) < 0:                   # turn the face so that its normal points outwards
                    tri[1], tri[2] = tri[2], tri[1]
                    n = -n
                n = n / np.linalg.norm(n)
                pos.extend(tri)
                nrm.extend([n, n, n])
                jnt.extend([p, p, p])
    V = len(pos)
    joints = np.zeros((V, 4), np.uint8)
    joints[:, 0] = jnt
    weights = np.zeros((V, 4), np.float32)
    weights[:, 0] = 1.0
    return (np.asarray(pos, np.float32).reshape(V, 3), np.asarray(nrm, np.float32).reshape(V, 3), joints, weights,
            np.arange(V, dtype=np.uint16))


def _surface(mesh):
    """A ``BodyModel``'s surface as glTF vertex data: (positions = v_shaped (V, 3) f32, the rest normals (V, 3) f32, joints (V, 4)
    u8, weights (V, 4) f32, indices (3F,) u16 or, above 65 535 vertices, u32).  Normals: the faces' area-weighted normals (the
    cross products as they are) summed per vertex in float64 and normalised; a vertex whose sum is zero gets (0, 1, 0).  Joints and
    weights: each vertex's four largest weights, ties to the lower joint, renormalised to sum to 1 in float64."""
    V, faces = mesh.V, mesh.faces
    p = mesh.v_shaped
    n = np.zeros((V, 3), np.float64)
    fn = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    for c in range(3):
        np.add.at(n, faces[:, c], fn)
    length = np.sqrt((n * n).sum(1))
    flat = ~(length > 0)
    n[~flat] /= length[~flat, None]
    n[flat] = (0.0, 1.0, 0.0)
    w = mesh.weights
    top = np.argsort(-w, axis=1, kind="stable")[:, :4]                    # stable: among equal weights the lower joint first
    wt = np.take_along_axis(w, top, 1)
    wt = wt / wt.sum(1, keepdims=True)
    top = np.where(wt != 0, top, 0)
    return (p.astype(np.float32), n.astype(np.float32), top.astype(np.uint8), wt.astype(np.float32),
            faces.reshape(-1).astype(np.uint16 if V <= 65535 else np.uint32))


def build_glb(block, T, dn, fps, *, parents=None, offsets=None, colors=PALETTE, body=True, mesh=None) -> bytes:
    """One clip's block (F = T (1 + 99 dn) float32, a numpy array as ``animation_block(...)[i].cpu().numpy()`` gives it) -> the
    bytes of a .glb file.  Pure host code: the 12-byte header, a JSON chunk, one BIN chunk that is the block as it is followed by
    the static data.

    Scene: per dancer d 24 joint nodes ``d{d}_{name}`` (JOINT_NAMES), children by ``parents``, static ``translation`` =
    ``offsets[j]`` (joint 0 has none: its translation is animated); one animation with, per dancer, a ``translation`` channel on
    joint 0 and 24 ``rotation`` channels, LINEAR, all on one time accessor whose min / max are read from the block.  ``body``:
    a skin per dancer and a mesh of one octahedron per bone in the dancer's colour (``colors[d % n]``, sRGB 0..255) -- without
    it a viewer has nothing to shade, only the armature.  ``fps`` is what the block was made with; it names the animation.

    ``mesh``: a ``BodyModel`` (``load_body_model``).  The dancers' meshes are then the model's surface instead of the octahedra:
    POSITION ``v_shaped``, NORMAL the rest normals, JOINTS_0 / WEIGHTS_0 each vertex's four largest weights renormalised, inverse
    bind matrices that translate by -J_j, and the skeleton is the MODEL's (its parents, its offsets as the nodes' translations):
    an explicit ``parents`` or ``offsets`` beside ``mesh`` raises, the body would bind at one skeleton and move on another.  The
    file's vertices are ``skin(..., pose_blend=False, origin="pelvis")`` turned to Y-up, with the four kept weights: the
    pose-corrective blend shapes and weights beyond four cannot be expressed in core glTF."""
    T, dn = int(T), int(dn)
    if mesh is not None:
        if parents is not None or offsets is not None:
            raise L.TcdiffError("build_glb: mesh= brings the model's own skeleton; parents= or offsets= beside it would move the body on "
                                "a skeleton it is not bound to")
        if not body:
            raise L.TcdiffError("build_glb: mesh= beside body=False")
        if not all(hasattr(mesh, k) for k in ("v_shaped", "faces", "weights", "J", "offsets", "parents")):
            raise L.TcdiffError("build_glb: mesh must be what load_body_model returns")
        parents, offsets = mesh.parents, mesh.offsets
    parents = [int(p) for p in (SMPL_PARENTS if parents is None else parents)]
    offsets = np.asarray(SMPL_OFFSETS if offsets is None else offsets, np.float64)
    if T < 1 or dn < 1:
        raise L.TcdiffError(f"build_glb: T and dn must be >= 1, got {T}, {dn}")
    if len(parents) != 24 or offsets.shape != (24, 3) or not np.isfinite(offsets).all():
        raise L.TcdiffError("build_glb: the skeleton is 24 parents and 24 x 3 finite offsets")
    block = np.ascontiguousarray(np.asarray(block), dtype="<f4").reshape(-1)
    F = block_floats(T, dn)
    if block.size != F:
        raise L.TcdiffError(f"build_glb: the block of {T} frames of {dn} dancers holds {F} floats, got {block.size}")
    if not np.isfinite(block).all():
        raise L.TcdiffError("build_glb: the block holds a non-finite value (a NaN or infinite pose)")
    rest = _rest(parents, offsets)

    views, accessors, chunks = [], [], [block.tobytes()]
    size = [4 * F]

    def view(data: bytes, target=None) -> int:
        v = {"buffer": 0, "byteOffset": size[0], "byteLength": len(data)}
        if target is not None:
            v["target"] = target
        views.append(v)
        pad = -len(data) % 4
        chunks.append(data + b"\0" * pad)
        size[0] += len(data) + pad
        return len(views) - 1

    def accessor(bv, offset, ctype, count, kind, **extra) -> int:
        accessors.append({"bufferView": bv, "byteOffset": offset, "componentType": ctype, "count": count, "type": kind, **extra})
        return len(accessors) - 1

    views.append({"buffer": 0, "byteOffset": 0, "byteLength": 4 * F})                 # view 0: the device-made block
    times = accessor(0, 0, _FLOAT, T, "SCALAR", min=[float(block[0])], max=[float(block[T - 1])])
    nodes, samplers, channels, roots = [], [], [], []
    for d in range(dn):
        base = T + 99 * T * d
        for j in range(24):
            node = {"name": f"d{d}_{JOINT_NAMES[j]}"}
            kids = [24 * d + k for k in range(24) if parents[k] == j]
            if kids:
                node["children"] = kids
            if j:
                node["translation"] = [float(x) for x in offsets[j]]
            nodes.append(node)
            if parents[j] < 0:
                roots.append(24 * d + j)
        out = accessor(0, 4 * base, _FLOAT, T, "VEC3")
        samplers.append({"input": times, "output": out, "interpolation": "LINEAR"})
        channels.append({"sampler": len(samplers) - 1, "target": {"node": 24 * d, "path": "translation"}})
        for j in range(24):
            out = accessor(0, 4 * (base + 3 * T + 4 * T * j), _FLOAT, T, "VEC4")
            samplers.append({"input": times, "output": out, "interpolation": "LINEAR"})
            channels.append({"sampler": len(samplers) - 1, "target": {"node": 24 * d + j, "path": "rotation"}})
    gltf = {"asset": {"version": "2.0", "generator": "tcdiff_amd"}, "scene": 0}

    if mesh is not None:
        pos, nrm, jnt, wgt, idx = _surface(mesh)
    else:
        pos, nrm, jnt, wgt, idx = _bones(parents, rest) if body else (np.zeros((0, 3), np.float32),) * 5
    if len(pos):
        ibm = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (24, 1))             # column-major: the translation is 12 .. 14
        ibm[:, 12:15] = -rest if mesh is None else -mesh.J          # POSITION is in the model's frame: the pelvis at J_0
        a_ibm = accessor(view(ibm.astype("<f4").tobytes()), 0, _FLOAT, 24, "MAT4")
        attributes = {
            "POSITION": accessor(view(pos.astype("<f4").tobytes(), _ARRAY_BUFFER), 0, _FLOAT, len(pos), "VEC3",
                                 min=[float(x) for x in pos.min(0)], max=[float(x) for x in pos.max(0)]),
            "NORMAL": accessor(view(nrm.astype("<f4").tobytes(), _ARRAY_BUFFER), 0, _FLOAT, len(pos), "VEC3"),
            "JOINTS_0": accessor(view(jnt.tobytes(), _ARRAY_BUFFER), 0, _UBYTE, len(pos), "VEC4"),
            "WEIGHTS_0": accessor(view(wgt.astype("<f4").tobytes(), _ARRAY_BUFFER), 0, _FLOAT, len(pos), "VEC4")}
        wide = idx.dtype == np.uint32
        a_idx = accessor(view(idx.astype("<u4" if wide else "<u2").tobytes(), _ELEMENT_ARRAY_BUFFER), 0, _UINT if wide else _USHORT,
                         len(idx), "SCALAR")
        colors = np.asarray(colors, np.float64)
        if colors.ndim != 2 or colors.shape[0] < 1 or colors.shape[1] != 3 or (colors < 0).any() or (colors > 255).any():
            raise L.TcdiffError("build_glb: colors must be (n >= 1, 3) values in 0..255")
        gltf["materials"], gltf["meshes"], gltf["skins"] = [], [], []
        for d in range(dn):
            rgb = [_srgb_to_linear(v) for v in colors[d % len(colors)]]
            gltf["materials"].append({"name": f"d{d}", "pbrMetallicRoughness": {"baseColorFactor": rgb + [1.0], "metallicFactor": 0.0,
                                                                                 "roughnessFactor": 0.8}})
            gltf["meshes"].append({"name": f"d{d}_bones" if mesh is None else f"d{d}_surface",
                                   "primitives": [{"attributes": attributes, "indices": a_idx, "material": d, "mode": 4}]})
            gltf["skins"].append({"name": f"d{d}", "joints": list(range(24 * d, 24 * d + 24)), "inverseBindMatrices": a_ibm,
                                  "skeleton": 24 * d})
            nodes.append({"name": f"d{d}_body", "mesh": d, "skin": d})
            roots.append(len(nodes) - 1)
    gltf["scenes"] = [{"nodes": roots}]
    gltf["nodes"] = nodes
    gltf["animations"] = [{"name": f"dance_{float(fps):g}fps", "samplers": samplers, "channels": channels}]
    gltf["accessors"], gltf["bufferViews"] = accessors, views
    gltf["buffers"] = [{"byteLength": size[0]}]

    text = json.dumps(gltf, separators=(",", ":"), allow_nan=False).encode("ascii")
    text += b" " * (-len(text) % 4)
    binary = b"".join(chunks)
    total = 12 + 8 + len(text) + 8 + len(binary)
    if total > 0xFFFFFFFF:
        raise L.TcdiffError("build_glb: a .glb file holds at most 2^32 - 1 bytes")
    return b"".join([struct.pack("<4sII", b"glTF", 2, total), struct.pack("<I4s", len(text), b"JSON"), text,
                     struct.pack("<I4s", len(binary), b"BIN\0"), binary])


def write_glb(path, smpl_poses, smpl_trans, dn, *, fps=30.0, mesh=None, **kw) -> list:
    """``animation_block`` once for all clips, one device-to-host copy, then ``build_glb`` per clip.  ``path``: one path per clip
    (fewer paths: only the first clips are written), or a single path for a single clip.  ``mesh`` (a ``BodyModel``: the dancers'
    surfaces instead of the stick bodies) and ``kw`` go to ``build_glb``.  Returns the paths written."""
    if mesh is not None:
        kw["mesh"] = mesh
    single = isinstance(path, (str, os.PathLike))
    paths = [path] if single else list(path)
    block = animation_block(smpl_poses, smpl_trans, dn, fps)
    if len(paths) > block.shape[0] or (single and block.shape[0] != 1):
        raise L.TcdiffError(f"write_glb: {'a single path' if single else str(len(paths)) + ' paths'} for {block.shape[0]} clip(s)")
    dn = int(dn)
    T = block.shape[1] // (1 + 99 * dn)
    host = block[:len(paths)].cpu().numpy()
    written = []
    for p, one in zip(paths, host):
        p = os.fspath(p)
        with open(p, "wb") as f:
            f.write(build_glb(one, T, dn, fps, **kw))
        written.append(p)
    return written


def glb_out_names(mode: str, epoch, name) -> list:
    """The file names ``render_sample`` writes under ``glb_out``: ``export.fk_out_names``' with .glb in place of .pkl"""
    if name is None:
        raise L.TcdiffError("render_sample: glb_out needs the clips' names")
    return [os.path.splitext(n)[0] + ".glb" for n in fk_out_names(mode, epoch, name)]


def write_glb_out(glb_out, mode: str, epoch, name, q, pos, dn, *, fps=30.0, mesh=None, **kw) -> list:
    """Writes ``export_poses``' first two results as .glb files, one per clip with all its dancers (the first min(b, len(name))
    clips, as the reference's zip), or one per song in "long" mode.  Returns the paths written."""
    names = glb_out_names(mode, epoch, name)
    Path(glb_out).mkdir(parents=True, exist_ok=True)
    n = 1 if _is_long(mode) else min(len(names), q.shape[0])
    if n < 1:
        return []
    return write_glb([os.path.join(glb_out, f) for f in names[:n]], q[:n], pos[:n], dn, fps=fps, mesh=mesh, **kw)


def convert_fk_out(pkl_path, glb_path=None, fps=30.0, mesh=None, **kw) -> str:
    """A pickle that ``write_fk_out`` (or the reference) wrote earlier -> a .glb file beside it (or at ``glb_path``): what the
    reference's 1-preProcess_group_smpl.py and 2-ConvertPkl2FBX_SMPL.py do together.  The number of dancers is
    ``full_pose.shape[0]``."""
    with open(pkl_path, "rb") as f:
        data = pickle.load(f)
    try:
        poses, trans, dn = np.asarray(data["smpl_poses"]), np.asarray(data["smpl_trans"]), int(np.shape(data["full_pose"])[0])
    except (KeyError, TypeError, IndexError) as e:
        raise L.TcdiffError(f"convert_fk_out: {pkl_path} holds no smpl_poses, smpl_trans and full_pose") from e
    if poses.ndim != 2 or poses.shape[1] != 72 or trans.shape != (poses.shape[0], 3) or dn < 1 or poses.shape[0] < 1 or \
            poses.shape[0] % dn:
        raise L.TcdiffError(f"convert_fk_out: smpl_poses {poses.shape} and smpl_trans {trans.shape} are not (frames * {dn}, 72) and "
                            f"(frames * {dn}, 3)")
    dev = "cuda" if torch.cuda.is_available() else "cpu"              # off the GPU animation_block raises: no CPU fallback
    q = torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(dev)
    p = torch.from_numpy(np.ascontiguousarray(trans, np.float32)).to(dev)
    out = os.path.splitext(os.fspath(pkl_path))[0] + ".glb" if glb_path is None else os.fspath(glb_path)
    return write_glb(out, q, p, dn, fps=fps, mesh=mesh, **kw)[0]
