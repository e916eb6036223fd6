"""The dancers' bodies: a user-supplied SMPL model skinned on the GPU.

    body = load_body_model("SMPL_NEUTRAL.npz")                     # the user's file, under the user's licence; none is shipped
    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)
    vertices = skin(body, q, pos)                                  # (clips, frames * dn, V, 3) float32 on the device, Z-up
    write_glb(paths, q, pos, dn, mesh=body)                        # the same surface as a skinned mesh inside the .glb

``skin`` is two launches on the current stream (``tcs_skin_vertices``, csrc/skin.hip; defined in include/tcdiff_skin.h): one
thread per pose builds the pose feature and the joints' transforms in float64, then the hot path adds the pose-corrective blend
shapes (a [poses x 208] x [208 x 3V] product on v_mfma_f32_32x32x2_f32) and blends the transforms per vertex, float32, one store.
No synchronisation, no host copy, no CPU fallback.  Parity with smplx and with the official model files is unpinned: neither is a
dependency; the definitions restate Loper et al. 2015 as smplx evaluates it and the tests hold the kernels to that restatement on
seeded synthetic models.  Per-frame normals and shaded frames of the vertices: tcdiff_amd/shade.py.  Not built: shipping a model,
one body shape per dancer.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import pickle
from collections.abc import Mapping

import numpy as np
import torch

from . import _lib as L
from . import kernels as K

KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "kintree_table", "f")
POSE_TILE = L.SKIN.constants["TC_SKIN_POSE_TILE"]
VERT_TILE = L.SKIN.constants["TC_SKIN_VERT_TILE"]
_FEAT = L.SKIN.constants["TC_SKIN_FEAT"]
_ORIGINS = {"pelvis": L.SKIN.constants["TC_SKIN_ORIGIN_PELVIS"], "smpl": L.SKIN.constants["TC_SKIN_ORIGIN_SMPL"]}
_LIMIT = 2 ** 31 - 1
K_MAX = 8


# ---- reading the user's file ---------------------------------------------------------------------------------------------------------
class _Unreadable:
    """Stands in for an object of a class the unpickler will not import (chumpy's, for one): it swallows whatever state the pickle
    hands it and remembers where it came from."""
    _origin = "?"

    def __new__(cls, *a, **k):
        return object.__new__(cls)

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        pass

    def __call__(self, *a, **k):
        return self

    def append(self, *a):
        pass

    def extend(self, *a):
        pass

    def __setitem__(self, *a):
        pass


_SAFE_BUILTINS = {"dict", "list", "tuple", "set", "frozenset", "int", "float", "complex", "str", "bytes", "bytearray", "slice", "range",
                  "object", "bool"}
_SAFE_MODULES = {"numpy", "scipy", "collections", "copyreg", "copy_reg", "_codecs"}


class _ModelUnpickler(pickle.Unpickler):
    """Classes of numpy, scipy (if installed) and a few plain builtins are loaded; every other class becomes an ``_Unreadable``.
    Nothing is imported in the hope that it exists."""

    def find_class(self, module, name):
        top = module.split(".")[0]
        if top in ("builtins", "__builtin__"):
            if name in _SAFE_BUILTINS:
                return super().find_class(module, name)
        elif top in _SAFE_MODULES and importlib.util.find_spec("copyreg" if top == "copy_reg" else top) is not None:
            return super().find_class(module, name)
        return type("_Unreadable", (_Unreadable,), {"_origin": f"{module}.{name}"})


def _read(source) -> dict:
    if isinstance(source, Mapping):
        return dict(source)
    path = os.fspath(source)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npz":
        with np.load(path, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    if ext == ".pkl":
        with open(path, "rb") as f:
            data = _ModelUnpickler(f, encoding="latin1").load()
        if not isinstance(data, Mapping):
            raise L.TcdiffError(f"load_body_model: {path} does not hold a mapping of arrays")
        return dict(data)
    raise L.TcdiffError(f"load_body_model: {path!r} is neither a .npz nor a .pkl file (nor a mapping of arrays)")


def _array(data, key, dtype=np.float64) -> np.ndarray:
    if key not in data:
        raise L.TcdiffError(f"load_body_model: the model has no {key!r} (it needs {', '.join(KEYS)})")
    v = data[key]
    if isinstance(v, _Unreadable):
        raise L.TcdiffError(f"load_body_model: {key!r} is a {v._origin} object, which cannot be read without that package; convert "
                            "the model to a .npz file of plain arrays where the package is installed "
                            "(numpy.savez(path, **{k: numpy.array(v) for k, v in model.items()})) and load that")
    if hasattr(v, "toarray") and not isinstance(v, np.ndarray):           # a scipy sparse matrix
        v = v.toarray()
    try:
        a = np.asarray(v)
        if a.dtype == object:
            raise TypeError("an array of objects")
        a = np.ascontiguousarray(a, dtype)                                # one layout whatever the source's: one order of every sum
    except (TypeError, ValueError) as e:
        raise L.TcdiffError(f"load_body_model: {key!r} is not an array of numbers ({e})") from e
    if dtype is np.float64 and not np.isfinite(a).all():
        raise L.TcdiffError(f"load_body_model: {key!r} holds a value that is not finite")
    return a


def _integers(a, key) -> np.ndarray:
    """whole numbers as int64; values that do not fit (the official files' root parent is 2^32 - 1) are kept out of range"""
    if a.dtype.kind == "f":
        if not np.isfinite(a).all() or (a != np.floor(a)).any():
            raise L.TcdiffError(f"load_body_model: {key!r} must hold whole numbers")
        a = np.clip(a, -1.0, 2.0 ** 31)
    elif a.dtype.kind == "u":
        a = np.minimum(a, 2 ** 31)
    elif a.dtype.kind != "i":
        raise L.TcdiffError(f"load_body_model: {key!r} must hold whole numbers, not {a.dtype}")
    return a.astype(np.int64)


def faces_closed(faces) -> bool:
    """(F, 3) whole numbers >= 0 -> True iff every directed edge of the faces occurs once and its reverse once (an edge from a
    vertex to itself never does)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tail, head = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    if (tail == head).any():
        return False
    n = int(f.max()) + 1
    edges, counts = np.unique(tail * n + head, return_counts=True)
    if (counts != 1).any():
        return False
    return bool(np.array_equal(edges, np.unique(head * n + tail)))


class BodyModel:
    """What ``load_body_model`` returns: the float64 host arrays (``build_glb`` reads them) and, per device, the float32 images
    the kernels read, made on first use.

    ``V``, ``K`` (the largest number of nonzero weights of a vertex), ``parents`` (list, the root's -1), ``faces`` (F, 3) int64,
    ``betas``, ``v_shaped`` (V, 3), ``J`` (24, 3), ``offsets`` (24, 3), ``blend`` (207, 3V), ``weights`` (V, 24) dense,
    ``weight_values`` / ``weight_joints`` (V, K) in ascending joint order, padded with weight 0 on joint 0."""

    def __init__(self, v_shaped, J, offsets, parents, blend, weights, weight_values, weight_joints, faces, betas):
        self.v_shaped, self.J, self.offsets, self.parents, self.blend = v_shaped, J, offsets, parents, blend
        self.weights, self.weight_values, self.weight_joints, self.faces, self.betas = weights, weight_values, weight_joints, faces, betas
        self.V, self.K = int(v_shaped.shape[0]), int(weight_values.shape[1])
        self._parents_c = (C.c_int * 24)(*parents)
        self._images = {}
        self._adjacency = None
        self._closed = None
        for a in (v_shaped, J, offsets, blend, weights, weight_values, weight_joints, faces, betas):
            a.setflags(write=False)

    def adjacency(self):
        """The vertex-to-face adjacency in CSR form, ``(start int32 (V + 1,), faces int32 (3F,))``: vertex v is named by the faces
        ``faces[start[v]:start[v + 1]]``, in ascending face index (a face that names v twice is listed twice; a vertex that no face
        names has an empty range).  Built once with numpy and cached; what ``tcr_mesh_vertices`` sums a vertex normal over."""
        if self._adjacency is None:
            flat = self.faces.reshape(-1)
            order = np.argsort(flat, kind="stable")                       # stable: ascending face index under each vertex
            start = np.zeros(self.V + 1, np.int32)
            start[1:] = np.cumsum(np.bincount(flat, minlength=self.V))
            listed = (order // 3).astype(np.int32)
            start.setflags(write=False)
            listed.setflags(write=False)
            self._adjacency = (start, listed)
        return self._adjacency

    def closed(self) -> bool:
        """Is the mesh a closed, consistently wound surface: does every directed edge (i -> j of a face) occur exactly once, and its
        reverse exactly once?  On the host with numpy, once, cached; what ``mesh_contact`` asks before it counts rays."""
        if self._closed is None:
            self._closed = faces_closed(self.faces)
        return self._closed

    def images(self, device) -> dict:
        """the float32 device images, each float64 array rounded once: v_shaped, blend, J, offsets, weights (V, K), joints (V, K) int32;
        and the mesh as the shading kernels read it: faces (F, 3), adj_start (V + 1,), adj_faces (3F,), int32"""
        device = torch.device(device)
        if device.type != "cuda":
            raise L.TcdiffError("BodyModel: the device images live on MI355X only (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._images:
            def up(a, dtype):
                return torch.from_numpy(np.array(a, dtype, order="C")).to(device)
            self._images[device] = {"v_shaped": up(self.v_shaped, np.float32), "blend": up(self.blend, np.float32),
                                    "J": up(self.J, np.float32), "offsets": up(self.offsets, np.float32),
                                    "weights": up(self.weight_values, np.float32), "joints": up(self.weight_joints, np.int32),
                                    "faces": up(self.faces, np.int32), "adj_start": up(self.adjacency()[0], np.int32),
                                    "adj_faces": up(self.adjacency()[1], np.int32)}
        return self._images[device]


def load_body_model(source, betas=None, device=None) -> BodyModel:
    """``source``: a mapping of arrays, a .npz path or a .pkl path with the SMPL model's arrays -- ``v_template`` (V, 3),
    ``shapedirs`` (V, 3, B), ``posedirs`` (V, 3, 207), ``J_regressor`` (24, V) (dense or a scipy sparse matrix), ``weights``
    (V, 24), ``kintree_table`` (2, 24) (row 0 the parents, the root's any value outside 0..23), ``f`` (F, 3).  A .pkl member of a
    class whose package is not installed (the official files hold chumpy objects) raises and names the key: convert the file to
    .npz where the package is.  Nothing is downloaded and no package is imported on the chance that it exists.

    ``betas``: up to B shape coefficients (zeros by default); one body shape for all dancers.  Every shape is checked, every
    value must be finite, faces must index below V, a vertex must have 1..8 nonzero weights, a joint's parent must come before
    it.  ``device``: where to put the float32 images now; "cpu" (or no GPU) leaves them to the first ``skin``."""
    data = _read(source)
    vt = _array(data, "v_template")
    if vt.ndim != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
        raise L.TcdiffError(f"load_body_model: 'v_template' must be (V >= 1, 3), got {vt.shape}")
    V = vt.shape[0]
    sd = _array(data, "shapedirs")
    if sd.ndim != 3 or sd.shape[:2] != (V, 3):
        raise L.TcdiffError(f"load_body_model: 'shapedirs' must be ({V}, 3, B), got {sd.shape}")
    B = sd.shape[2]
    pd = _array(data, "posedirs")
    if pd.shape != (V, 3, 207):
        raise L.TcdiffError(f"load_body_model: 'posedirs' must be ({V}, 3, 207), got {pd.shape}")
    jr = _array(data, "J_regressor")
    if jr.shape != (24, V):
        raise L.TcdiffError(f"load_body_model: 'J_regressor' must be (24, {V}), got {jr.shape}")
    w = _array(data, "weights")
    if w.shape != (V, 24):
        raise L.TcdiffError(f"load_body_model: 'weights' must be ({V}, 24), got {w.shape}")
    kt = _array(data, "kintree_table", None)
    if kt.shape != (2, 24):
        raise L.TcdiffError(f"load_body_model: 'kintree_table' must be (2, 24), got {kt.shape}")
    row = _integers(kt[0], "kintree_table")
    parents = [int(p) if 0 <= int(p) < 24 else -1 for p in row]
    if parents.count(-1) != 1:
        raise L.TcdiffError(f"load_body_model: 'kintree_table' must name exactly one root (a parent outside 0..23), got {parents.count(-1)}")
    for j, p in enumerate(parents):
        if p >= j:
            raise L.TcdiffError(f"load_body_model: 'kintree_table' gives joint {j} the parent {p}: a parent must come before its child "
                                "(a cycle, or joints out of order)")
    faces = _array(data, "f", None)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise L.TcdiffError(f"load_body_model: 'f' must be (F >= 1, 3), got {faces.shape}")
    faces = _integers(faces, "f")
    if faces.min() < 0 or faces.max() >= V:
        raise L.TcdiffError(f"load_body_model: 'f' indexes vertex {int(faces.max() if faces.max() >= V else faces.min())} of {V}")
    count = (w != 0).sum(1)
    if count.min() < 1 or count.max() > K_MAX:
        v = int(np.argmax((count < 1) | (count > K_MAX)))
        raise L.TcdiffError(f"load_body_model: 'weights' gives vertex {v} {int(count[v])} nonzero weights; 1..{K_MAX} are supported")
    b = np.zeros(B, np.float64)
    if betas is not None:
        given = np.asarray(betas, np.float64).reshape(-1)
        if given.size > B or not np.isfinite(given).all():
            raise L.TcdiffError(f"load_body_model: betas must be at most {B} finite numbers, got {given.size}")
        b[:given.size] = given
    v_shaped = vt + sd @ b
    J = jr @ v_shaped
    offsets = np.zeros((24, 3), np.float64)
    for j, p in enumerate(parents):
        if p >= 0:
            offsets[j] = J[j] - J[p]
    blend = np.ascontiguousarray(pd.reshape(3 * V, 207).T)                # blend[k][3v + c] = posedirs[v][c][k]
    Kw = int(count.max())
    wv, wj = np.zeros((V, Kw), np.float64), np.zeros((V, Kw), np.int32)
    for v in range(V):                                                    # ascending joint order, padded with weight 0 on joint 0
        nz = np.flatnonzero(w[v])
        wv[v, :nz.size], wj[v, :nz.size] = w[v, nz], nz
    body = BodyModel(np.ascontiguousarray(v_shaped), J, offsets, parents, blend, w.copy(), wv, wj, np.ascontiguousarray(faces), b)
    if device is not None and torch.device(device).type == "cuda":
        body.images(device)
    return body


# ---- skinning ---------------------------------------------------------------------------------------------------------------------------
def skin(body, smpl_poses, smpl_trans, *, pose_blend=True, origin="pelvis", return_joints=False, out=None):
    """smpl_poses (clips, n, 24, 3) and smpl_trans (clips, n, 3) as ``export_poses`` returns them, or the pickles' (n, 72) and
    (n, 3) as one clip; float32 on the device.  Returns the vertices (clips, n, V, 3) float32 on the device in the data's frame
    (Z-up), and with ``return_joints`` the posed joints (clips, n, 24, 3) too.

    ``origin="pelvis"`` puts the pelvis at ``smpl_trans``, as ``export_poses``' joints and the .glb's root node place it;
    ``"smpl"`` adds ``smpl_trans`` to the model's own frame, SMPL's convention.  ``pose_blend=False`` leaves the pose-corrective
    blend shapes out (what a core-glTF skin can express).  ``out``: a contiguous float32 (clips, n, V, 3) device tensor to
    write into.  Two launches on the current stream, no synchronisation, no host copy.  An output above 2^31 - 1 floats raises
    and names the largest n that fits: the caller chunks."""
    if not isinstance(body, BodyModel):
        raise L.TcdiffError("skin: body must be what load_body_model returns")
    if not isinstance(smpl_poses, torch.Tensor) or not isinstance(smpl_trans, torch.Tensor):
        raise L.TcdiffError("skin: smpl_poses and smpl_trans must be tensors")
    if origin not in _ORIGINS:
        raise L.TcdiffError(f"skin: origin must be 'pelvis' or 'smpl', got {origin!r}")
    if smpl_poses.dim() == 2 and smpl_poses.shape[-1] == 72:              # the pickles' layout: one clip
        smpl_poses, smpl_trans = smpl_poses.reshape(1, -1, 24, 3), smpl_trans.unsqueeze(0) if smpl_trans.dim() == 2 else smpl_trans
    if smpl_poses.dim() != 4 or tuple(smpl_poses.shape[2:]) != (24, 3):
        raise L.TcdiffError(f"skin: smpl_poses must be (clips, poses, 24, 3) or (poses, 72), got {tuple(smpl_poses.shape)}")
    clips, n = smpl_poses.shape[:2]
    if tuple(smpl_trans.shape) != (clips, n, 3):
        raise L.TcdiffError(f"skin: smpl_trans must be ({clips}, {n}, 3) beside these poses, got {tuple(smpl_trans.shape)}")
    if clips < 1 or n < 1:
        raise L.TcdiffError(f"skin: {clips} clip(s) of {n} poses: nothing to skin")
    V, P = body.V, clips * n
    if P * V * 3 > _LIMIT or P * 288 > _LIMIT:
        fits = min(_LIMIT // (3 * V * clips), _LIMIT // (288 * clips))
        raise L.TcdiffError(f"skin: {clips} x {n} poses of {V} vertices are more than 2^31 - 1 floats; at most n = {fits} poses per "
                            f"clip fit in one call ({clips} clip(s)): skin in chunks")
    if not smpl_poses.is_cuda or not smpl_trans.is_cuda:
        raise L.TcdiffError("skin runs on MI355X only (no CPU fallback)")
    if smpl_trans.device != smpl_poses.device:
        raise L.TcdiffError("skin: smpl_poses and smpl_trans must be on one device")
    dev = smpl_poses.device
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != (clips, n, V, 3) \
                or not out.is_contiguous():
            raise L.TcdiffError(f"skin: out must be a contiguous float32 ({clips}, {n}, {V}, 3) tensor on {dev}")
    q = smpl_poses.detach().float().contiguous()
    p = smpl_trans.detach().float().contiguous()
    with torch.cuda.device(dev):
        im = body.images(dev)
        if out is None:
            out = torch.empty(clips, n, V, 3, dtype=torch.float32, device=dev)
        feat = torch.empty(P, _FEAT, dtype=torch.float32, device=dev)
        A = torch.empty(P, 24, 12, dtype=torch.float32, device=dev)
        joints = torch.empty(clips, n, 24, 3, dtype=torch.float32, device=dev) if return_joints else None
        K.skin_vertices(q, p, P, im["v_shaped"], im["blend"], im["J"], im["offsets"], body._parents_c, im["weights"], im["joints"], V,
                        body.K, int(bool(pose_blend)), _ORIGINS[origin], feat, A, joints, out)
    return (out, joints) if return_joints else out
