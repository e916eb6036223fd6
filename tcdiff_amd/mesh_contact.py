"""Do the dancers' SURFACES pass through each other?  Mesh-level contact between the bodies ``skin`` leaves on the device, per clip and
pair of dancers, in three launches (``tcm_mesh_contact``, csrc/meshcontact.hip), float64 throughout:

* ``mesh_contact_rate`` / ``mesh_contact_episodes``: the share of frames in which a vertex of one body is inside the other, and the
  runs of such frames.  A vertex is inside by a signed ray count (a winding number, not a parity) along the vertical axis.
* ``mesh_depth_max`` / ``mesh_deepest``: the largest distance of an inside vertex to the other body's surface (the closed-form
  point-triangle distance over every face), and the frame, dancer and vertex that attains it.
* ``mesh_inside_mean``: the mean number of inside vertices a frame.

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)        # what evaluate_mesh_contact does
    print(summarize(mesh_contact(body, skin(body, q, pos), dn)))

include/tcdiff_meshcontact.h is the definition.  The construction is the textbook one, restated; parity with any other tool is
unpinned.  Not built: edge-edge crossings between vertices (a limb thinner than the vertex spacing can pass unseen), mesh-level
contact of a dancer with itself (``self_contact``, tcdiff_amd/self_contact.py, measures it on the capsules), the gap between surfaces
that do not touch, using any of this inside ``keep_apart`` or ``ground``, a penetration volume, a spatial hierarchy.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .body import BodyModel, faces_closed, skin
from .export import export_poses

METRICS = ("mesh_contact_rate", "mesh_contact_episodes", "mesh_depth_max", "mesh_deepest", "mesh_inside_mean")
_LIMIT = 2 ** 31 - 1


def _fail(msg):
    raise L.TcdiffError(f"mesh_contact: {msg}")


def _faces(body_or_faces, check_closed):
    """-> (the BodyModel or None, faces as a contiguous (F, 3) int32 host array); the closedness asked of whichever was given"""
    if isinstance(body_or_faces, BodyModel):
        body, faces = body_or_faces, np.ascontiguousarray(body_or_faces.faces, np.int32)
        if check_closed and not body.closed():
            _fail("the body's mesh is not closed (a directed edge without its one reverse): inside is not defined; "
                  "check_closed=False counts the rays anyway")
        return body, faces
    faces = body_or_faces
    if isinstance(faces, torch.Tensor):
        if faces.dtype not in (torch.int32, torch.int64):
            _fail(f"faces must be int32 or int64, got {faces.dtype}")
        faces = faces.detach().cpu().numpy()                  # an input check on the host, once: the faces, never the vertices
    if not isinstance(faces, np.ndarray) or faces.dtype.kind not in "iu":
        _fail(f"the first argument must be a BodyModel or (F, 3) whole-numbered faces, got {type(body_or_faces).__name__}")
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        _fail(f"faces must be (F >= 1, 3), got {faces.shape}")
    if 3 * faces.shape[0] > _LIMIT:
        _fail(f"at most {_LIMIT // 3} faces, got {faces.shape[0]}")
    if int(faces.min()) < 0 or int(faces.max()) > _LIMIT:
        _fail(f"faces must index vertices: {int(faces.min())} .. {int(faces.max())}")
    if check_closed and not faces_closed(faces):
        _fail("the mesh is not closed (a directed edge without its one reverse): inside is not defined; check_closed=False counts "
              "the rays anyway")
    return None, np.ascontiguousarray(faces, np.int32)


def mesh_contact(body_or_faces, vertices, dn, *, up=2, return_frames=False, check_closed=True) -> dict:
    """``vertices`` (b, T dn, V, 3) float32 on the device, in metres, as ``skin`` returns them (row = frame dn + dancer), read in place
    through its strides (only the trailing V x 3 must be contiguous); ``body_or_faces``: the ``BodyModel`` they were skinned from, or
    (F, 3) faces (numpy or a tensor; copied to the host once for the checks) -- one mesh for every dancer.

    A vertex of dancer a is inside dancer b when the rays from it along +``up`` cross b's surface a non-zero signed number of times;
    its depth is its distance to b's surface.  Returns device tensors per clip and pair (``pairs(dn)`` gives the order; P = dn (dn - 1)
    / 2): float64 (b, P) ``mesh_contact_rate`` (over the frames whose vertices are all finite, NaN without one), ``mesh_depth_max``
    (metres, 0 without contact), ``mesh_inside_mean``; int64 (b, P) ``mesh_contact_episodes`` and (b, P, 3) ``mesh_deepest`` (frame,
    dancer whose vertex it is, vertex; -1 without contact).  With ``return_frames`` also ``inside`` int32 (b, P, T, 2) (a in b, b in
    a; -1 on a frame with a non-finite vertex) and ``depth`` float64 (b, P, T) (NaN there).  One dancer gives empty (b, 0) tensors
    and launches nothing.  Nothing is copied to the host; ``metrics.summarize`` does that.

    ``check_closed``: raise unless every directed edge of the mesh occurs once and its reverse once (checked on the host, once per
    body); with False the signed count is still defined and is returned.  The definition: include/tcdiff_meshcontact.h."""
    body, faces = _faces(body_or_faces, check_closed)
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 4 or vertices.shape[3] != 3:
        _fail(f"vertices must be (b, T * dn, V, 3), got {tuple(vertices.shape) if isinstance(vertices, torch.Tensor) else type(vertices)}")
    if vertices.dtype != torch.float32:
        _fail(f"vertices must be float32, got {vertices.dtype}")
    if min(vertices.shape) < 1:
        _fail(f"vertices {tuple(vertices.shape)} has an empty dimension")
    if vertices.stride(-1) != 1 or vertices.stride(-2) != 3:
        _fail(f"the trailing 2 dimension(s) of vertices must be contiguous (strides {tuple(vertices.stride())})")
    if isinstance(dn, bool) or not isinstance(dn, (int, np.integer)) or dn < 1:
        _fail(f"dn must be an int >= 1, got {dn!r}")
    b, rows, V = vertices.shape[:3]
    dn = int(dn)
    if rows % dn:
        _fail(f"{rows} rows of vertices are not T * dn with dn = {dn}")
    T = rows // dn
    if isinstance(up, bool) or up not in (0, 1, 2):
        _fail(f"up must be 0, 1 or 2, got {up!r}")
    if (body is not None and body.V != V) or int(faces.max()) >= V:
        _fail(f"the faces index vertex {int(faces.max())}, the body has {V if body is None else body.V} and vertices holds {V}")
    P = dn * (dn - 1) // 2
    if b * rows * V * 3 > _LIMIT or b * T * P * 2 > _LIMIT:
        _fail(f"more than {_LIMIT} vertex components or (clip, frame, ordered pair) triples: the caller chunks the clips")
    if not vertices.is_cuda:
        _fail("runs on MI355X only (no CPU fallback)")
    dev = vertices.device
    vertices = vertices.detach()
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)
    out = {"mesh_contact_rate": f64(b, P), "mesh_contact_episodes": i64(b, P), "mesh_depth_max": f64(b, P), "mesh_deepest": i64(b, P, 3),
           "mesh_inside_mean": f64(b, P)}
    if return_frames:
        out.update(inside=torch.empty(b, P, T, 2, dtype=torch.int32, device=dev), depth=f64(b, P, T))
    if P == 0:
        return out
    with torch.cuda.device(dev):
        faces_dev = body.images(dev)["faces"] if body is not None else torch.from_numpy(np.array(faces)).to(dev)
        workspace = torch.empty(K.mesh_contact_workspace(b, dn, T, V, faces.shape[0]), dtype=torch.uint8, device=dev)
        K.mesh_contact(vertices, faces_dev, faces, dn, int(up), workspace, out.get("inside"), out.get("depth"), out["mesh_contact_rate"],
                       out["mesh_contact_episodes"], out["mesh_depth_max"], out["mesh_deepest"], out["mesh_inside_mean"])
    return out


def evaluate_mesh_contact(samples, normalizer, dn, body, mode="normal", **kw) -> dict:
    """The sampler's normalised samples (b, S * dn, 151) -> ``mesh_contact`` of their skinned bodies: ``export_poses``, ``skin``, then
    ``mesh_contact``, everything on the device.  In "long" mode the b windows are one song, so the result has one row."""
    q, pos, _, _ = export_poses(samples, normalizer, mode, dn)
    return mesh_contact(body, skin(body, q, pos), dn, **kw)
