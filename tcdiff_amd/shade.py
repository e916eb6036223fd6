"""What does the generated dance look like with bodies?  The vertices ``skin`` returns, drawn on the device as shaded, depth-tested
frames by a small software rasteriser for triangle meshes (``tcr_mesh_vertices`` + ``tcr_mesh_raster``, csrc/shade.hip; the
picture is defined in include/tcdiff_shade.h): a per-pixel depth test, so dancers occlude each other limb by limb, and smooth
(interpolated-normal) Lambert shading in the dancer's colour.

    body = load_body_model("SMPL_NEUTRAL.npz")                              # the user's file; none is shipped
    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)
    vertices = skin(body, q, pos)                                           # (b, T * dn, V, 3) on the device
    frames = draw_bodies(body, vertices, dn)                                # (b, T, 480, 480, 3) uint8, on the device
    frames = draw_body_samples(samples, normalizer, dn, body)               # the same over the floor grid, trails and foot markers
    normals = vertex_normals(body, vertices)                                # (b, T * dn, V, 3) float32 unit vectors

Three launches per call on the current stream, no synchronisation, no host copy, no CPU fallback.  The camera is ``draw.camera``'s
(orthographic).  Parity with any other renderer is unpinned: the reference's counterpart is an offline Blender pipeline.  Not
built: anti-aliasing, perspective, textures, shadows, pose correctives beyond what ``skin`` applies, muxed audio.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .body import BodyModel, skin
from .draw import PALETTE, _rgb, camera, draw_dance
from .export import export_poses

TILE = L.SHADE.constants["TC_SHADE_TILE"]
CHUNK = L.SHADE.constants["TC_SHADE_CHUNK"]
MAX_SIDE = L.SHADE.constants["TC_SHADE_MAX_SIDE"]
_PER_TRIANGLE = L.SHADE.constants["TC_SHADE_SCRATCH_PER_TRIANGLE"]
_LIMIT = 2 ** 31 - 1
_DRAW_DANCE_KEYS = ("grid", "markers", "line_width", "trail_len", "floor", "contact_threshold", "still", "trail_alpha", "trail_width",
                    "marker_radius", "parents")


def scratch_bytes(b, T, dn, F) -> int:
    """the scratch ``tcr_mesh_raster`` needs (the header's formula): one packed pixel box per triangle of every frame and one per
    chunk of them"""
    G = int(dn) * int(F)
    return _PER_TRIANGLE * int(b) * int(T) * (G + (G + CHUNK - 1) // CHUNK)


def _vertices(what, body, vertices):
    if not isinstance(body, BodyModel):
        raise L.TcdiffError(f"{what}: body must be what load_body_model returns")
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 4 or tuple(vertices.shape[2:]) != (body.V, 3):
        got = tuple(vertices.shape) if isinstance(vertices, torch.Tensor) else type(vertices)
        raise L.TcdiffError(f"{what}: vertices must be (clips, poses, {body.V}, 3) as skin returns them, got {got}")
    if vertices.dtype != torch.float32:
        raise L.TcdiffError(f"{what}: vertices must be float32, got {vertices.dtype}")
    if vertices.shape[0] < 1 or vertices.shape[1] < 1:
        raise L.TcdiffError(f"{what}: vertices {tuple(vertices.shape)} has an empty dimension")
    if not vertices.is_cuda:
        raise L.TcdiffError(f"{what} runs on MI355X only (no CPU fallback)")
    if vertices.numel() > _LIMIT:
        raise L.TcdiffError(f"{what}: {tuple(vertices.shape)} is more than 2^31 - 1 floats: draw in chunks of clips or frames")
    return vertices.detach().contiguous()


def make_shade_style(*, background=(255, 255, 255), ambient=0.35, light=(0.0, -1.0, 0.0)) -> L.ShadeStyle:
    """``light``: the direction toward the light in world axes, normalised here in float64; ``ambient`` in [0, 1]"""
    ambient = float(ambient)
    if not 0.0 <= ambient <= 1.0:
        raise L.TcdiffError(f"draw_bodies: ambient must be in [0, 1], got {ambient}")
    l = np.asarray(light, np.float64).reshape(-1)
    if l.shape != (3,) or not np.isfinite(l).all() or not np.linalg.norm(l) > 0:
        raise L.TcdiffError(f"draw_bodies: light must be three finite numbers, not all zero, got {light!r}")
    l = l / np.linalg.norm(l)
    st = L.ShadeStyle()
    st.background = (L.C.c_ubyte * 3)(*_rgb("background", background))
    st.ambient = ambient
    st.light = (L.C.c_float * 3)(*[float(x) for x in l])
    return st


def vertex_normals(body, vertices) -> torch.Tensor:
    """vertices (clips, n, V, 3) float32 on the device, as ``skin`` returns them -> the unit vertex normals (clips, n, V, 3) float32
    on the device: per vertex the area-weighted sum of its faces' normals (float64 on the device, one rounding at the store), zero
    for a vertex that no face names.  One launch, no atomics: the same vertices give the same bits."""
    v = _vertices("vertex_normals", body, vertices)
    dev = v.device
    with torch.cuda.device(dev):
        im = body.images(dev)
        out = torch.empty_like(v)
        K.mesh_vertices(v, im["faces"], im["adj_start"], im["adj_faces"], v.shape[0] * v.shape[1], body.V, body.faces.shape[0],
                        [0.0] * 12, None, out)
    return out


def draw_bodies(body, vertices, dn, *, width=480, height=480, view=None, colors=None, background=(255, 255, 255), ambient=0.35,
                light=None, under=None, center=(0.0, 0.0, 1.0), span=4.0, up=2, elev=40.0, azim=-90.0) -> torch.Tensor:
    """vertices (b, T * dn, V, 3) float32 on the device, as ``skin`` returns them (row = frame * dn + dancer) -> frames
    (b, T, height, width, 3) uint8 RGB on the device: every dancer's surface, depth-tested per pixel and shaded
    ``ambient + (1 - ambient) |n . light|`` with the interpolated vertex normal, in the dancer's colour.

    ``view``: a 3 x 4 matrix as ``draw.camera`` returns it (default: ``camera(width, height, elev=elev, azim=azim, center=center,
    span=span, up=up)``, ``draw_dance``'s).  ``light``: the direction toward the light in world axes; None is a headlight, the
    unit vector from the scene toward the camera (minus row 2 of the view, normalised in float64).  ``colors``: the dancers'
    palette, (n, 3) values 0..255, dancer d takes d % n (default: ``draw.PALETTE``).  ``under``: uint8 frames of the output's
    shape on the same device, shown wherever no body is (default: ``background``).  The picture's definition:
    include/tcdiff_shade.h."""
    v = _vertices("draw_bodies", body, vertices)
    dn = int(dn)
    b, n = v.shape[:2]
    if dn < 1 or n % dn:
        raise L.TcdiffError(f"draw_bodies: {n} poses are not a whole number of frames of {dn} dancers")
    T = n // dn
    W, H = int(width), int(height)
    if W < 1 or H < 1 or W > MAX_SIDE or H > MAX_SIDE:
        raise L.TcdiffError(f"draw_bodies: width and height must be in 1..{MAX_SIDE}, got {width!r}, {height!r}")
    if T > 65535 or b > 65535:
        raise L.TcdiffError(f"draw_bodies: at most 65535 clips of 65535 frames per call, got {b} x {T}")
    F = int(body.faces.shape[0])
    if b * T * H * W * 3 > _LIMIT or b * n * F > _LIMIT:
        raise L.TcdiffError(f"draw_bodies: {b} x {T} frames of {W} x {H} pixels and {dn * F} triangles are more than 2^31 - 1 bytes "
                            "or triangles: draw in chunks of clips or frames")
    if view is None:
        view = camera(W, H, elev=elev, azim=azim, center=center, span=span, up=up)
    view = np.asarray(view.detach().cpu() if isinstance(view, torch.Tensor) else view, np.float32)
    if view.shape != (3, 4) or not np.isfinite(view).all():
        raise L.TcdiffError(f"draw_bodies: view must be a finite 3 x 4 matrix, got shape {view.shape}")
    if light is None:
        light = -view[2, :3].astype(np.float64)
    style = make_shade_style(background=background, ambient=ambient, light=light)
    colors = np.asarray(PALETTE if colors is None else colors)
    if colors.ndim != 2 or colors.shape[0] < 1 or colors.shape[1] != 3 or (colors < 0).any() or (colors > 255).any():
        raise L.TcdiffError("draw_bodies: colors must be (n >= 1, 3) values in 0..255")
    dev = v.device
    if under is not None:
        if not isinstance(under, torch.Tensor) or under.dtype != torch.uint8 or tuple(under.shape) != (b, T, H, W, 3):
            raise L.TcdiffError(f"draw_bodies: under must be a uint8 ({b}, {T}, {H}, {W}, 3) tensor")
        if under.device != dev:
            raise L.TcdiffError("draw_bodies: vertices and under must be on one device")
        under = under.contiguous()
    with torch.cuda.device(dev):
        im = body.images(dev)
        pal = torch.from_numpy(colors.astype(np.uint8)).to(dev)
        screen, normals = torch.empty_like(v), torch.empty_like(v)
        scratch = torch.empty(scratch_bytes(b, T, dn, F) // 4, dtype=torch.int32, device=dev)
        frames = torch.empty(b, T, H, W, 3, dtype=torch.uint8, device=dev)
        K.mesh_vertices(v, im["faces"], im["adj_start"], im["adj_faces"], b * n, body.V, F, view.reshape(-1).tolist(), screen, normals)
        K.mesh_raster(screen, normals, im["faces"], b, T, dn, body.V, F, W, H, pal, pal.shape[0], style, under, scratch, frames)
    return frames


def draw_body_poses(body, q, pos, poses, contacts, dn, *, pose_blend=True, **kw) -> torch.Tensor:
    """What ``export_poses`` returned for some clips -> their frames: ``skin``, then ``draw_dance`` for the floor grid, the trails and
    the foot markers (and the bones, which the bodies cover), then ``draw_bodies`` over it.  Keywords go to both where both take
    them (the size, the camera, ``colors``, ``background``); ``ambient`` and ``light`` to the bodies, the rest to ``draw_dance``."""
    stick = {k: kw.pop(k) for k in _DRAW_DANCE_KEYS if k in kw}
    shade = {k: kw.pop(k) for k in ("ambient", "light") if k in kw}
    vertices = skin(body, q, pos, pose_blend=pose_blend)
    under = draw_dance(poses, contacts, **kw, **stick)
    return draw_bodies(body, vertices, dn, under=under, **kw, **shade)


def draw_body_samples(samples, normalizer, dn, body, mode="normal", **kw) -> torch.Tensor:
    """The sampler's normalised samples (b, S * dn, 151) -> frames of their skinned bodies over the stick picture's floor grid,
    trails and foot markers: ``export_poses``, ``skin``, ``draw_dance``, ``draw_bodies``, everything on the device.  In "long" mode
    the b windows are one song, (1, T, H, W, 3), as in ``draw_samples``."""
    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)
    return draw_body_poses(body, q, pos, poses, contacts, dn, **kw)
