"""What does the generated dance look like?  The stick-figure clip of the reference's ``skeleton_render`` (vis.py:223-327: 23
bones per dancer in the dancer's colour, the root's trail on the floor, four foot markers that turn red while a foot is planted)
drawn on the device by a small software rasteriser (``tcdiff_draw_project`` + ``tcdiff_draw_raster``, csrc/draw.hip; the picture
is defined in include/tcdiff_hip.h), and an animated-PNG writer that needs the standard library only.

    q, pos, poses, contacts = export_poses(samples, normalizer, mode, dn)        # what draw_samples does
    frames = draw_dance(poses, contacts)                                         # (b, T, 480, 480, 3) uint8, on the device
    write_apng("clip0.png", frames[0].cpu())                                     # host work: zlib

The frames are not matplotlib's pixels: the reference draws through matplotlib's default perspective box with its own line caps
and anti-aliasing; here the projection is orthographic at the same two view angles.  An animated PNG has no sound; the clip with
its music is ``write_draw_out(..., format="avi")`` (tcdiff_amd/video.py: Motion-JPEG AVI, encoded on the device).  The dancers'
skinned bodies instead of the sticks: tcdiff_amd/shade.py (``write_draw_out(..., body=...)``).
"""
from __future__ import annotations

import math
import os
import struct
import zlib
from fractions import Fraction
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from . import kernels as K
from .export import _is_long, export_poses
from .fk import SMPL_PARENTS

PALETTE = ((0xE3, 0xBA, 0x8F), (0xFF, 0x6B, 0x6B), (0x0A, 0xBD, 0xE3), (0x57, 0x65, 0x74), (0x01, 0xA3, 0xA4))      # vis.py:255
PLANTED_RGB, FREE_RGB = (255, 0, 0), (0, 128, 0)          # matplotlib's "r" and "g" (vis.py:153)
GRID_RGB = (209, 209, 209)          # 255 - 209 is even: a line that covers half a pixel of a white page is no rounding tie


def _axes(up: int):
    """world axis indices of the canonical (x, y, up) frame: a cyclic permutation, so handedness is kept"""
    if up not in (0, 1, 2):
        raise L.TcdiffError(f"draw: up must be 0, 1 or 2, got {up!r}")
    return ((up + 1) % 3, (up + 2) % 3, up)


def camera(width, height, *, elev=40.0, azim=-90.0, center=(0.0, 0.0, 1.0), span=4.0, up=2) -> np.ndarray:
    """The 3 x 4 view matrix ``tcdiff_draw_project`` takes: rows give screen x (pixels), screen y (pixels, down) and depth
    (larger = farther) of (X, Y, Z, 1).  An orthographic camera with matplotlib's convention for the two angles (defaults:
    ``view_init(elev=40, azim=-90)``, vis.py:251).  With a, e in radians, in the frame whose third axis is ``up``:

        r = (-sin a, cos a, 0)    u = (-sin e cos a, -sin e sin a, cos e)    c = (cos e cos a, cos e sin a, sin e)
        s = min(W, H) / span      x = W / 2 + s (P - C) . r      y = H / 2 - s (P - C) . u      depth = -(P - C) . c

    ``span`` metres fill the shorter side (4 = the reference's axrange, vis.py:268).  ``center`` C lands in the middle of the
    image; (0, 0, 1) puts a standing dancer there, which is a choice (the reference centres its box on height 2.5).  For
    ``up`` = 0 or 1 the canonical (x, y, up) axes are the world's axes rotated cyclically, and ``center`` stays in world axes.
    These are not matplotlib's pixels: matplotlib's default is a perspective box.  Computed in float64, returned as float32."""
    W, H, span = float(width), float(height), float(span)
    if not (W >= 1 and H >= 1 and span > 0):
        raise L.TcdiffError(f"camera: width and height must be >= 1 and span > 0, got {width!r}, {height!r}, {span!r}")
    ax = _axes(up)
    a, e = math.radians(float(azim)), math.radians(float(elev))
    canon = np.array([[-math.sin(a), math.cos(a), 0.0],
                      [-math.sin(e) * math.cos(a), -math.sin(e) * math.sin(a), math.cos(e)],
                      [math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)]], np.float64)
    ruc = np.zeros((3, 3), np.float64)
    for k in range(3):
        ruc[:, ax[k]] = canon[:, k]
    C = np.asarray(center, np.float64).reshape(3)
    s = min(W, H) / span
    m = np.zeros((3, 4), np.float64)
    m[0, :3], m[0, 3] = s * ruc[0], W / 2 - s * (C @ ruc[0])
    m[1, :3], m[1, 3] = -s * ruc[1], H / 2 + s * (C @ ruc[1])
    m[2, :3], m[2, 3] = -ruc[2], C @ ruc[2]
    return m.astype(np.float32)


def floor_grid(view, *, center=(0.0, 0.0, 1.0), span=4.0, floor=0.0, up=2) -> np.ndarray:
    """The floor grid as screen-space segments (n, 4) float32: lines every metre over ``span`` around ``center`` on the plane
    ``up`` = ``floor``, through the same ``view``.  Projected in float64 on the host."""
    ax = _axes(up)
    view = np.asarray(view, np.float64).reshape(3, 4)
    C = np.asarray(center, np.float64).reshape(3)
    half = float(span) / 2
    n = int(math.floor(half + 1e-9))
    ticks = [float(k) for k in range(-n, n + 1)]
    segs = []
    for first, second in ((ax[0], ax[1]), (ax[1], ax[0])):            # lines along `second` at every tick of `first`
        for k in ticks:
            ends = []
            for side in (-half, half):
                P = np.zeros(4, np.float64)
                P[3] = 1.0
                P[first], P[second], P[up] = C[first] + k, C[second] + side, float(floor)
                ends.extend((view[:2] @ P).tolist())
            segs.append(ends)
    return np.asarray(segs, np.float32).reshape(-1, 4)


def _check_view(name, t, shape, inner):
    if not isinstance(t, torch.Tensor) or t.dim() != len(shape) or any(w is not None and s != w for s, w in zip(t.shape, shape)):
        want = ", ".join("*" if w is None else str(w) for w in shape)
        raise L.TcdiffError(f"draw_dance: {name} must be ({want}), got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if t.dtype != torch.float32:
        raise L.TcdiffError(f"draw_dance: {name} must be float32, got {t.dtype}")
    want = 1
    for k in range(1, inner + 1):                  # the trailing dimensions are read as one contiguous run
        if t.shape[-k] != 1 and t.stride(-k) != want:
            raise L.TcdiffError(f"draw_dance: the trailing {inner} dimension(s) of {name} must be contiguous "
                                f"(strides {tuple(t.stride())})")
        want *= t.shape[-k]


def _rgb(name, v):
    v = tuple(int(x) for x in v)
    if len(v) != 3 or any(not 0 <= x <= 255 for x in v):
        raise L.TcdiffError(f"draw_dance: {name} must be three values in 0..255, got {v}")
    return v


def make_style(*, background=(255, 255, 255), grid_rgb=GRID_RGB, grid_width=1.0, grid_alpha=1.0, line_width=4.0, trail_width=None,
               trail_alpha=0.6, trail_len=0, markers=True, marker_radius=None) -> L.DrawStyle:
    """Widths in pixels (a half-width is width / 2).  ``trail_width`` defaults to half of ``line_width``, ``marker_radius`` to
    ``line_width`` (the reference's scatter has size 0 and shows nothing: the size is a choice)."""
    line_width = float(line_width)
    trail_width = line_width / 2 if trail_width is None else float(trail_width)
    marker_radius = line_width if marker_radius is None else float(marker_radius)
    for name, v in (("line_width", line_width), ("trail_width", trail_width), ("marker_radius", marker_radius),
                    ("grid_width", float(grid_width))):
        if not 0 <= v <= 16384:
            raise L.TcdiffError(f"draw_dance: {name} must be in [0, 16384] pixels, got {v}")
    for name, v in (("trail_alpha", trail_alpha), ("grid_alpha", grid_alpha)):
        if not 0 <= float(v) <= 1:
            raise L.TcdiffError(f"draw_dance: {name} must be in [0, 1], got {v}")
    st = L.DrawStyle()
    for field, v in (("background", _rgb("background", background)), ("static_rgb", _rgb("grid_rgb", grid_rgb)),
                     ("planted_rgb", PLANTED_RGB), ("free_rgb", FREE_RGB)):
        setattr(st, field, (L.C.c_ubyte * 3)(*v))
    st.static_hw, st.static_alpha = float(grid_width) / 2, float(grid_alpha)
    st.line_hw, st.trail_hw, st.trail_alpha = line_width / 2, trail_width / 2, float(trail_alpha)
    st.trail_len, st.markers, st.marker_radius = int(trail_len), int(bool(markers)), marker_radius
    return st


def draw_dance(joints, contacts=None, *, width=480, height=480, view=None, grid=True, markers=True, line_width=4.0, trail_len=0,
               colors=None, background=(255, 255, 255), center=(0.0, 0.0, 1.0), span=4.0, floor=0.0, up=2, elev=40.0, azim=-90.0,
               contact_threshold=0.95, still=0.01, trail_alpha=0.6, trail_width=None, marker_radius=None, parents=None) -> torch.Tensor:
    """joints (b, dn, T, 24, 3) float32 on the device, in metres, read in place through its strides (only the trailing 24 x 3
    must be contiguous); contacts (optional) (b, dn, T, 4) float32, feet 7, 8, 10, 11: a foot's marker is red while its channel
    is above ``contact_threshold``; without contacts, while the foot moves less than ``still`` metres to the next frame.

    Returns frames (b, T, height, width, 3) uint8 RGB on the device.  ``view``: a 3 x 4 matrix as ``camera`` returns it (default:
    ``camera(width, height, elev=elev, azim=azim, center=center, span=span, up=up)``).  ``grid``: lines every metre over ``span`` on
    the plane ``up = floor``, drawn under everything else.  The root's trail is drawn on that plane too, ``trail_len`` segments of
    it (<= 0: all, as the reference).  ``colors``: the dancers' palette, (n, 3) values 0..255, dancer d takes d % n (default: the
    reference's five, vis.py:255).  ``line_width`` in pixels.  The picture's definition: include/tcdiff_hip.h."""
    _check_view("joints", joints, (None, None, None, 24, 3), 2)
    b, dn, T = joints.shape[:3]
    if min(b, dn, T) < 1:
        raise L.TcdiffError(f"draw_dance: joints {tuple(joints.shape)} has an empty dimension")
    dev = joints.device
    if contacts is not None:
        _check_view("contacts", contacts, (b, dn, T, 4), 1)
    if not joints.is_cuda or (contacts is not None and not contacts.is_cuda):
        raise L.TcdiffError("draw_dance runs on MI355X only (no CPU fallback)")
    if contacts is not None:
        if contacts.device != dev:
            raise L.TcdiffError("draw_dance: joints and contacts must be on one device")
    W, H = int(width), int(height)
    if W < 1 or H < 1:
        raise L.TcdiffError(f"draw_dance: width and height must be >= 1, got {width!r}, {height!r}")
    _axes(up)
    if view is None:
        view = camera(W, H, elev=elev, azim=azim, center=center, span=span, up=up)
    view = np.asarray(view.detach().cpu() if isinstance(view, torch.Tensor) else view, np.float32)
    if view.shape != (3, 4) or not np.isfinite(view).all():
        raise L.TcdiffError(f"draw_dance: view must be a finite 3 x 4 matrix, got shape {view.shape}")
    colors = np.asarray(PALETTE if colors is None else colors)
    if colors.ndim != 2 or colors.shape[0] < 1 or colors.shape[1] != 3 or (colors < 0).any() or (colors > 255).any():
        raise L.TcdiffError("draw_dance: colors must be (n >= 1, 3) values in 0..255")
    style = make_style(background=background, line_width=line_width, trail_width=trail_width, trail_alpha=trail_alpha,
                       trail_len=trail_len, markers=markers, marker_radius=marker_radius)
    if T > 65535 or b > 65535:
        raise L.TcdiffError(f"draw_dance: at most 65535 clips of 65535 frames per call, got {b} x {T}")
    segs = floor_grid(view, center=center, span=span, floor=floor, up=up) if grid else np.zeros((0, 4), np.float32)
    with torch.cuda.device(dev):
        static = torch.from_numpy(segs).to(dev) if len(segs) else None
        pal = torch.from_numpy(colors.astype(np.uint8)).to(dev)
        pts = torch.empty(b, T, dn, 24, 3, dtype=torch.float32, device=dev)
        trail = torch.empty(b, T, dn, 2, dtype=torch.float32, device=dev)
        order = torch.empty(b, T, dn, dtype=torch.int32, device=dev)
        planted = torch.empty(b, T, dn, 4, dtype=torch.uint8, device=dev)
        frames = torch.empty(b, T, H, W, 3, dtype=torch.uint8, device=dev)
        K.draw_project(joints, contacts, view.reshape(-1).tolist(), float(floor), int(up), float(contact_threshold), float(still),
                       pts, trail, order, planted)
        K.draw_raster(pts, trail, order, planted, b, dn, T, W, H, SMPL_PARENTS if parents is None else parents, static, len(segs),
                      pal, pal.shape[0], style, frames)
    return frames


def draw_samples(samples, normalizer, dn, mode="normal", **kw) -> torch.Tensor:
    """The sampler's normalised samples (b, S * dn, 151) -> frames of their exported poses: ``export_poses`` then ``draw_dance``
    with the exported contact channels, everything on the device.  In "long" mode the b windows are one song: (1, T, H, W, 3),
    and the markers follow the feet's displacement (the export drops the contact channels there)."""
    _, _, poses, contacts = export_poses(samples, normalizer, mode, dn)
    return draw_dance(poses, contacts, **kw)


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_apng(path, frames, fps=30, level=6) -> str:
    """frames: host uint8 (T, H, W, 3) RGB, a numpy array or a CPU tensor -> an animated PNG at ``path``: IHDR, acTL, then per
    frame fcTL + IDAT (frame 0) or fdAT (later frames), IEND.  Full frames, filter 0 on every row, a delay of 1 / fps seconds,
    looping forever; any PNG viewer shows frame 0 and browsers play it.  ``zlib`` and ``struct`` only.  The compression is host
    work (profiles/draw.txt).  No audio: tcdiff_amd/video.py writes the clip with its music."""
    if isinstance(frames, torch.Tensor):
        if frames.is_cuda:
            raise L.TcdiffError("write_apng: frames must be on the host (frames.cpu()); the encode is host work")
        frames = frames.numpy()
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8 or min(frames.shape) < 1:
        raise L.TcdiffError(f"write_apng: frames must be uint8 (T >= 1, H, W, 3), got {frames.dtype} {frames.shape}")
    delay = (1 / Fraction(fps)).limit_denominator(65535) if fps == fps and fps > 0 else None
    if delay is None or delay.numerator > 65535 or delay.numerator < 1:
        raise L.TcdiffError(f"write_apng: fps must give a delay a PNG can hold, got {fps!r}")
    T, H, W, _ = frames.shape
    out = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)),
           _chunk(b"acTL", struct.pack(">II", T, 0))]
    seq = 0
    for t in range(T):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, delay.numerator, delay.denominator, 0, 0)))
        seq += 1
        rows = np.zeros((H, 1 + 3 * W), np.uint8)                     # filter type 0 in front of every row
        rows[:, 1:] = frames[t].reshape(H, 3 * W)
        data = zlib.compress(rows.tobytes(), level)
        if t == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    path = os.fspath(path)
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return path


def draw_out_names(mode: str, epoch, name) -> list:
    """The file names ``render_sample`` writes under ``draw_out``: the reference's clip names (model/diffusion.py:960-964 with
    vis.py:317; vis.py:313 in "long" mode) with the extension of what is written here."""
    if name is None:
        raise L.TcdiffError("render_sample: draw_out needs the clips' names")
    if _is_long(mode):
        return [f'{epoch}_{"_".join(os.path.splitext(os.path.basename(name[0]))[0].split("_")[:-1])}.png']
    return [f"e{epoch}_b{num}_{os.path.splitext(os.path.basename(filename))[0]}.png" for num, filename in enumerate(name)]


def write_draw_out(draw_out, mode: str, epoch, name, poses, contacts, *, render_len=512, fps=30, body=None, q=None, pos=None,
                   format="png", quality=90, subsampling="420", audio=None, **kw) -> list:
    """Draws ``export_poses``' joints clip by clip -- device memory stays at one clip's frames -- and writes one animated PNG per
    clip (the first min(b, len(name)) clips, as the reference's zip), or one per song of its first ``render_len`` frames in "long"
    mode (model/diffusion.py:921).  Returns the paths written.

    With a ``body`` (what ``load_body_model`` returns; keyword only) and ``export_poses``' ``q`` and ``pos``, each clip's frames
    are its skinned bodies over the stick picture (tcdiff_amd/shade.py), skinned and drawn one clip at a time.  The file names and
    the writer are the same.

    ``format="avi"`` (keyword only) writes Motion-JPEG AVI files under the same names with the extension .avi instead
    (tcdiff_amd/video.py): each clip's frames are encoded on the device at ``quality`` and ``subsampling``, and only the compressed
    bytes cross to the host.  ``audio``: a list of (samples, sample_rate) per written file, or None for files without sound."""
    if format not in ("png", "avi"):
        raise L.TcdiffError(f'write_draw_out: format must be "png" or "avi", got {format!r}')
    names = draw_out_names(mode, epoch, name)
    if format == "avi":
        names = [os.path.splitext(n)[0] + ".avi" for n in names]
        if audio is not None and len(audio) < min(poses.shape[0], len(names)):
            raise L.TcdiffError(f"write_draw_out: {len(audio)} audio tracks for {min(poses.shape[0], len(names))} files")
    elif audio is not None:
        raise L.TcdiffError("write_draw_out: an animated PNG carries no audio (format=\"avi\" does)")
    if body is not None and (q is None or pos is None):
        raise L.TcdiffError("write_draw_out: a body needs export_poses' q and pos beside the joints")
    Path(draw_out).mkdir(parents=True, exist_ok=True)
    dn = poses.shape[1]
    if _is_long(mode):
        poses, contacts = poses[:1, :, :render_len], None
        if body is not None:
            q, pos = q[:1, :render_len * dn], pos[:1, :render_len * dn]
    written = []
    for num, outname in zip(range(poses.shape[0]), names):
        clip = poses[num:num + 1], None if contacts is None else contacts[num:num + 1]
        if body is None:
            frames = draw_dance(*clip, **kw)
        else:
            from .shade import draw_body_poses
            frames = draw_body_poses(body, q[num:num + 1], pos[num:num + 1], *clip, dn, **kw)
        if format == "avi":
            from .video import encode_jpeg, write_avi
            samples, rate = (None, None) if audio is None else audio[num]
            written.append(write_avi(os.path.join(draw_out, outname), encode_jpeg(frames[0], quality, subsampling), fps=fps,
                                     audio=samples, sample_rate=rate))
            continue
        written.append(write_apng(os.path.join(draw_out, outname), frames[0].cpu(), fps=fps))
    return written
