"""Float64 restatement of render_sample's pose export (reference model/diffusion.py:811-988) for the tests of
tcdiff_pose_export / tcdiff_amd/export.py: the oracle's rotation and FK functions in float64, and the reference's reshape
order.  The fade / slerp weights are torch.linspace's float32 values, as the reference uses them.

``export(x, scale, min_, mode, dn)`` returns what ``export.export_poses`` returns (same shapes).  Four switches emulate
kernel defects: ``fade_reversed`` (fade_in and fade_out exchanged), ``no_flip`` (slerp without the negative-dot flip),
``dancer_major`` (rows read as dancer * S + frame instead of frame * dn + dancer) and ``no_clamp`` (unnormalize without
the clip to [-1, 1]).

BOUNDS are the bounds the GPU tests hold the kernel to, per region, in ``scaled_err``'s measure (max |error| / max(1, |value|)),
set from the first MI355X run."""
from __future__ import annotations

import torch

from oracle import tcdiff_oracle as O

# error of the float32 kernel against this float64 restatement, as scaled_err measures it (set from an MI355X run: see the
# commit message)
BOUNDS = {"root": 5e-7, "axis_angle": 2e-5, "joints": 1e-5, "contact": 2e-7}


def fade_tables(half: int):
    """(linspace(0, 1, half), linspace(1, 0, half)) as the reference evaluates them: float32, on the host."""
    return torch.linspace(0, 1, half).double(), torch.linspace(1, 0, half).double()


def unnormalize(x, scale, min_, clamp=True):
    x = x.double()
    if clamp:
        x = x.clamp(-1, 1)
    return (x - min_.double()) / scale.double()


def slerp(x, y, a, flip=True):
    """dataset/quaternion.py:35-71 in float64 (same branches: the flip, the linear weights where 1 - dot < 0.01)."""
    d = (x * y).sum(-1)
    if flip:
        neg = d < 0
        d = torch.where(neg, -d, d)
        y = torch.where(neg[..., None], -y, y)
    a = torch.zeros_like(d) + a
    lin = (1.0 - d) < 0.01
    om = torch.arccos(torch.where(lin, torch.zeros_like(d), d).clamp(-1, 1))
    so = torch.where(lin, torch.ones_like(om), torch.sin(om))
    a0 = torch.where(lin, 1.0 - a, torch.sin((1.0 - a) * om) / so)
    a1 = torch.where(lin, a, torch.sin(a * om) / so)
    return a0[..., None] * x + a1[..., None] * y


def stitch_parts(x, scale, min_, dn, *, no_clamp=False, dancer_major=False):
    """un-normalised contacts (b, S, dn, 4), roots (b, S, dn, 3) and axis-angles (b, S, dn, 24, 3) of every window / clip"""
    b, n, _ = x.shape
    S = n // dn
    u = unnormalize(x, scale, min_, clamp=not no_clamp)
    if dancer_major:
        u = u.reshape(b, dn, S, 151).transpose(1, 2)
    u = u.reshape(b, S, dn, 151)
    q = O.ax_from_6v(u[..., 7:].reshape(b, S, dn, 24, 6))
    return u[..., :4], u[..., 4:7], q


def export(x, scale, min_, mode, dn, *, fade_reversed=False, no_flip=False, dancer_major=False, no_clamp=False):
    b, n, _ = x.shape
    S = n // dn
    contact, pos, q = stitch_parts(x, scale, min_, dn, no_clamp=no_clamp, dancer_major=dancer_major)
    if mode != "long":
        joints = O.smpl_fk(q.reshape(b, S * dn, 24, 3), pos.reshape(b, S * dn, 3))
        return (q.reshape(b, S * dn, 24, 3), pos.reshape(b, S * dn, 3),
                joints.reshape(b, S, dn, 24, 3).permute(0, 2, 1, 3, 4), contact.permute(0, 2, 1, 3))
    h = S // 2
    T = S + h * (b - 1)
    w_in, w_out = fade_tables(h)
    if fade_reversed:
        w_in, w_out = w_out, w_in
    fo = torch.ones(S, dtype=torch.float64)
    fi = torch.ones(S, dtype=torch.float64)
    fo[h:] = w_out
    fi[:h] = w_in
    p = pos.clone()
    p[:-1] *= fo[:, None, None]
    p[1:] *= fi[:, None, None]
    full_pos = torch.zeros(T, dn, 3, dtype=torch.float64)
    for i in range(b):
        full_pos[i * h:i * h + S] += p[i]
    full_q = torch.zeros(T, dn, 24, 3, dtype=torch.float64)
    full_q[:h] = q[0, :h]
    if b > 1:
        wts = fade_tables(h)[0][None, :, None, None]
        merged = O.quaternion_to_axis_angle(slerp(O.axis_angle_to_quaternion(q[:-1, h:]), O.axis_angle_to_quaternion(q[1:, :h]),
                                                  wts, flip=not no_flip))
        for i in range(b - 1):
            full_q[h + i * h:h + (i + 1) * h] = merged[i]
    full_q[T - h:] = q[-1, h:]
    joints = O.smpl_fk(full_q.reshape(1, T * dn, 24, 3), full_pos.reshape(1, T * dn, 3))
    return (full_q.reshape(1, T * dn, 24, 3), full_pos.reshape(1, T * dn, 3),
            joints.reshape(1, T, dn, 24, 3).permute(0, 2, 1, 3, 4), None)


def overlap_frames(b: int, S: int):
    """frames of a stitched song that two windows share (the cross-faded / slerped ones)"""
    h = S // 2
    return torch.arange(h, h * b) if b > 1 else torch.arange(0)


def regions(out):
    """{region: float64 tensor} of export()'s / export_poses' results"""
    q, pos, joints, contact = (None if t is None else t.detach().double().cpu() for t in out)
    r = {"root": pos, "axis_angle": q, "joints": joints}
    if contact is not None:
        r["contact"] = contact
    return r


def long_overlap_regions(out, b: int, S: int, dn: int):
    """the overlap frames of a long-mode result: root, axis-angles, joints"""
    q, pos, joints, _ = (None if t is None else t.detach().double().cpu() for t in out)
    T = pos.shape[1] // dn
    f = overlap_frames(b, S)
    return {"root@overlap": pos.reshape(T, dn, 3)[f], "axis_angle@overlap": q.reshape(T, dn, 24, 3)[f],
            "joints@overlap": joints[0][:, f]}


def scaled_err(a, ref) -> float:
    """max |a - ref| / max(1, |ref|): float32 holds an axis-angle of norm 4 to a few ulps of 4, not of 1"""
    a, ref = a.double().cpu(), ref.double().cpu()
    return float(((a - ref).abs() / ref.abs().clamp(min=1.0)).max()) if ref.numel() else 0.0


def max_err(a: dict, b: dict) -> dict:
    return {k: float((a[k] - b[k]).abs().max()) if a[k].numel() else 0.0 for k in a}
