"""Restatement of AIOZDataset.process_dataset (reference dataset/group_dataset.py:167-238) for the tests of
tcdiff_motion_ingest / tcdiff_amd/dataset.py.  Every function works in the dtype it is given: in float64 it is the reference
for the kernel, in float32 every torch operation rounds where the reference's own float32 run rounds (``process(...,
dtype=torch.float32)`` is the switch).

The pytorch3d pieces the oracle does not have are restated here from pytorch3d 0.7.1's published definitions ("parity
unpinned": the package is not installed): ``quaternion_to_matrix`` (two_s = 2 / (q . q)), ``axis_angle_to_matrix`` (through
the quaternion), ``matrix_to_rotation_6d`` (the first two rows) and ``RotateAxisAngle`` about X (a float32 matrix whatever the
points' dtype, applied to row vectors: y' = c y - s z, z' = s y + c z).  tests/golden/make_golden_ingest.py binds the real
reference to exactly these.

``process(pos, q, ...)`` takes (clips, dn, sq, 3) and (clips, dn, sq, 72) and returns a dict: ``raw`` and ``feats``
(clips, dn, sq, 151), the per-clip ``data_min_`` / ``data_max_`` / ``scale_`` / ``min_`` (clips, 151), and the Z-up ``root``,
``aa`` (clips, dn, sq, 24, 3) and FK ``joints``.  Six switches emulate kernel defects: ``backward_diff`` (contacts from
feet[t] - feet[t - 1], the first frame 1), ``right_multiply`` (the root rotation multiplied on the right), ``columns_6d``
(6-D from the matrix columns), ``pos_sign`` (the position rotated by -90 degrees), ``fit_all_clips`` (one normalizer over all
clips) and ``root6d_before`` (joint 0's 6-D taken before the root rotation)."""
from __future__ import annotations

import math

import torch

from oracle import tcdiff_oracle as O

NFEAT = 151
FEET = (7, 8, 10, 11)                       # dataset/group_dataset.py:204
REGIONS = {"root": slice(4, 7), "rot6d_root": slice(7, 13), "rot6d": slice(13, NFEAT)}
EPS32 = float(torch.finfo(torch.float32).eps)
MARGIN = 8.0                                # GPU bound = MARGIN x the reference's own float32-vs-float64 error


# ---- pytorch3d 0.7.1, restated -----------------------------------------------------------------------------------------
def quaternion_to_matrix(quaternions: torch.Tensor) -> torch.Tensor:
    r, i, j, k = torch.unbind(quaternions, -1)
    two_s = 2.0 / (quaternions * quaternions).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(quaternions.shape[:-1] + (3, 3))


def axis_angle_to_matrix(axis_angle: torch.Tensor) -> torch.Tensor:
    return quaternion_to_matrix(O.axis_angle_to_quaternion(axis_angle))


def matrix_to_rotation_6d(matrix: torch.Tensor) -> torch.Tensor:
    return matrix[..., :2, :].clone().reshape(matrix.shape[:-2] + (6,))


class RotateAxisAngle:
    """pytorch3d.transforms.RotateAxisAngle about X: the angle, its cosine and sine are float32 (the class's default dtype),
    the matrix is transposed for row vectors, and transform_points is points @ M."""

    def __init__(self, angle, axis: str = "X", degrees: bool = True, dtype=torch.float32):
        if axis.upper() != "X":
            raise NotImplementedError("only the X axis is restated")
        a = torch.tensor(float(angle), dtype=dtype)
        if degrees:
            a = (a / 180.0) * math.pi
        self.cos, self.sin = torch.cos(a), torch.sin(a)

    def transform_points(self, points: torch.Tensor) -> torch.Tensor:
        c, s = self.cos.to(points.dtype), self.sin.to(points.dtype)
        x, y, z = points.unbind(-1)
        return torch.stack([x, c * y - s * z, s * y + c * z], -1)


# ---- the reference's steps ------------------------------------------------------------------------------------------------
def fit(rows: torch.Tensor):
    """dataset/scaler.py:50-70 with feature_range (-1, 1): (data_min_, data_max_, scale_, min_) of rows (n, 151); the
    near-constant threshold is float32's whatever the dtype (the reference fits in float32)"""
    lo, hi = rows.min(dim=0)[0], rows.max(dim=0)[0]
    rng = hi - lo
    rng = torch.where(rng < 10 * EPS32, torch.ones_like(rng), rng)
    scale = 2.0 / rng
    return lo, hi, scale, -1.0 - lo * scale


def transform(x: torch.Tensor, scale: torch.Tensor, min_: torch.Tensor) -> torch.Tensor:
    """dataset/scaler.py:73-78: two rounded operations, then the clip"""
    y = x * scale
    y = y + min_
    return y.clamp(-1.0, 1.0)


def process(pos, q, *, train: bool = True, scale=None, min_=None, dtype=torch.float64, backward_diff=False,
            right_multiply=False, columns_6d=False, pos_sign=False, fit_all_clips=False, root6d_before=False) -> dict:
    pos = torch.as_tensor(pos).to(dtype).clone()
    q = torch.as_tensor(q).to(dtype).clone()
    clips, dn, sq, _ = pos.shape
    aa = q.reshape(clips, dn, sq, 24, 3)
    aa_in = aa.clone()
    # 1. the root rotation, Y-up -> Z-up (group_dataset.py:184-191)
    rotation = torch.tensor([0.7071068, 0.7071068, 0, 0], dtype=dtype)
    root_quat = O.axis_angle_to_quaternion(aa[..., :1, :])
    root_quat = O.quaternion_multiply(root_quat, rotation) if right_multiply else O.quaternion_multiply(rotation, root_quat)
    aa[..., :1, :] = O.quaternion_to_axis_angle(root_quat)
    # 2. the root position (:195-198)
    rot = RotateAxisAngle(-90 if pos_sign else 90, axis="X", degrees=True)
    root = rot.transform_points(pos)
    # 3. FK (:201), every clip's dancers as the batch
    joints = O.smpl_fk(aa.reshape(clips * dn, sq, 24, 3), root.reshape(clips * dn, sq, 3)).reshape(clips, dn, sq, 24, 3)
    # 4. contacts (:204-207)
    feet = joints[..., FEET, :]
    feetv = torch.zeros(clips, dn, sq, 4, dtype=dtype)
    if backward_diff:
        feetv[:, :, 1:] = (feet[:, :, 1:] - feet[:, :, :-1]).norm(dim=-1)
    else:
        feetv[:, :, :-1] = (feet[:, :, 1:] - feet[:, :, :-1]).norm(dim=-1)
    contacts = (feetv < 0.01).to(dtype)
    # 5. 6-D rotations (:210)
    src = aa.clone()
    if root6d_before:
        src[..., 0, :] = aa_in[..., 0, :]
    mat = axis_angle_to_matrix(src)
    d6 = matrix_to_rotation_6d(mat.transpose(-1, -2) if columns_6d else mat)
    # 6. the row (:213-214)
    raw = torch.cat([contacts, root, d6.reshape(clips, dn, sq, 144)], -1)
    # 7-9. the normalizer (:217-221)
    if train:
        if fit_all_clips:
            stats = [torch.stack([s] * clips) for s in fit(raw.reshape(-1, NFEAT))]
        else:
            stats = [torch.stack(s) for s in zip(*(fit(raw[c].reshape(-1, NFEAT)) for c in range(clips)))]
        lo, hi, sc, mn = stats
    else:
        sc = torch.as_tensor(scale).to(dtype).reshape(1, NFEAT).expand(clips, NFEAT)
        mn = torch.as_tensor(min_).to(dtype).reshape(1, NFEAT).expand(clips, NFEAT)
        lo = hi = None
    feats = transform(raw, sc[:, None, None, :], mn[:, None, None, :])
    return {"raw": raw, "feats": feats, "data_min_": lo, "data_max_": hi, "scale_": sc, "min_": mn, "root": root, "aa": aa,
            "joints": joints, "feetv": feetv}


# ---- measures and bounds --------------------------------------------------------------------------------------------------
def scaled_err(a, ref) -> float:
    """max |a - ref| / max(1, |ref|)"""
    a, ref = a.double().cpu(), ref.double().cpu()
    return float(((a - ref).abs() / ref.abs().clamp(min=1.0)).max()) if ref.numel() else 0.0


def region_err(a, ref) -> dict:
    return {k: scaled_err(a[..., s], ref[..., s]) for k, s in REGIONS.items()}


def golden_f64_raw(g) -> torch.Tensor:
    """the reference's float64 run: stored as its float32 run plus the (float32) difference of the two"""
    return torch.from_numpy(g["raw_f32"]).double() + torch.from_numpy(g["raw_f64_minus_f32"]).double()


def reference_error(g) -> dict:
    """per region, the error of the reference's own float32 run against its float64 run (both in the golden)"""
    return region_err(torch.from_numpy(g["raw_f32"]), golden_f64_raw(g))


def raw_bounds(g) -> dict:
    """what the GPU tests hold the kernel's raw features to, against float64: MARGIN x reference_error"""
    return {k: MARGIN * v for k, v in reference_error(g).items()}


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """the spacing of float32 at |x| (float64 tensor in, float64 out)"""
    m = x.abs().clamp(min=float(torch.finfo(torch.float32).tiny))
    return 2.0 ** (torch.floor(torch.log2(m)) - 23)


def normalised_bound(raw_bound: dict, raw_ref: torch.Tensor, scale: torch.Tensor, min_: torch.Tensor) -> torch.Tensor:
    """per element of the normalised features: the raw bound (scaled_err's measure, so times max(1, |raw|)) times that
    column's scale_, plus one float32 ulp of the result for each of the two transform operations.  The clip only shrinks
    errors.  The contact columns have no raw error."""
    raw_ref, scale, min_ = raw_ref.double(), scale.double(), min_.double()
    per_col = torch.zeros(NFEAT, dtype=torch.float64)
    for k, s in REGIONS.items():
        per_col[s] = raw_bound[k]
    result = (raw_ref * scale + min_).clamp(-1.0, 1.0)
    return per_col * raw_ref.abs().clamp(min=1.0) * scale.abs() + 2.0 * ulp32(result)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
INPUT_SCALE = 2.0 ** -10


def synth_motion(clips: int, dn: int, sq: int, seed: int):
    """(pos (clips, dn, sq, 3), q (clips, dn, sq, 72)) float64, every value a multiple of 2^-10: root walks that are cumulative
    sums; axis-angles of magnitude 0.1 .. 2.4 rad whose root, once rotated to Z-up, also stays below 2.5 rad (so the way back
    through the export is unambiguous); joint 5 of clip 0 held at exactly zero rotation (a column range of exactly 0); in the
    last clip, dancer 0 stands still over frames 5 .. 9 (contacts of both values)."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.cumsum(torch.randn(clips, dn, sq, 3, generator=g, dtype=torch.float64) * 0.05, dim=2)
    pos = pos + torch.randn(clips, dn, 1, 3, generator=g, dtype=torch.float64)

    def draw(shape):
        u = torch.randn(shape + (3,), generator=g, dtype=torch.float64)
        return u / u.norm(dim=-1, keepdim=True) * (0.1 + 2.3 * torch.rand(shape + (1,), generator=g, dtype=torch.float64))

    def quantize(t):
        return torch.round(t / INPUT_SCALE) * INPUT_SCALE

    aa = quantize(draw((clips, dn, sq, 24)))
    rotation = torch.tensor([0.7071068, 0.7071068, 0, 0], dtype=torch.float64)
    for _ in range(64):                     # redraw the roots whose Z-up rotation would come near pi
        z = O.quaternion_to_axis_angle(O.quaternion_multiply(rotation, O.axis_angle_to_quaternion(aa[..., 0, :])))
        bad = z.norm(dim=-1) >= 2.45
        if not bool(bad.any()):
            break
        aa[..., 0, :] = torch.where(bad[..., None], quantize(draw((clips, dn, sq))), aa[..., 0, :])
    assert not bool(bad.any())
    aa[0, :, :, 5] = 0.0
    pos = quantize(pos)
    if sq >= 10:
        aa[-1, 0, 5:10] = aa[-1, 0, 5:6]
        pos[-1, 0, 5:10] = pos[-1, 0, 5:6]
    return pos, aa.reshape(clips, dn, sq, 72)


def thresholds_clear(pos, q) -> bool:
    """in float64: no foot speed within 1e-4 of 0.01, and every column range of every clip exactly 0 or above 1e-3"""
    r = process(pos, q)
    v = r["feetv"][:, :, :-1]
    rng = r["data_max_"] - r["data_min_"]
    return bool(((v - 0.01).abs() > 1e-4).all()) and bool(((rng == 0) | (rng > 1e-3)).all())


def synth_clear(clips: int, dn: int, sq: int, seed: int):
    """synth_motion with the first seed from ``seed`` on whose draws keep clear of both thresholds; returns (pos, q, seed)"""
    for s in range(seed, seed + 100):
        pos, q = synth_motion(clips, dn, sq, s)
        if thresholds_clear(pos, q):
            return pos, q, s
    raise AssertionError("no seed keeps clear of the thresholds")
