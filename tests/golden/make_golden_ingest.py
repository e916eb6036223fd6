"""ingest.npz: what the REAL reference's AIOZDataset.process_dataset (dataset/group_dataset.py:167-238) makes of 3 clips x 2
dancers x 20 frames of synthetic motion (tests/ingest_ref.py: synth_clear), on an instance made with __new__ (no files):

  train=True   float32 (the reference's own run) and float64 (torch's default dtype set to float64: everything up to the
               `.float()` of :214 is then float64; the normalizer is float32 either way, so only the un-normalised rows of
               that run are kept);
  train=False  float32, with a normalizer narrower than the data (so that the clip acts).
The un-normalised rows are recorded where the reference builds them (vectorize_many's result, before `.float()`), the fitted
normalizers where it constructs them.

pytorch3d is absent.  The four functions the oracle has (axis_angle_to_quaternion, quaternion_to_axis_angle,
quaternion_multiply, quaternion_apply) are bound to it in dataset.group_dataset, dataset.quaternion and vis; axis_angle_to_matrix,
matrix_to_rotation_6d and RotateAxisAngle to the restatements of tests/ingest_ref.py.  RotateAxisAngle's matrix is float32 in
pytorch3d, so the real transform_points would refuse float64 points: the restatement casts the float32 matrix instead.

Every reference call gets its own copies of pos and q: torch.Tensor(ndarray) shares the array's memory and
`local_q[:, :, :1, :] = root_q` (:191) writes into it.

The golden maker asserts, in float64, that no foot speed lies within 1e-4 of 0.01 and that every column range is exactly 0 or
above 1e-3, and otherwise draws again with the next seed.  Stored (data only): the int16 inputs (multiples of 2^-10), the
float32 run's features, un-normalised rows and per-clip data_min_ / data_max_ / scale_ / min_, the float64 run's un-normalised
rows as their (float32) difference from the float32 run's, and the test-mode normalizer and features.  Build container only
(needs the reference checkout)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refload  # noqa: E402
from oracle import tcdiff_oracle as O  # noqa: E402
import ingest_ref as R  # noqa: E402

refload.load()
import dataset.group_dataset as RG  # noqa: E402
import dataset.quaternion as RQ  # noqa: E402
import vis as RV  # noqa: E402
from dataset.preprocess import Normalizer  # noqa: E402

for mod in (RG, RQ, RV):
    for fn in ("axis_angle_to_quaternion", "quaternion_to_axis_angle", "quaternion_multiply", "quaternion_apply"):
        if hasattr(mod, fn):
            setattr(mod, fn, getattr(O, fn))
    for fn in ("axis_angle_to_matrix", "matrix_to_rotation_6d", "quaternion_to_matrix", "RotateAxisAngle"):
        if hasattr(mod, fn):
            setattr(mod, fn, getattr(R, fn))

recorded_raw, recorded_norm = [], []
_vectorize_many = RG.vectorize_many


def vectorize_many(data):
    out = _vectorize_many(data)
    recorded_raw.append(out.detach().clone())
    return out


class RecordingNormalizer(Normalizer):
    def __init__(self, data):
        super().__init__(data)
        recorded_norm.append(self)


RG.vectorize_many = vectorize_many
RG.Normalizer = RecordingNormalizer


def run(pos, q, train, normalizer=None, dtype=torch.float32):
    """the real process_dataset on fresh copies of the inputs -> (features, un-normalised rows, the fitted normalizers)"""
    recorded_raw.clear()
    recorded_norm.clear()
    ds = RG.AIOZDataset.__new__(RG.AIOZDataset)
    ds.train, ds.normalizer, ds.data_len = train, normalizer, -1
    np_dt = np.float32 if dtype == torch.float32 else np.float64
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        out = ds.process_dataset(pos.numpy().astype(np_dt).copy(), q.numpy().astype(np_dt).copy())
    finally:
        torch.set_default_dtype(old)
    return np.asarray(out), torch.stack(list(recorded_raw)), list(recorded_norm), ds.normalizer


CLIPS, DN, SQ = 3, 2, 20
pos, q, seed = R.synth_clear(CLIPS, DN, SQ, 2025)
pos_i, q_i = (torch.round(t / R.INPUT_SCALE).to(torch.int16) for t in (pos, q))
assert torch.equal(pos_i.double() * R.INPUT_SCALE, pos) and torch.equal(q_i.double() * R.INPUT_SCALE, q)
assert float(q.reshape(CLIPS, DN, SQ, 24, 3).norm(dim=-1).max()) < 2.5

feats32, raw32, norms32, last32 = run(pos, q, True, dtype=torch.float32)
again, _, _, _ = run(pos, q, True, dtype=torch.float32)
assert np.array_equal(feats32, again)                       # fresh copies: the run repeats
feats64, raw64, norms64, _ = run(pos, q, True, dtype=torch.float64)
assert feats32.shape == (CLIPS, DN, SQ, 151) and feats32.dtype == np.float32 and feats64.dtype == np.float32
assert raw32.dtype == torch.float32 and raw64.dtype == torch.float64
assert len(norms32) == CLIPS and last32 is norms32[-1]
assert torch.equal(raw32[..., :4], raw64[..., :4].float())  # the same contacts in both precisions
c = raw32[..., :4]
assert float(c.min()) == 0.0 and float(c.max()) == 1.0 and bool((c[:, :, -1] == 1).all())

# test mode: a normalizer fitted on the middle half of clip 0's values, so that rows of every clip fall outside it
rows = raw32[0].reshape(-1, 151)
mid = rows.sort(dim=0)[0][DN * SQ // 4: 3 * DN * SQ // 4]
given = Normalizer(mid.clone())
feats_test, raw_test, none, kept = run(pos, q, False, normalizer=given, dtype=torch.float32)
assert not none and kept is given and torch.equal(raw_test, raw32)
assert int((np.abs(feats_test) == 1).sum()) > 1000 and int((np.abs(feats_test) < 1).sum()) > 1000

out = {"pos": pos_i.numpy(), "q": q_i.numpy(), "input_scale": np.float64(R.INPUT_SCALE), "seed": np.int64(seed),
       "feats_f32": feats32, "raw_f32": raw32.numpy(),
       "raw_f64_minus_f32": (raw64 - raw32.double()).float().numpy(),
       "test_scale_": given.scaler.scale_.numpy(), "test_min_": given.scaler.min_.numpy(), "test_feats_f32": feats_test}
for name in ("data_min_", "data_max_", "scale_", "min_"):
    out[name] = torch.stack([getattr(n.scaler, name) for n in norms32]).numpy()
    assert out[name].dtype == np.float32 and out[name].shape == (CLIPS, 151)
# the stored difference gives the float64 run back to well below the 1e-10 the CPU test holds the restatement to
assert float((R.golden_f64_raw(out) - raw64).abs().max()) < 1e-13
path = os.path.join(HERE, "ingest.npz")
np.savez_compressed(path, **out)
print(seed, {k: v.shape for k, v in out.items()}, os.path.getsize(path), R.reference_error(out))
assert os.path.getsize(path) < 300 * 1024
