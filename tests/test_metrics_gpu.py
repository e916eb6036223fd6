"""tcdiff_motion_metrics (csrc/metrics.hip) and tcdiff_amd/metrics.py on an MI355X against the numpy float64 restatement
tests/metrics_ref.py.

The bound is rtol 1e-10 on every floating-point output with NaN at the same places, and equality on the two counts.  It is
derived, not measured: kernel and restatement do the same float64 operations on the same float32 inputs up to the order of
the sums -- each of at most ~1e4 non-negative terms, so an order error of at most N 2^-53 ~ 1e-12 -- and sqrt / exp good to a few
ulp.  No case is excluded: the reference alone first shows that no decision (contact threshold, still, radius, local minimum) is
a near-tie on the seeded inputs."""
import numpy as np
import pytest
import torch

import metrics_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-10
COUNTS = ("contact_frames", "motion_beats")
_want = {}


def _reference(shape, **kw):
    key = (shape, tuple(sorted(kw.items())))
    if key not in _want:
        joints, contacts, beats = R.synth(*shape)
        assert R.decisions_clear(joints, contacts, beats, **kw), "a decision of the reference is a near-tie on these inputs"
        _want[key] = R.metrics(joints, contacts, beats, **kw)
    return _want[key]


def _device_inputs(shape):
    return tuple(torch.from_numpy(a).to(DEV) for a in R.synth(*shape))


def _compare(got, want, what):
    assert list(got) == [k for k in ("pfc", "contact_slide", "contact_break", "contact_frames", "collision_rate", "beat_align",
                                     "motion_beats") if k in want], (what, list(got))
    for k, w in want.items():
        g = got[k]
        assert g.is_cuda and tuple(g.shape) == w.shape, (what, k, tuple(g.shape))
        g = g.cpu().numpy()
        if k in COUNTS:
            assert g.dtype == np.int64 and np.array_equal(g, w), (what, k, g, w)
            continue
        assert g.dtype == np.float64
        nan = np.isnan(w)
        err = np.abs(g - w)[~nan]
        nz = w[~nan] != 0
        rel = float((err[nz] / np.abs(w[~nan][nz])).max()) if nz.any() else 0.0
        print(f"{what} {k}: NaN {int(nan.sum())} of {w.size}, worst relative error {rel:.3e}")
        assert np.array_equal(np.isnan(g), nan), (what, k, g, w)
        assert bool((err <= RTOL * np.abs(w[~nan])).all()), (what, k, g, w)


def _same_bits(a, b):
    assert list(a) == list(b)
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), k


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_float64_restatement(shape):
    """T = 1, 3, 4: the NaN / zero rules; T = 20: N below the filter radius; 45, 150, 1125: not multiples of 64; 1125: a sequence
    longer than the per-sequence workgroup's 256 threads, several frames per thread"""
    joints, contacts, beats = _device_inputs(shape)
    _compare(M.motion_metrics(joints, contacts, beats), _reference(shape), shape)


def test_other_parameters():
    shape = (2, 3, 45)
    kw = dict(fps=60, up=1, contact_threshold=0.5, still=0.02, radius=0.5, sigma_smooth=2.0, sigma_beat=1.5)
    joints, contacts, beats = _device_inputs(shape)
    _compare(M.motion_metrics(joints, contacts, beats, **kw), _reference(shape, **kw), kw)
    kw = dict(up=0, sigma_smooth=12.0)                       # radius 48 > N = 44
    _compare(M.motion_metrics(joints, contacts, beats, **kw), _reference(shape, **kw), kw)


def test_reflection_wraps_more_than_a_whole_period():
    """N = 7 under a filter radius of 20 > 2 N: a wrong multi-period wrap would lose the motion beat on frame 3 of dancer 0 or give
    dancer 1 one, and move beat_align = (1 + exp(-4 / 18)) / 2"""
    joints, contacts, beats = R.short_wrap_case()
    assert R.decisions_clear(joints, contacts, beats)
    want = R.metrics(joints, contacts, beats)
    assert want["motion_beats"].tolist() == [[1, 0]] and abs(want["beat_align"][0, 0] - (1 + np.exp(-4 / 18)) / 2) < 1e-15
    got = M.motion_metrics(*(torch.from_numpy(a).to(DEV) for a in (joints, contacts, beats)))
    _compare(got, want, "T = 8")


def test_absent_inputs_omit_their_keys():
    shape = (2, 3, 45)
    joints, contacts, beats = _device_inputs(shape)
    full = M.motion_metrics(joints, contacts, beats)
    none = M.motion_metrics(joints)
    assert list(none) == ["pfc", "collision_rate"]
    only_c = M.motion_metrics(joints, contacts)
    assert list(only_c) == ["pfc", "contact_slide", "contact_break", "contact_frames", "collision_rate"]
    only_b = M.motion_metrics(joints, beats=beats)
    assert list(only_b) == ["pfc", "collision_rate", "beat_align", "motion_beats"]
    for part in (none, only_c, only_b):
        _same_bits(part, {k: full[k] for k in part})


def test_strided_views_are_read_in_place_and_runs_repeat():
    """the frame-major layout tcdiff_pose_export writes, permuted as export_poses permutes it, without the copy"""
    shape = (2, 3, 45)
    joints, contacts, beats = _device_inputs(shape)
    jv = joints.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)          # (b, T, dn, 24, 3) storage
    cv = contacts.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not jv.is_contiguous() and not cv.is_contiguous() and torch.equal(jv, joints)
    first = M.motion_metrics(joints, contacts, beats)
    _same_bits(M.motion_metrics(jv, cv, beats), first)
    _same_bits(M.motion_metrics(joints, contacts, beats), first)
    _compare(first, _reference(shape), "contiguous")
    wide = torch.zeros(2, 3, 45, 30, 3, device=DEV)                                  # a slice with larger outer strides
    wide[:, :, :, 3:27] = joints
    _same_bits(M.motion_metrics(wide[:, :, :, 3:27], contacts, beats), first)
    with pytest.raises(L.TcdiffError, match="contiguous"):
        M.motion_metrics(joints.transpose(-1, -2).contiguous().transpose(-1, -2), contacts, beats)
    with pytest.raises(L.TcdiffError):
        M.motion_metrics(joints, contacts[:, :, :-1], beats)
    with pytest.raises(L.TcdiffError, match="uint8"):
        M.motion_metrics(joints, contacts, beats.bool())
    with pytest.raises(L.TcdiffError):
        M.motion_metrics(joints, contacts, beats, up=3)
    with pytest.raises(L.TcdiffError):
        M.motion_metrics(joints, contacts, beats, sigma_smooth=200.0)


def test_evaluate_samples_is_export_then_metrics():
    g = torch.Generator().manual_seed(11)
    dn, S = 3, 20
    norm = tio.Normalizer(torch.randn(400, 151, generator=g))
    x = (torch.rand(2, S * dn, 151, generator=g) * 2 - 1).to(DEV)
    cond = torch.rand(2, 2 * S + 1, 438, generator=g)
    cond[..., 53] = (torch.rand(2, 2 * S + 1, generator=g) < 0.2).float()
    cond = cond.to(DEV)
    got = M.evaluate_samples(x, norm, cond, dn)
    _, _, poses, contacts = E.export_poses(x, norm, "normal", dn)
    assert tuple(poses.shape) == (2, dn, S, 24, 3)
    _same_bits(got, M.motion_metrics(poses, contacts, M.beats_from_cond(cond, S)))
    assert "contact_frames" in got and "beat_align" in got
    # the frame-major storage the export kernel writes, read through the permuted view, gives the same bits as the copy
    pv = poses.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)
    _same_bits(M.motion_metrics(pv, contacts, M.beats_from_cond(cond, S)), got)
    assert all(type(v) is float for v in M.summarize(got).values())
    # long mode: 3 half-overlapping windows of 20 frames are one song of 40; the export drops the contacts
    x3 = (torch.rand(3, S * dn, 151, generator=g) * 2 - 1).to(DEV)
    cond3 = (torch.rand(3, 2 * S, 438, generator=g) < 0.2).float().to(DEV)
    got = M.evaluate_samples(x3, norm, cond3, dn, mode="long", radius=0.4)
    _, _, full, none = E.export_poses(x3, norm, "long", dn)
    assert none is None and tuple(full.shape) == (1, dn, 40, 24, 3)
    assert list(got) == ["pfc", "collision_rate", "beat_align", "motion_beats"] and tuple(got["pfc"].shape) == (1, dn)
    _same_bits(got, M.motion_metrics(full, None, M.beats_from_cond(cond3, 40, long=True), radius=0.4))
