"""tci_self_contact (csrc/selfcontact.hip) and tcdiff_amd/self_contact.py on an MI355X against the numpy float64 restatement
tests/selfcontact_ref.py.

The bound is rtol 1e-10 plus atol 1e-12 on every floating-point output with NaN at the same places, and equality on every integer
output and on the per-frame `closest` plane -- the bound tests/test_group_gpu.py holds its float64 kernels to.  It is derived there,
not measured: kernel and restatement do the same float64 operations on the same float32 inputs up to the order of the sums (here one
sum, of at most a few hundred terms below 1, in the SAME order) and sqrt / division good to an ulp.  No case is excluded on the seeded
comparison scenes: the restatement alone first shows (here again, and for every input in tests/test_selfcontact_cpu.py) that no
decision is a near-tie.  The one scene with the DEFAULT radii has exact ties by construction (equal radii on bones that share a
joint); there `closest` is left out of the comparison in the frames whose reference lead is <= 1e-9, at most a tenth of them, and
the gap is compared all the same.  The worst error per output is printed; profiles/selfcontact.txt holds a run's figures."""
import importlib

import numpy as np
import pytest
import torch

import group_ref
import selfcontact_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd import metrics as M
from tcdiff_amd.apart import keep_apart
from tcdiff_amd.footlock import foot_lock
from tcdiff_amd.ground import ground

S = importlib.import_module("tcdiff_amd.self_contact")          # the package's attribute of this name is the function
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-10, 1e-12
_want = {}


def _reference(J, key, **kw):
    if key not in _want:
        ref = R.self_contact(J, details=True, **kw)
        ok, why = R.judge(ref)
        assert ok, f"a decision of the reference is a near-tie on these inputs: {why}"
        _want[key] = ref
    return _want[key]


def _compare(got, want, what, skip_closest=None):
    """skip_closest: a (b, dn, T) bool plane of the frames whose `closest` (and `self_closest`'s bones, if its frame is one) is left
    out; None: nothing is"""
    assert list(got) == R.ORDER + ["gap", "closest"], (what, list(got))
    for k in R.FLOATS + R.INTS:
        g, w = got[k], want[k]
        assert g.is_cuda and tuple(g.shape) == w.shape, (what, k, tuple(g.shape), w.shape)
        g = g.cpu().numpy()
        if k in R.INTS:
            assert g.dtype == (np.int32 if k == "closest" else np.int64), (what, k, g.dtype)
            if skip_closest is not None and k == "closest":
                g, w = g[~skip_closest], w[~skip_closest]
            if skip_closest is not None and k == "self_closest":
                assert np.array_equal(g[..., 0], w[..., 0]), (what, k, g, w)          # the frame is always compared
                b, dn = w.shape[:2]
                keep = np.array([[w[c, d, 0] < 0 or not skip_closest[c, d, w[c, d, 0]] for d in range(dn)] for c in range(b)])
                g, w = g[keep], w[keep]
            assert np.array_equal(g, w), (what, k, g, w)
            continue
        assert g.dtype == np.float64
        nan = np.isnan(w)
        err = np.abs(g - w)[~nan]
        print(f"{what} {k}: NaN {int(nan.sum())} of {w.size}, worst error {float(err.max()) if err.size else 0.0:.3e}")
        assert np.array_equal(np.isnan(g), nan), (what, k, g, w)
        assert bool((err <= ATOL + RTOL * np.abs(w[~nan])).all()), (what, k, g, w)


def _same_bits(a, b):
    assert list(a) == list(b)
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), k


def _dev(J):
    return torch.from_numpy(np.array(J, np.float32, order="C")).to(DEV)          # a copy: synth's arrays are read-only


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_float64_restatement(shape):
    """(1, 1, 1): one dancer, one frame, one wave of a four-frame workgroup; (2, 3, 5): a partial last workgroup, the clip and dancer
    indexing; 70 frames: past one lane's frames in the sums; 300: past the second launch's 256 threads and over several tiles of words"""
    J = R.synth(*shape)
    radii = R.scene_radii()
    _compare(S.self_contact(_dev(J), radii=radii, return_frames=True), _reference(J, shape, radii=radii), shape)


def test_other_parameters():
    """another tree and other radii; tolerance = 0; a hand-picked three-pair mask; hops = 0 and rest_margin = 0"""
    for n, (shape, seed, kw) in enumerate(R.parameter_cases()):
        J = R.synth(*shape, seed=seed)
        _compare(S.self_contact(_dev(J), return_frames=True, **kw), _reference(J, ("parameters", n), **kw), sorted(kw))


def test_the_default_radii():
    """radii=None: equal radii on bones that share a joint make exact ties; `closest` is compared wherever the reference leads by more
    than 1e-9, the gap everywhere"""
    shape, seed = R.DEFAULT_RADII_SCENE
    J = R.synth(*shape, seed=seed)
    want = R.self_contact(J, details=True)
    tie = want["details"]["frame_lead"] <= R.MARGIN
    assert want["details"]["tolerance_lead"] > R.MARGIN and want["details"]["dancer_lead"] > R.MARGIN
    print(f"default radii: {int(tie.sum())} of {tie.size} frames lead by <= 1e-9 ({tie.mean():.3f}; the cap is 0.10)")
    assert tie.mean() <= 0.10
    got = S.self_contact(_dev(J), return_frames=True)
    _compare(got, want, "default radii", skip_closest=tie)
    _same_bits(got, S.self_contact(_dev(J), radii=group_ref.capsule_radii(), mask=R.self_pairs(), return_frames=True))


def test_the_exact_tie_and_a_nan_joint_on_the_device():
    """inputs whose arithmetic is exact, so that the tie is a tie on the device too: the smallest code, the first frame"""
    kw = dict(parents=R.CHAIN, radii=np.full(24, 0.25), mask=R.pair_mask([(1, 5), (2, 5)]), tolerance=0.0)
    J = R.tie_body(T=2)[None, None]
    want = R.self_contact(J, **kw)
    got = S.self_contact(_dev(J), return_frames=True, **kw)
    assert (want["closest"] == 24 * 1 + 5).all() and want["self_closest"][0, 0].tolist() == [0, 1, 5]
    for k in R.FLOATS + R.INTS:
        assert np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True), k
    one = dict(parents=R.CHAIN, radii=np.full(24, 0.25), mask=R.pair_mask([(1, 3), (1, 5), (3, 5)]), tolerance=0.125)
    a = [1.0, 0.25, 0.25, 1.0, 0.125, 1.0, 0.25, 1.0, 0.375]             # the last frame is AT the tolerance: no contact
    for poison in (None, (4, 3, 1), (4, 5, 2)):                          # clean; a NaN on bone 3 of the deepest frame; on bone 5
        B = R.bars(a, a[::-1])
        if poison:
            B[poison] = np.nan
        want = R.self_contact(B[None, None], **one)
        got = S.self_contact(_dev(B[None, None]), return_frames=True, **one)
        for k in R.FLOATS + R.INTS:
            assert np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True), (poison, k)
        assert bool(np.isnan(want["gap"][0, 0, 4])) == bool(poison) and want["gap"][0, 0, 8] == -0.125


def test_the_frame_planes_land_where_they_are_told_and_nothing_else_is_written():
    shape = (2, 3, 5)
    b, dn, T = shape
    pad = 37
    J = _dev(R.synth(*shape))
    radii = R.scene_radii()
    public = S.self_contact(J, radii=radii, return_frames=True)
    sizes = {"gap": (b, dn, T), "closest": (b, dn, T), "self_closest": (b, dn, 3), "self_pair_frames": (b, dn, 253)}
    buf, view = {}, {}
    for k in R.ORDER + ["gap", "closest"]:
        shp = sizes.get(k, (b, dn))
        n = int(np.prod(shp))
        buf[k] = torch.full((n + 2 * pad,), -77, dtype=public[k].dtype, device=DEV)
        view[k] = buf[k][pad:pad + n].view(shp)
    nbytes = K.self_contact_workspace(b, dn, T)
    assert nbytes == 44 * b * dn * T
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    mask = R.self_pairs(radii=radii)
    words = [sum(1 << int(k - 64 * w) for k in np.flatnonzero(mask) if k // 64 == w) for w in range(4)]

    def run(gap, closest):
        K.self_contact(J, [-1] + R.SMPL_PARENTS[1:], radii.tolist(), words, 0.03, ws[:nbytes], gap, closest, view["self_contact_rate"],
                       view["self_gap_min"], view["self_contact_episodes"], view["self_closest"], view["self_depth_mean"],
                       view["self_pair_frames"])
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all())
        for k in buf:
            assert bool((buf[k][:pad] == -77).all()) and bool((buf[k][-pad:] == -77).all()), k
    run(view["gap"], view["closest"])
    _same_bits({k: view[k] for k in public}, public)
    for k in ("gap", "closest"):
        view[k].fill_(-77)
    run(None, None)                                                       # the planes in the workspace: the caller's are not written
    assert bool((buf["gap"] == -77).all()) and bool((buf["closest"] == -77).all())
    metrics = {k: v for k, v in public.items() if k not in ("gap", "closest")}
    _same_bits({k: view[k] for k in metrics}, metrics)
    _same_bits(S.self_contact(J, radii=radii), metrics)                   # return_frames=False: the same metrics, no plane
    assert list(S.self_contact(J, radii=radii)) == R.ORDER


def test_strided_views_are_read_in_place_and_runs_repeat():
    """the frame-major layout tcdiff_pose_export writes, permuted as export_poses permutes it, without the copy"""
    shape = (2, 3, 150)
    J = _dev(R.synth(*shape))
    jv = J.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)          # (b, T, dn, 24, 3) storage
    assert not jv.is_contiguous() and torch.equal(jv, J)
    first = S.self_contact(J, return_frames=True)
    _same_bits(S.self_contact(jv, return_frames=True), first)
    _same_bits(S.self_contact(J, return_frames=True), first)                    # two runs, the same bits
    wide = torch.zeros(2, 3, 150, 30, 3, device=DEV)                            # a slice with larger outer strides
    wide[:, :, :, 3:27] = J
    _same_bits(S.self_contact(wide[:, :, :, 3:27], return_frames=True), first)
    one = S.self_contact(J[:, 1:2], return_frames=True)                          # one dancer of three, in place
    for k in first:
        x, y = one[k], first[k][:, 1:2]
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y), k
    with pytest.raises(L.TcdiffError, match="contiguous"):
        S.self_contact(J.transpose(-1, -2).contiguous().transpose(-1, -2))
    with pytest.raises(L.TcdiffError, match="tolerance"):
        S.self_contact(J, tolerance=-1.0)


def test_evaluate_self_contact_is_export_then_self_contact_and_summarize_takes_it():
    g = torch.Generator().manual_seed(11)
    dn, Sq = 3, 20
    norm = tio.Normalizer(torch.randn(400, 151, generator=g))
    x = (torch.rand(2, Sq * dn, 151, generator=g) * 2 - 1).to(DEV)
    got = S.evaluate_self_contact(x, norm, dn)
    _, _, poses, _ = E.export_poses(x, norm, "normal", dn)
    assert tuple(poses.shape) == (2, dn, Sq, 24, 3) and list(got) == R.ORDER and tuple(got["self_contact_rate"].shape) == (2, 3)
    assert tuple(got["self_closest"].shape) == (2, 3, 3) and tuple(got["self_pair_frames"].shape) == (2, 3, 253)
    _same_bits(got, S.self_contact(poses))
    summary = M.summarize(got)
    assert list(summary) == R.ORDER and all(type(v) is float for v in summary.values())
    framed = M.summarize(S.self_contact(poses, return_frames=True))
    assert list(framed) == R.ORDER + ["gap", "closest"] and all(type(v) is float for v in framed.values())
    # long mode: 3 half-overlapping windows of 20 frames are one song of 40
    x3 = (torch.rand(3, Sq * dn, 151, generator=g) * 2 - 1).to(DEV)
    got = S.evaluate_self_contact(x3, norm, dn, mode="long", tolerance=0.01, hops=1)
    _, _, full, _ = E.export_poses(x3, norm, "long", dn)
    assert tuple(full.shape) == (1, dn, 40, 24, 3) and tuple(got["self_closest"].shape) == (1, 3, 3)
    _same_bits(got, S.self_contact(full, tolerance=0.01, hops=1))


def test_the_correctors_joints_are_accepted_as_they_are():
    g = torch.Generator().manual_seed(12)
    dn, Sq = 3, 20
    norm = tio.Normalizer(torch.randn(400, 151, generator=g))
    x = (torch.rand(2, Sq * dn, 151, generator=g) * 2 - 1).to(DEV)
    q, pos, poses, contacts = E.export_poses(x, norm, "normal", dn)
    for name, joints in (("keep_apart", keep_apart(pos, poses, dn=dn).joints), ("ground", ground(pos, poses, contacts, dn=dn).joints),
                         ("foot_lock", foot_lock(q, pos, contacts, dn=dn).joints)):
        got = S.self_contact(joints, return_frames=True)
        want = R.self_contact(joints.cpu().numpy())
        for k in ("gap", "self_contact_rate", "self_gap_min"):
            assert np.allclose(got[k].cpu().numpy(), want[k], rtol=RTOL, atol=ATOL, equal_nan=True), (name, k)
        assert tuple(got["self_pair_frames"].shape) == (2, dn, 253) and int(got["self_pair_frames"].max()) <= Sq, name
