"""tcdiff_pose_export (csrc/export.hip) and render_sample's fk_out export on an MI355X: the kernel against the float64
restatement tests/export_ref.py region by region (roots, axis-angles, joints, contacts; the stitched overlap frames on their
own; rotations near pi; slerp pairs with negative dots and in the linear branch; a one-window song), render_sample's files
against the real reference's (tests/golden/render_export.npz), its return value without fk_out, and the launcher's refusals."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import export_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DN = 2


def _normalizer(scale, min_):
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_, n.scaler.min_ = scale.float(), min_.float()
    return n


IDENTITY = _normalizer(torch.ones(151), torch.zeros(151))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "render_export.npz")))


def _inputs(g, mode):
    x = torch.from_numpy(g[f"{mode}_x"]).float() * float(g["sample_scale"])
    return x, torch.from_numpy(g["scale_"]), torch.from_numpy(g["min_"])


def _check(x, norm, mode, dn, what, b=None):
    """kernel vs float64, every region; returns {region: observed}"""
    got = E.export_poses(x.to(DEV), norm, mode, dn)
    torch.cuda.synchronize()
    ref = R.export(x, norm.scaler.scale_, norm.scaler.min_, mode, dn)
    g, r = R.regions(got), R.regions(ref)
    obs = {k: R.scaled_err(g[k], r[k]) for k in r}
    if mode == "long" and b > 1:
        S = x.shape[1] // dn
        go, ro = R.long_overlap_regions(got, b, S, dn), R.long_overlap_regions(ref, b, S, dn)
        obs.update({k: R.scaled_err(go[k], ro[k]) for k in ro})
    for k in r:
        assert g[k].shape == r[k].shape, (what, k)
    print(f"[render_export] {what}: " + ", ".join(f"{k} {v:.2e} / {R.BOUNDS[k.split('@')[0]]:.0e}" for k, v in obs.items()))
    for k, v in obs.items():
        assert v <= R.BOUNDS[k.split("@")[0]], (what, k, v)
    return got


@pytest.mark.parametrize("mode", ["normal", "long"])
def test_kernel_against_float64_on_the_golden_inputs(gold, mode):
    x, scale, mn = _inputs(gold, mode)
    _check(x, _normalizer(scale, mn), mode, DN, f"golden {mode}", b=x.shape[0])


def _rot6(aa):
    """axis-angle (..., 3) float64 -> the 6-D rows (b1, b2) of its rotation matrix"""
    ang = aa.norm(dim=-1, keepdim=True)
    u = aa / ang.clamp(min=1e-300)
    c, s = torch.cos(ang)[..., None], torch.sin(ang)[..., None]
    K_ = torch.zeros(aa.shape[:-1] + (3, 3), dtype=aa.dtype)
    K_[..., 0, 1], K_[..., 0, 2], K_[..., 1, 2] = -u[..., 2], u[..., 1], -u[..., 0]
    K_ = K_ - K_.transpose(-1, -2)
    Rm = torch.eye(3, dtype=aa.dtype) + s * K_ + (1 - c) * (K_ @ K_)
    return torch.cat([Rm[..., 0, :], Rm[..., 1, :]], -1)


def _rows(aa, root, contact):
    """sample rows (..., 151) of an identity normalizer from axis-angles (..., 24, 3), roots (..., 3), contacts (..., 4)"""
    return torch.cat([contact, root, _rot6(aa.double()).reshape(aa.shape[:-2] + (144,))], -1).float()


def test_rotations_near_pi(gold):
    g = torch.Generator().manual_seed(11)
    b, S = 2, 150
    u = torch.randn(b, S * DN, 24, 3, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    eps = 10.0 ** -torch.randint(2, 7, (b, S * DN, 24, 1), generator=g).double()
    aa = u * (torch.pi - eps)
    root = torch.rand(b, S * DN, 3, generator=g, dtype=torch.float64) * 2 - 1
    contact = (torch.rand(b, S * DN, 4, generator=g) > 0.5).double()
    _check(_rows(aa, root, contact), IDENTITY, "normal", DN, "near pi", b=b)


def test_slerp_pairs_flip_and_linear_branch():
    """a 3-window song whose overlapping halves are chosen pair by pair: close rotations (linear branch), close rotations
    whose quaternions take opposite signs (negative dot, then linear), and unrelated ones (spherical branch)"""
    from oracle import tcdiff_oracle as O
    g = torch.Generator().manual_seed(12)
    b, S, h = 3, 150, 75
    u = torch.randn(b, S, DN, 24, 3, generator=g, dtype=torch.float64)
    aa = u / u.norm(dim=-1, keepdim=True) * torch.rand(b, S, DN, 24, 1, generator=g, dtype=torch.float64) * 3.0
    kind = (torch.arange(h) % 3)[:, None, None, None]
    for k in range(b - 1):
        prev = aa[k, h:]
        near = prev + torch.randn(prev.shape, generator=g, dtype=torch.float64) * 0.01
        # a quaternion on the boundary |w| = |x| (w > 0 > x) nudged to either side: matrix_to_quaternion then picks w for one
        # and x for the other, so the two come out with opposite signs
        r = (torch.rand(h, DN, 24, 2, generator=g, dtype=torch.float64) - 0.5)
        q0 = torch.cat([torch.ones(h, DN, 24, 1), -torch.ones(h, DN, 24, 1), r], -1).double()
        nudge = torch.tensor([0.01, 0.0, 0.0, 0.0], dtype=torch.float64)
        qa, qb = q0 + nudge, q0 - nudge
        qa, qb = qa / qa.norm(dim=-1, keepdim=True), qb / qb.norm(dim=-1, keepdim=True)
        aa[k, h:] = torch.where(kind == 1, O.quaternion_to_axis_angle(qa), prev)
        aa[k + 1, :h] = torch.where(kind == 0, near, torch.where(kind == 1, O.quaternion_to_axis_angle(qb), aa[k + 1, :h]))
    root = torch.rand(b, S, DN, 3, generator=g, dtype=torch.float64) * 2 - 1
    contact = torch.zeros(b, S, DN, 4, dtype=torch.float64)
    x = _rows(aa, root, contact).reshape(b, S * DN, 151)
    # the pairs the stitch sees (as the reference computes them)
    _, _, q = R.stitch_parts(x, torch.ones(151), torch.zeros(151), DN)
    d = (O.axis_angle_to_quaternion(q[:-1, h:]) * O.axis_angle_to_quaternion(q[1:, :h])).sum(-1)
    lin = (1 - d.abs()) < 0.01
    assert int((lin & (d < 0)).sum()) > 100 and int((lin & (d > 0)).sum()) > 100 and int((~lin & (d < 0)).sum()) > 100
    _check(x, IDENTITY, "long", DN, "slerp pairs", b=b)


def test_long_mode_with_one_window(gold):
    x, scale, mn = _inputs(gold, "long")
    got = _check(x[:1], _normalizer(scale, mn), "long", DN, "long b=1", b=1)
    assert got[0].shape == (1, 150 * DN, 24, 3) and got[2].shape == (1, DN, 150, 24, 3)
    nrm = E.export_poses(x[:1].to(DEV), _normalizer(scale, mn), "normal", DN)     # one window = one clip, unstitched
    for a, c in zip(got[:3], nrm[:3]):
        assert torch.equal(a, c)


@pytest.fixture(scope="module")
def diffusion():
    from oracle import tcdiff_oracle as O
    from tcdiff_amd import DanceDecoder, GaussianDiffusion
    S = 60
    sd = O.synth_state_dict(dn=DN, seq_len=S)
    model = DanceDecoder(nfeats=151, seq_len=S, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=F.gelu, required_dancer_num=DN)
    model.load_state_dict(sd)
    diff = GaussianDiffusion(model, S, 151, None, schedule="cosine", n_timestep=100, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=S).to(DEV).eval()
    cond = torch.stack([O.synth_cond(c, S) for c in range(2)])
    return diff, cond, S


@pytest.mark.parametrize("mode", ["normal", "long"])
def test_render_sample_writes_the_reference_files(gold, diffusion, mode, tmp_path):
    diff, _, _ = diffusion
    x, scale, mn = _inputs(gold, mode)
    if mode == "long":
        epoch, names = 3, ["data/test/features/gLH_sBM_c01_d16_mLH2_ch04_slice0.npy"]
    else:
        epoch, names = 7, ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]
    ret = diff.render_sample(x, None, _normalizer(scale, mn), epoch, str(tmp_path / "render"), fk_out=str(tmp_path / "fk"),
                             name=names, mode=mode, required_dancer_num=DN)
    assert ret is x                                           # the samples come back as given
    files = sorted(os.listdir(tmp_path / "fk"))
    assert files == sorted(gold[f"{mode}_files"].tolist())
    worst = {}
    for f in files:
        with open(tmp_path / "fk" / f, "rb") as fh:
            d = pickle.load(fh)
        assert list(d) == ["smpl_poses", "smpl_trans", "full_pose"]
        pre = "long_" if mode == "long" else f"normal_{int(f.split('_')[1])}_"
        for k, region in (("smpl_trans", "root"), ("smpl_poses", "axis_angle"), ("full_pose", "joints")):
            v, want = d[k], gold[pre + k]
            assert type(v) is np.ndarray and v.dtype == np.float32 and v.shape == want.shape, (f, k)
            # the golden is the reference's float32 run, itself within 1e-5 of float64 (test_render_export_cpu.py)
            e = R.scaled_err(torch.from_numpy(v), torch.from_numpy(want))
            worst[k] = max(worst.get(k, 0.0), e)
            assert e <= R.BOUNDS[region] + 1e-5, (f, k, e)
    print(f"[render_export] render_sample {mode} vs golden: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert not (tmp_path / "render").exists()                 # nothing is drawn


def test_render_sample_without_fk_out_returns_todays_samples(diffusion, tmp_path):
    diff, cond, S = diffusion
    shape = (2, S * DN, 151)
    torch.manual_seed(7)
    want = diff.ddim_sample(shape, cond).detach().cpu()
    norm = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
    for kw in ({}, {"normalizer": norm}, {"fk_out": str(tmp_path / "none")}):
        torch.manual_seed(7)
        got = diff.render_sample(shape, cond, required_dancer_num=DN, **kw)
        assert torch.equal(got, want), kw
    assert not (tmp_path / "none").exists()
    # with both, the same samples come back and the files hold their export
    torch.manual_seed(7)
    got = diff.render_sample(shape, cond, norm, 1, None, fk_out=str(tmp_path / "fk"), name=["data/a/b/c.npy", "data/a/b/d.npy"],
                             required_dancer_num=DN)
    assert torch.equal(got, want)
    q, pos, poses, _ = E.export_poses(want.to(DEV), norm, "normal", DN)
    assert sorted(os.listdir(tmp_path / "fk")) == ["1_0_c.pkl", "1_1_d.pkl"]
    with open(tmp_path / "fk" / "1_1_d.pkl", "rb") as fh:
        d = pickle.load(fh)
    assert np.array_equal(d["smpl_poses"], q[1].reshape(-1, 72).cpu().numpy())
    assert np.array_equal(d["full_pose"], poses[1].cpu().numpy()) and d["full_pose"].shape == (DN, S, 24, 3)


def test_argument_refusals():
    x = torch.zeros(3, 150 * DN, 151, device=DEV)
    sc, mn = torch.ones(151, device=DEV), torch.zeros(151, device=DEV)
    fade = torch.zeros(150, device=DEV)
    t, p, j, c = (torch.empty(450 * DN, n, device=DEV) for n in (3, 72, 72, 4))
    ok = dict(samples=x, b=3, S=150, dn=DN, mode=L.EXPORT_LONG, scale=sc, min_=mn, fade=fade, parents=SMPL_PARENTS,
              offsets=SMPL_OFFSETS, smpl_trans=t, smpl_poses=p, full_pose=j, contact=c)
    K.pose_export(**ok)
    torch.cuda.synchronize()
    bad = [dict(samples=None), dict(scale=None), dict(min_=None), dict(smpl_trans=None), dict(smpl_poses=None),
           dict(full_pose=None), dict(fade=None), dict(b=0), dict(dn=0), dict(S=0), dict(S=149), dict(mode=2),
           dict(mode=L.EXPORT_NORMAL, contact=None), dict(parents=[0] * 24)]
    for change in bad:
        with pytest.raises(L.TcdiffError):
            K.pose_export(**{**ok, **change})
    with pytest.raises(L.TcdiffError):                        # an odd frame count in long mode, through the host module
        E.export_poses(torch.zeros(2, 149 * DN, 151, device=DEV), IDENTITY, "long", DN)
    with pytest.raises(L.TcdiffError):                        # no CPU fallback
        E.export_poses(torch.zeros(2, 150 * DN, 151), IDENTITY, "normal", DN)
