"""CPU checks of render_sample's pose export (no GPU): the float64 restatement tests/export_ref.py against the real
reference's float32 output (tests/golden/render_export.npz), write_fk_out's files against the reference's, the host build
of fk_math.h's quat_slerp against a float64 slerp, and the four emulated kernel defects against the GPU bounds."""
import ctypes as C
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

import export_ref as R
from tcdiff_amd import export as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DN = 2


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "render_export.npz")))


def _inputs(g, mode):
    x = torch.from_numpy(g[f"{mode}_x"]).float() * float(g["sample_scale"])
    return x, torch.from_numpy(g["scale_"]), torch.from_numpy(g["min_"])


def _golden_results(g, mode):
    """the golden pickles' arrays in export_poses' shapes"""
    if mode == "long":
        return (torch.from_numpy(g["long_smpl_poses"]).reshape(1, -1, 24, 3), torch.from_numpy(g["long_smpl_trans"])[None],
                torch.from_numpy(g["long_full_pose"])[None], None)
    return (torch.stack([torch.from_numpy(g[f"normal_{n}_smpl_poses"]).reshape(-1, 24, 3) for n in range(2)]),
            torch.stack([torch.from_numpy(g[f"normal_{n}_smpl_trans"]) for n in range(2)]),
            torch.stack([torch.from_numpy(g[f"normal_{n}_full_pose"]) for n in range(2)]),
            torch.stack([torch.from_numpy(g[f"normal_render_contact_{n}"]) for n in range(2)]))


@pytest.mark.parametrize("mode", ["normal", "long"])
def test_float64_restatement_matches_the_reference_golden(gold, mode):
    x, scale, mn = _inputs(gold, mode)
    ref = R.regions(R.export(x, scale, mn, mode, DN))
    got = R.regions(_golden_results(gold, mode))
    assert set(ref) == set(got)
    for k in ref:
        assert ref[k].shape == got[k].shape, k
        assert R.scaled_err(got[k], ref[k]) <= 1e-5, (k, R.scaled_err(got[k], ref[k]))


def test_long_golden_covers_both_slerp_branches_and_the_flip(gold):
    from oracle import tcdiff_oracle as O
    x, scale, mn = _inputs(gold, "long")
    _, _, q = R.stitch_parts(x, scale, mn, DN)
    d = (O.axis_angle_to_quaternion(q[:-1, 75:]) * O.axis_angle_to_quaternion(q[1:, :75])).sum(-1)
    assert int((d < 0).sum()) > 50 and int(((1 - d.abs()) < 0.01).sum()) > 50 and int(((1 - d.abs()) >= 0.01).sum()) > 50
    assert int((x.abs() > 1).sum()) > 100           # the clamp matters


@pytest.mark.parametrize("mode", ["normal", "long"])
def test_write_fk_out_reproduces_the_reference_files(gold, mode, tmp_path):
    q, pos, poses, _ = _golden_results(gold, mode)
    if mode == "long":
        epoch, names = 3, ["data/test/features/gLH_sBM_c01_d16_mLH2_ch04_slice0.npy"]
    else:
        epoch, names = 7, ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]
    written = E.write_fk_out(str(tmp_path), mode, epoch, names, q, pos, poses)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(gold[f"{mode}_files"].tolist()) == sorted(os.path.basename(p) for p in written)
    for f in files:
        with open(tmp_path / f, "rb") as fh:
            d = pickle.load(fh)
        assert list(d) == ["smpl_poses", "smpl_trans", "full_pose"]
        pre = "long_" if mode == "long" else f"normal_{int(f.split('_')[1])}_"
        for k, v in d.items():
            want = gold[pre + k]
            assert type(v) is np.ndarray and v.dtype == np.float32 and v.shape == want.shape, (f, k, v.shape, want.shape)
            assert np.array_equal(v, want), (f, k)


def test_fk_out_names_follow_the_reference():
    assert E.fk_out_names("normal", 5, ["data/test/features/a_b.npy", "data/x/features/npy_c.npy"]) == \
        ["5_0_a_b.pkl", "5_1_wav_c.pkl"]
    assert E.fk_out_names("ctrl", "e", ["data/test/features/z.npy"]) == ["e_0_z.pkl"]
    assert E.fk_out_names("long", 2, ["data/test/features/song_a_slice7.npy", "ignored"]) == ["2_song_a.pkl"]


def _slerp_host(tmp_path):
    so = str(tmp_path / "slerp_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "host", "slerp_host.cpp")])
    lib = C.CDLL(so)
    lib.host_quat_slerp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    return lib


def test_quat_slerp_on_the_host_against_float64(tmp_path):
    """fk_math.h's quat_slerp (the kernel's source, built with g++) against R.slerp: the negative-dot flip, the linear branch
    (1 - dot < 0.01), generic pairs, and the weights 0 and 1."""
    lib = _slerp_host(tmp_path)
    g = torch.Generator().manual_seed(5)
    n = 4096
    x = torch.randn(n, 4, generator=g, dtype=torch.float64)
    x = x / x.norm(dim=-1, keepdim=True)
    y = torch.randn(n, 4, generator=g, dtype=torch.float64)
    y = y / y.norm(dim=-1, keepdim=True)
    near = x + torch.randn(n, 4, generator=g, dtype=torch.float64) * 0.02            # 1 - dot well below 0.01
    near = near / near.norm(dim=-1, keepdim=True)
    y[: n // 4] = near[: n // 4]
    y[n // 4: n // 2] = -near[n // 4: n // 2]                                        # flip, then linear
    a = torch.rand(n, generator=g, dtype=torch.float64)
    a[::7], a[1::7] = 0.0, 1.0
    x32, y32, a32 = x.float().contiguous(), y.float().contiguous(), a.float().contiguous()
    out = torch.empty(n, 4)
    lib.host_quat_slerp(x32.data_ptr(), y32.data_ptr(), a32.data_ptr(), n, out.data_ptr())
    ref = R.slerp(x32.double(), y32.double(), a32.double())
    d = (x32.double() * y32.double()).sum(-1)
    lin = (1 - d.abs()) < 0.01
    assert int((d < 0).sum()) > n // 4 and int(lin.sum()) >= n // 2 - 8 and int((~lin).sum()) > n // 4
    err = (out.double() - ref).abs().amax(-1)
    assert float(err.max()) < 2e-6, float(err.max())
    for m in (a32 == 0, a32 == 1):                                                   # the end points are x and +-y
        assert float(err[m].max()) < 5e-7
    flip = R.slerp(x32.double(), y32.double(), a32.double(), flip=False)
    assert float((flip - ref)[d < 0].abs().max()) > 0.5                               # without the flip: far off


DEFECTS = {"fade_reversed": ("long", ["root", "joints"]), "no_flip": ("long", ["axis_angle", "joints"]),
           "dancer_major": ("normal", ["root", "axis_angle", "joints", "contact"]),
           "no_clamp": ("normal", ["root", "axis_angle", "joints", "contact"])}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_emulated_defect_moves_its_region_past_the_gpu_bound(gold, defect):
    mode, regs = DEFECTS[defect]
    x, scale, mn = _inputs(gold, mode)
    good = R.regions(R.export(x, scale, mn, mode, DN))
    bad = R.regions(R.export(x, scale, mn, mode, DN, **{defect: True}))
    moved = R.max_err(good, bad)
    for k in regs:
        assert moved[k] > 100 * R.BOUNDS[k], (defect, k, moved[k], R.BOUNDS[k])
    if mode == "long":
        ov_good = R.long_overlap_regions(R.export(x, scale, mn, mode, DN), 3, 150, DN)
        ov_bad = R.long_overlap_regions(R.export(x, scale, mn, mode, DN, **{defect: True}), 3, 150, DN)
        assert R.max_err(ov_good, ov_bad)[regs[0] + "@overlap"] > 100 * R.BOUNDS[regs[0]]
