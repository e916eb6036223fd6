"""CPU checks of the motion ingest (no GPU): the restatement tests/ingest_ref.py against the real reference's float64 and
float32 runs (tests/golden/ingest.npz), the six emulated kernel defects against the GPU bounds, the host build of fk_math.h's
ingest functions against float64, AIOZDataset.load_aioz's file logic against the reference's on a temporary tree, and the
normalizer.pkl a test-mode dataset writes, read back by plain pickle under the reference's modules."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import ingest_ref as R
from oracle import refload
from oracle import tcdiff_oracle as O
from tcdiff_amd import dataset as D
from tcdiff_amd import io as tio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("data_min_", "data_max_", "scale_", "min_")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ingest.npz")))


def _inputs(g):
    s = float(g["input_scale"])
    return torch.from_numpy(g["pos"]).double() * s, torch.from_numpy(g["q"]).double() * s


@pytest.fixture(scope="module")
def ref64(gold):
    return R.process(*_inputs(gold))


def test_golden_inputs_are_the_synthetic_motion_and_keep_clear_of_the_thresholds(gold):
    pos, q = _inputs(gold)
    p2, q2 = R.synth_motion(3, 2, 20, int(gold["seed"]))
    assert torch.equal(pos, p2) and torch.equal(q, q2)
    assert R.thresholds_clear(pos, q)
    assert float(q.reshape(3, 2, 20, 24, 3).norm(dim=-1).max()) < 2.5
    raw = torch.from_numpy(gold["raw_f32"])
    assert bool((raw[0, :, :, 7 + 6 * 5: 13 + 6 * 5] == torch.tensor([1.0, 0, 0, 0, 1, 0])).all())      # the joint held at zero
    rng = gold["data_max_"] - gold["data_min_"]
    assert int((rng[0] == 0).sum()) >= 6 and bool((gold["scale_"][rng == 0] == 2.0).all())               # range 0 -> 1
    c = raw[..., :4]
    assert int((c == 0).sum()) > 50 and int((c[:, :, :-1] == 1).sum()) >= 16 and bool((c[:, :, -1] == 1).all())


def test_float64_restatement_matches_the_reference_float64_run(gold, ref64):
    want = R.golden_f64_raw(gold)
    assert ref64["raw"].shape == want.shape
    assert float((ref64["raw"] - want).abs().max()) <= 1e-10, float((ref64["raw"] - want).abs().max())


def test_float32_restatement_matches_the_reference_float32_run(gold, ref64):
    pos, q = _inputs(gold)
    r32 = R.process(pos, q, dtype=torch.float32)
    err = R.reference_error(gold)
    raw = torch.from_numpy(gold["raw_f32"])
    assert torch.equal(r32["raw"][..., :4], raw[..., :4])                              # contacts: exact
    for k in STATS:                                                                     # fitted statistics: exact
        assert r32[k].dtype == torch.float32 and torch.equal(r32[k], torch.from_numpy(gold[k])), k
    got = R.region_err(r32["raw"], ref64["raw"])
    for k, v in got.items():                                                            # the rest: to that float32 error
        assert v <= 2 * err[k], (k, v, err[k])
        assert R.scaled_err(r32["raw"][..., R.REGIONS[k]], raw[..., R.REGIONS[k]]) <= 2 * err[k], k
    bound = R.normalised_bound({k: 2 * v for k, v in err.items()}, ref64["raw"], ref64["scale_"][:, None, None],
                               ref64["min_"][:, None, None])
    assert bool(((r32["feats"].double() - torch.from_numpy(gold["feats_f32"]).double()).abs() <= bound).all())
    assert bool(((ref64["feats"] - torch.from_numpy(gold["feats_f32"]).double()).abs() <= bound).all())
    # test mode with the golden's normalizer
    t32 = R.process(pos, q, train=False, scale=gold["test_scale_"], min_=gold["test_min_"], dtype=torch.float32)
    want = torch.from_numpy(gold["test_feats_f32"])
    sc, mn = torch.from_numpy(gold["test_scale_"]), torch.from_numpy(gold["test_min_"])
    bound = R.normalised_bound({k: 2 * v for k, v in err.items()}, ref64["raw"], sc, mn)
    assert bool(((t32["feats"].double() - want.double()).abs() <= bound).all())
    assert torch.equal(t32["feats"].abs() == 1, want.abs() == 1)                        # the same elements clip


DEFECTS = {"backward_diff": ["contacts"], "right_multiply": ["rot6d_root"], "columns_6d": ["rot6d", "rot6d_root"],
           "pos_sign": ["root"], "fit_all_clips": ["stats", "feats"], "root6d_before": ["rot6d_root"]}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_emulated_defect_moves_its_region_past_the_gpu_bound(gold, ref64, defect):
    bad = R.process(*_inputs(gold), **{defect: True})
    bounds = R.raw_bounds(gold)
    for region in DEFECTS[defect]:
        if region == "contacts":                  # checked exactly on the GPU: any changed contact is caught
            assert int((bad["raw"][..., :4] != ref64["raw"][..., :4]).sum()) > 10
        elif region == "stats":                   # checked bit for bit on the GPU
            assert float((bad["scale_"] - ref64["scale_"]).abs().max()) > 1e-3
        elif region == "feats":
            nb = R.normalised_bound(bounds, ref64["raw"], ref64["scale_"][:, None, None], ref64["min_"][:, None, None])
            assert float(((bad["feats"] - ref64["feats"]).abs() / nb).max()) > 10
        else:
            s = R.REGIONS[region]
            moved = R.scaled_err(bad["raw"][..., s], ref64["raw"][..., s])
            assert moved > 10 * bounds[region], (defect, region, moved, bounds[region])
    for region, s in R.REGIONS.items():           # and nothing else moves
        if region not in DEFECTS[defect] and defect != "fit_all_clips":
            assert R.scaled_err(bad["raw"][..., s], ref64["raw"][..., s]) == 0, (defect, region)


# ---- the host build of fk_math.h ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ingest_host") / "ingest_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "host", "ingest_host.cpp")])
    lib = C.CDLL(so)
    for name in ("host_rot6_from_quat", "host_ax_to_6v", "host_root_yup_to_zup", "host_rotate_x90"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    return lib


def _call(fn, x, width):
    x = x.float().contiguous()
    out = torch.empty(x.shape[0], width)
    fn(x.data_ptr(), x.shape[0], out.data_ptr())
    return x.double(), out.double()


def test_host_build_of_the_ingest_functions_against_float64(gold, host):
    err = R.reference_error(gold)
    g = torch.Generator().manual_seed(3)
    n = 4096
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    aa = u / u.norm(dim=-1, keepdim=True) * torch.rand(n, 1, generator=g, dtype=torch.float64) * 3.1
    aa[:8] = 0.0
    aa[8:16] *= 1e-8                                                # the small-angle series
    # 6-D rows of a quaternion that is not of unit length (two_s carries the length)
    qn = torch.randn(n, 4, generator=g, dtype=torch.float64)
    x, out = _call(host.host_rot6_from_quat, qn, 6)
    assert float((out - R.matrix_to_rotation_6d(R.quaternion_to_matrix(x))).abs().max()) < 2e-6
    x, out = _call(host.host_ax_to_6v, aa, 6)
    want = R.matrix_to_rotation_6d(R.axis_angle_to_matrix(x))
    assert float((out - want).abs().max()) <= R.MARGIN * err["rot6d"]
    assert bool((out[:8] == torch.tensor([1.0, 0, 0, 0, 1, 0], dtype=torch.float64)).all())
    assert float((out - R.matrix_to_rotation_6d(R.axis_angle_to_matrix(x).transpose(-1, -2))).abs().max()) > 0.5   # not the columns
    # the root step: left multiplication by the float32 constant, standardised to w >= 0
    x, out = _call(host.host_root_yup_to_zup, aa, 3)
    rot = torch.tensor([0.7071068, 0.7071068, 0, 0]).double()       # float32(0.7071068), as the kernel holds it
    quat = O.quaternion_multiply(rot, O.axis_angle_to_quaternion(x))
    want = O.quaternion_to_axis_angle(quat)
    assert float(quat[:, 0].min()) >= 0 and int((O.quaternion_raw_multiply(rot, O.axis_angle_to_quaternion(x))[:, 0] < 0).sum()) > 100
    far = want.norm(dim=-1) < 3.0                                   # away from pi, where the axis is ill-conditioned
    assert int(far.sum()) > n // 2
    assert float((out - want)[far].abs().max()) < 1e-5
    right = O.quaternion_to_axis_angle(O.quaternion_multiply(O.axis_angle_to_quaternion(x), rot))
    assert float((right - want).abs().max()) > 0.5                  # not the right-hand product
    # the position rotation: float32 cosine and sine of float32(pi / 2), two rounded products and a rounded sum
    p = torch.randn(n, 3, generator=g, dtype=torch.float64) * 4
    x, out = _call(host.host_rotate_x90, p, 3)
    want32 = R.RotateAxisAngle(90, "X").transform_points(x.float())
    assert torch.equal(out.float(), want32)                         # bit for bit the float32 evaluation
    c = float(R.RotateAxisAngle(90, "X").cos)
    assert c == float(np.cos(np.float32(np.pi / 2))) and -4.4e-8 < c < -4.3e-8
    assert float((out - R.RotateAxisAngle(90, "X").transform_points(x)).abs().max()) < 5e-7
    assert float((out - R.RotateAxisAngle(-90, "X").transform_points(x)).abs().max()) > 1.0


# ---- the dataset's host side ----------------------------------------------------------------------------------------------
def _tree(root):
    """data/<train|test>/motions_sliced with one-, two- and three-dancer pickles, one clip without a feature file and one
    outside the split"""
    g = np.random.default_rng(0)
    spec = [("songA_slice0", 3, True), ("songA_slice1", 2, True), ("songB_x_slice0", 3, True), ("songB_x_slice1", 1, True),
            ("songC_slice0", 3, False), ("songD_slice0", 3, True), ("songA_slice10", 3, True)]
    for split in ("train", "test"):
        base = os.path.join(root, split)
        for d in ("motions_sliced", "feats438", "wavs_sliced"):
            os.makedirs(os.path.join(base, d))
        for name, dn, has_feat in spec:
            with open(os.path.join(base, "motions_sliced", name + ".pkl"), "wb") as f:
                pickle.dump({"pos": g.standard_normal((dn, 6, 3)).astype(np.float32),
                             "q": g.standard_normal((dn, 6, 72)).astype(np.float32)}, f)
            if has_feat:
                np.save(os.path.join(base, "feats438", name + ".npy"), g.standard_normal((6, 438)).astype(np.float32))
    return ["songA", "songB_x", "songC"]           # songD is outside the split


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("dancers", [3, 2])
def test_load_aioz_returns_the_reference_file_lists(tmp_path, train, dancers):
    split = _tree(str(tmp_path))
    ours = D.AIOZDataset.__new__(D.AIOZDataset)
    ours.data_path, ours.train, ours.split_file = str(tmp_path), train, split
    got = ours.load_aioz(dancers)
    base = os.path.join(str(tmp_path), "train" if train else "test")
    # sorted file order (slice10 before slice0's successor songB), features present, in the split, the dancer count
    names = ["songA_slice0", "songA_slice10", "songB_x_slice0"] if dancers == 3 else ["songA_slice1"]
    assert got["filenames"] == [os.path.join(base, "feats438", n + ".npy") for n in names]
    assert got["wavs"] == [os.path.join(base, "wavs_sliced", n + ".wav") for n in names]
    assert got["pos"].shape == (len(names), dancers, 6, 3) and got["q"].shape == (len(names), dancers, 6, 72)
    for k, n in enumerate(names):
        with open(os.path.join(base, "motions_sliced", n + ".pkl"), "rb") as f:
            d = pickle.load(f)
        assert np.array_equal(got["pos"][k], d["pos"]) and np.array_equal(got["q"][k], d["q"])
    if refload.available():                       # and the real reference's load_aioz on the same tree
        refload.load()
        import dataset.group_dataset as RG
        ref = RG.AIOZDataset.__new__(RG.AIOZDataset)
        ref.data_path, ref.train, ref.split_file = str(tmp_path), train, split
        want = ref.load_aioz(dancers)
        assert got["filenames"] == want["filenames"] and got["wavs"] == want["wavs"]
        assert np.array_equal(got["pos"], want["pos"]) and np.array_equal(got["q"], want["q"])


def test_process_motion_refuses_without_a_normalizer_or_a_gpu():
    pos, q = np.zeros((1, 2, 4, 3), np.float32), np.zeros((1, 2, 4, 72), np.float32)
    with pytest.raises(AssertionError):
        D.process_motion(pos, q, train=False, normalizer=None)
    if not torch.cuda.is_available():
        with pytest.raises(D.L.TcdiffError):
            D.process_motion(pos, q, train=True)


def test_normalizer_pkl_is_read_by_plain_pickle_under_the_reference_modules(tmp_path, gold):
    """a test-mode AIOZDataset writes normalizer.pkl before it loads anything (group_dataset.py:59-62); an empty split keeps
    the GPU out of this test.  A fresh interpreter without tcdiff_amd reads the file with plain pickle: under stand-in
    modules of the reference's names, and under the reference's own where its checkout is present."""
    _tree(str(tmp_path / "data"))
    norm = tio.Normalizer(torch.from_numpy(gold["raw_f32"]).reshape(-1, 151).clone())
    ds = D.AIOZDataset(str(tmp_path / "data"), str(tmp_path / "backup"), train=False, normalizer=norm, split_file=[])
    assert len(ds) == 0 and ds.normalizer is norm
    stub = tmp_path / "stub" / "dataset"
    stub.mkdir(parents=True)
    (stub / "__init__.py").write_text("")
    (stub / "preprocess.py").write_text("class Normalizer:\n    pass\n")
    (stub / "scaler.py").write_text("class MinMaxScaler:\n    pass\n")
    roots = [str(tmp_path / "stub")] + ([refload.REF] if refload.available() else [])
    for root in roots:
        code = ("import pickle, sys, torch\n"
                f"sys.path.insert(0, {root!r})\n"
                "import dataset.preprocess, dataset.scaler\n"
                f"n = pickle.load(open({str(tmp_path / 'backup' / 'normalizer.pkl')!r}, 'rb'))\n"
                "assert type(n) is dataset.preprocess.Normalizer and type(n.scaler) is dataset.scaler.MinMaxScaler\n"
                "assert 'tcdiff_amd' not in sys.modules\n"
                "assert n.scaler.clip and n.scaler.feature_range == (-1, 1)\n"
                "if hasattr(n, 'normalize'):\n"
                "    assert n.normalize(torch.zeros(1, 2, 151)).shape == (1, 2, 151)\n"
                "torch.save([n.scaler.scale_, n.scaler.min_], sys.argv[1])\n")
        subprocess.check_call([sys.executable, "-c", code, str(tmp_path / "back.pt")], cwd=str(tmp_path))
        sc, mn = torch.load(str(tmp_path / "back.pt"))
        assert torch.equal(sc, norm.scaler.scale_) and torch.equal(mn, norm.scaler.min_)
