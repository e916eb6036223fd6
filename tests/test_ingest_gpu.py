"""tcdiff_motion_ingest (csrc/ingest.hip) and tcdiff_amd/dataset.py on an MI355X, against the float64 restatement
tests/ingest_ref.py.  They read only tests/golden/.

Cases (the smallest at which the kernels can go wrong): the golden's 3 clips x 2 dancers x 20 frames (120 poses: the pose
kernel's last block is partial; 40 rows per clip: less than one workgroup), 1 x 3 x 150 (450 rows: several passes of the
workgroup per clip) and 2 x 1 x 1 (a single frame: every contact 1, every range 0).

The raw bounds are ingest_ref.MARGIN (8) x the error of the reference's own float32 run against its float64 run, region by
region, both in tests/golden/ingest.npz (root 4.6e-07, rot6d_root 3.3e-06, rot6d 2.2e-06 in scaled_err's measure); contacts and
the fitted statistics are exact.  Observed on an MI355X: see profiles/ingest.txt."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import export_ref as XR
import ingest_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import dataset as D
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATS = ("data_min_", "data_max_", "scale_", "min_")
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ingest.npz")))


@pytest.fixture(scope="module")
def bounds(gold):
    return R.raw_bounds(gold)


def _normalizer(scale, min_):
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_, n.scaler.min_ = torch.as_tensor(scale).float(), torch.as_tensor(min_).float()
    return n


@pytest.fixture(scope="module")
def cases(gold):
    """{name: (pos, q, float64 reference)}: computed once, never modified"""
    s = float(gold["input_scale"])
    out = {"3x2x20": (torch.from_numpy(gold["pos"]).double() * s, torch.from_numpy(gold["q"]).double() * s)}
    out["1x3x150"] = R.synth_clear(1, 3, 150, 31)[:2]
    out["2x1x1"] = R.synth_clear(2, 1, 1, 32)[:2]
    return {k: (p, q, R.process(p, q)) for k, (p, q) in out.items()}


CASES = ["3x2x20", "1x3x150", "2x1x1"]


def _report(what, obs, bounds):
    print(f"[ingest] {what}: " + ", ".join(f"{k} {v:.2e} / {bounds[k]:.1e}" for k, v in obs.items()))


@pytest.mark.parametrize("case", CASES)
def test_train_mode_against_float64(cases, bounds, case):
    pos, q, ref = cases[case]
    clips, dn, sq, _ = pos.shape
    feats, norm, st, raw = D.process_motion(pos.float().to(DEV), q.float().to(DEV), train=True, return_raw=True)
    torch.cuda.synchronize()
    assert feats.shape == raw.shape == (clips, dn, sq, 151) and feats.dtype == torch.float32 and feats.is_cuda
    raw_c, feats_c = raw.cpu(), feats.cpu()
    # contacts: exact; the last frame is always 1
    assert torch.equal(raw_c[..., :4].double(), ref["raw"][..., :4])
    assert bool((raw_c[:, :, -1, :4] == 1).all())
    # data_min_ / data_max_: torch.min / torch.max of the kernel's own raw rows, bit for bit
    rows = raw.reshape(clips, dn * sq, 151)
    lo, hi = rows.min(dim=1)[0].cpu(), rows.max(dim=1)[0].cpu()
    assert torch.equal(st["data_min_"].cpu(), lo) and torch.equal(st["data_max_"].cpu(), hi)
    # scale_ / min_: the reference's formula (dataset/scaler.py:63-67) on those statistics, bit for bit
    rng = hi - lo
    rng = torch.where(rng < 10 * torch.finfo(torch.float32).eps, torch.ones_like(rng), rng)
    scale = 2 / rng
    prod = lo * scale
    min_ = -1 - prod
    assert torch.equal(st["scale_"].cpu(), scale) and torch.equal(st["min_"].cpu(), min_)
    if case == "2x1x1":
        # one row per clip: every range 0 -> divisor 1, scale_ 2, min_ = -1 - 2 x; a contact of 1 normalises to exactly
        # 2 - 3 = -1 (the other columns to -1 within the rounding of min_, which the bound below covers)
        assert bool((scale == 2).all()) and bool((raw_c[..., :4] == 1).all()) and bool((feats_c[..., :4] == -1).all())
    else:
        assert int((hi - lo == 0).sum()) >= 6           # the joint held at zero: range exactly 0 -> divisor 1
    # the returned normalizer is the last clip's
    for k in STATS:
        assert torch.equal(getattr(norm.scaler, k), st[k][-1].cpu()), k
    assert norm.scaler.n_samples_seen_ == dn * sq and not norm.scaler.scale_.is_cuda
    # raw root and 6-D against float64, region by region
    obs = R.region_err(raw_c, ref["raw"])
    _report(f"{case} raw vs float64", obs, bounds)
    for k, v in obs.items():
        assert v <= bounds[k], (case, k, v, bounds[k])
    # normalised features: the float64 transform with the kernel's statistics
    sc, mn = st["scale_"].cpu().double()[:, None, None], st["min_"].cpu().double()[:, None, None]
    want = R.transform(ref["raw"], sc, mn)
    nb = R.normalised_bound(bounds, ref["raw"], sc, mn)
    ratio = float(((feats_c.double() - want).abs() / nb).max())
    print(f"[ingest] {case} normalised: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (case, ratio)
    assert float(feats_c.min()) >= -1 and float(feats_c.max()) <= 1


def test_train_mode_against_the_reference_golden(gold, bounds):
    """the kernel against the real reference's float32 run: the same contacts, statistics and features to both runs' bounds"""
    s = float(gold["input_scale"])
    pos, q = torch.from_numpy(gold["pos"]).float() * s, torch.from_numpy(gold["q"]).float() * s
    feats, norm, st, raw = D.process_motion(pos, q, train=True, return_raw=True)
    want_raw = torch.from_numpy(gold["raw_f32"])
    assert torch.equal(raw.cpu()[..., :4], want_raw[..., :4])
    err = R.reference_error(gold)
    for k, sl in R.REGIONS.items():
        assert R.scaled_err(raw.cpu()[..., sl], want_raw[..., sl]) <= bounds[k] + err[k], k
    both = {k: bounds[k] + err[k] for k in bounds}
    sc, mn = torch.from_numpy(gold["scale_"])[:, None, None], torch.from_numpy(gold["min_"])[:, None, None]
    nb = R.normalised_bound(both, want_raw, sc, mn)
    # y = 2 (x - lo) / range - 1: with e the raw error, x moves y by e scale_, lo by e scale_ and the range (2 e) by
    # (y + 1) e scale_ <= 2 e scale_ -- four times the raw term, and the float32 roundings of scale_ and min_ on top
    assert bool(((feats.cpu().double() - torch.from_numpy(gold["feats_f32"]).double()).abs() <= 5 * nb).all())
    for k in ("data_min_", "data_max_"):
        assert bool(((st[k].cpu().double() - torch.from_numpy(gold[k]).double()).abs()
                     <= max(both.values()) * torch.from_numpy(gold[k]).double().abs().clamp(min=1)).all()), k


@pytest.mark.parametrize("case", ["3x2x20", "1x3x150"])
def test_test_mode_with_the_golden_normalizer(gold, cases, bounds, case):
    pos, q, ref = cases[case]
    norm = _normalizer(gold["test_scale_"], gold["test_min_"])
    feats, back, st = D.process_motion(pos.float().to(DEV), q.float().to(DEV), train=False, normalizer=norm)
    assert back is norm and torch.equal(st["scale_"].cpu()[0], norm.scaler.scale_)
    sc, mn = norm.scaler.scale_.double(), norm.scaler.min_.double()
    want = R.transform(ref["raw"], sc, mn)
    nb = R.normalised_bound(bounds, ref["raw"], sc, mn)
    got = feats.cpu().double()
    ratio = float(((got - want).abs() / nb).max())
    print(f"[ingest] {case} test mode: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # values outside the given normalizer's range come out as exactly +-1
    pre = ref["raw"] * sc + mn
    above, below = pre > 1 + nb, pre < -1 - nb
    assert int(above.sum()) > 500 and int(below.sum()) > 500
    assert bool((got[above] == 1).all()) and bool((got[below] == -1).all())
    assert float(got.abs().max()) == 1.0
    if case == "3x2x20":                              # and the real reference's test-mode run
        ref_feats = torch.from_numpy(gold["test_feats_f32"]).double()
        err = R.reference_error(gold)
        nb2 = R.normalised_bound({k: bounds[k] + err[k] for k in bounds}, torch.from_numpy(gold["raw_f32"]), sc, mn)
        assert bool(((got - ref_feats).abs() <= nb2).all())


@pytest.mark.parametrize("fit", [True, False])
def test_sentinels_after_every_output_and_inputs_unchanged(cases, fit):
    pos, q, _ = cases["3x2x20"]
    clips, dn, sq, _ = pos.shape
    P = clips * dn * sq
    pos_d, q_d = pos.float().to(DEV).contiguous(), q.float().to(DEV).contiguous()
    pos_0, q_0 = pos_d.clone(), q_d.clone()
    pad = 256
    sizes = {"feats": P * 151, "raw": P * 151, "feet": P * 12, "stats": clips * 4 * 151}
    buf = {k: torch.full((n + pad,), SENTINEL, device=DEV) for k, n in sizes.items()}
    sc, mn = torch.full((151,), 0.5, device=DEV), torch.zeros(151, device=DEV)
    K.motion_ingest(pos_d, q_d, clips, dn, sq, SMPL_PARENTS, SMPL_OFFSETS, fit, None if fit else sc, None if fit else mn,
                    buf["feats"], buf["raw"], buf["feet"], buf["stats"])
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert bool((buf[k][n:] == SENTINEL).all()), k
        written = bool((buf[k][:n] != SENTINEL).all())
        assert written == (fit or k != "stats"), k              # stats is written in fit mode only
    assert torch.equal(pos_d, pos_0) and torch.equal(q_d, q_0)


def test_host_inputs_give_the_device_result_and_stay_unchanged(cases):
    pos, q, _ = cases["3x2x20"]
    pos_n, q_n = pos.float().numpy().copy(), q.float().numpy().copy()
    pos_0, q_0 = pos_n.copy(), q_n.copy()
    a = D.process_motion(pos_n, q_n, train=True, return_raw=True)
    b = D.process_motion(torch.from_numpy(pos_n).to(DEV), torch.from_numpy(q_n).to(DEV), train=True, return_raw=True)
    c = D.process_motion(torch.from_numpy(pos_n), torch.from_numpy(q_n).double(), train=True, return_raw=True)
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[3], other[3]) and a[0].is_cuda
        for k in STATS:
            assert torch.equal(a[2][k], other[2][k]) and torch.equal(getattr(a[1].scaler, k), getattr(other[1].scaler, k))
    assert np.array_equal(pos_n, pos_0) and np.array_equal(q_n, q_0)
    # data_len slices the dancer axis (group_dataset.py:227-228)
    d = D.process_motion(pos_n, q_n, train=True, data_len=1, return_raw=True)
    assert d[0].shape == (3, 1, 20, 151) and torch.equal(d[0], a[0][:, :1]) and torch.equal(d[3], a[3][:, :1])
    assert torch.equal(d[2]["scale_"], a[2]["scale_"])           # fitted on every dancer, as the reference fits before slicing
    with pytest.raises(AssertionError):
        D.process_motion(pos_n, q_n, train=False, normalizer=None)
    with pytest.raises(L.TcdiffError):
        D.process_motion(pos_n[..., :2], q_n, train=True)


def test_argument_refusals():
    clips, dn, sq = 2, 2, 5
    P = clips * dn * sq
    pos, q = torch.zeros(P, 3, device=DEV), torch.zeros(P, 72, device=DEV)
    feats, raw, feet, stats = (torch.empty(n, device=DEV) for n in (P * 151, P * 151, P * 12, clips * 4 * 151))
    sc, mn = torch.ones(151, device=DEV), torch.zeros(151, device=DEV)
    ok = dict(pos=pos, q=q, clips=clips, dn=dn, sq=sq, parents=SMPL_PARENTS, offsets=SMPL_OFFSETS, fit=True, scale=None, min_=None,
              feats=feats, raw=raw, feet=feet, stats=stats)
    K.motion_ingest(**ok)
    K.motion_ingest(**{**ok, "raw": None})                        # raw is optional
    K.motion_ingest(**{**ok, "fit": False, "scale": sc, "min_": mn, "stats": None})
    torch.cuda.synchronize()
    bad = [dict(pos=None), dict(q=None), dict(feats=None), dict(feet=None), dict(stats=None), dict(clips=0), dict(dn=0),
           dict(sq=0), dict(clips=-1), dict(parents=[0] * 24), dict(parents=[-1, 2, 0] + SMPL_PARENTS[3:]),
           dict(fit=False), dict(fit=False, scale=sc), dict(fit=False, min_=mn)]
    for change in bad:
        with pytest.raises(L.TcdiffError):
            K.motion_ingest(**{**ok, **change})
    lib = L.load()
    assert lib.tcdiff_motion_ingest(pos.data_ptr(), q.data_ptr(), clips, dn, sq, None, None, 1, None, None, feats.data_ptr(), None,
                                    feet.data_ptr(), stats.data_ptr(), None) == -1


def _short_way(aa):
    """the same rotations with angles in [0, pi].  The export's matrix_to_quaternion selects the candidate with the largest
    component, which may have w < 0, and quaternion_to_axis_angle then returns the angle 2 pi - theta about the opposite
    axis: the same rotation, written the long way round.  The inputs stay below 2.5 rad, so the short way is unambiguous."""
    aa = aa.double().cpu()
    ang = aa.norm(dim=-1, keepdim=True)
    return torch.where(ang > torch.pi, aa * (1 - 2 * torch.pi / ang.clamp(min=1.0)), aa)


@pytest.mark.parametrize("case", ["3x2x20", "1x3x150"])
def test_round_trip_through_the_pose_export(cases, bounds, case):
    """raw motion -> features (test mode, a normalizer wide enough that nothing clips) -> export_poses(mode="normal") -> the
    Z-up root positions, every joint's axis-angle, the FK joints and the contacts, against the float64 restatement.

    Bounds: the export tests' own per-region bounds (export_ref.BOUNDS, scaled_err's measure) plus what the ingest adds.  A
    feature column carries the ingest's raw bound r (times max(1, |raw|)) plus two float32 ulps of a normalised value
    (<= 2^-23 each) which the export divides by that column's scale_: d = r max(1, |raw|) + 2^-22 / scale_.  Root: d of the root
    columns.  Axis-angle: a 6-D error d moves the rotation vector by at most 4 d for angles below 2.5 rad (|d theta| <=
    sqrt(6) d / sinc(theta / 2), rounded up).  Joints: the root's d plus the axis-angle addition times the longest chain of
    bones (1.6 m).  Contacts: 0 / 1 to the export's contact bound plus 2^-22 / scale_."""
    pos, q, ref = cases[case]
    clips, dn, sq, _ = pos.shape
    raw = ref["raw"].reshape(-1, 151)
    lo, hi = raw.min(dim=0)[0], raw.max(dim=0)[0]
    wide = tio.Normalizer(torch.stack([lo - 0.25 * (hi - lo) - 0.25, hi + 0.25 * (hi - lo) + 0.25]).float())
    feats, _, _ = D.process_motion(pos.float().to(DEV), q.float().to(DEV), train=False, normalizer=wide)
    assert float(feats.abs().max()) < 1.0                        # nothing clips
    x = feats.permute(0, 2, 1, 3).reshape(clips, sq * dn, 151)   # frame-major, as the samplers return rows
    got_q, got_pos, got_joints, got_contact = E.export_poses(x, wide, "normal", dn)
    torch.cuda.synchronize()
    scale = wide.scaler.scale_.double()
    col = torch.zeros(151, dtype=torch.float64)
    for k, sl in R.REGIONS.items():
        col[sl] = bounds[k]
    d = col * raw.abs().max(dim=0)[0].clamp(min=1.0) + 2.0 ** -22 / scale
    add_root, add_6d = float(d[4:7].max()), float(d[7:].max())
    add_aa = 4 * add_6d
    bound = {"root": XR.BOUNDS["root"] + add_root, "axis_angle": XR.BOUNDS["axis_angle"] + add_aa,
             "joints": XR.BOUNDS["joints"] + add_root + 1.6 * add_aa, "contact": XR.BOUNDS["contact"] + float(d[:4].max())}
    fm = lambda t: t.permute(0, 2, 1, *range(3, t.dim())).reshape((clips, sq * dn) + tuple(t.shape[3:]))   # -> frame-major
    obs = {"root": XR.scaled_err(got_pos, fm(ref["root"])), "axis_angle": XR.scaled_err(_short_way(got_q), fm(ref["aa"])),
           "joints": XR.scaled_err(got_joints, ref["joints"]), "contact": XR.scaled_err(got_contact, ref["raw"][..., :4])}
    print(f"[ingest] {case} round trip: " + ", ".join(f"{k} {v:.2e} / {bound[k]:.1e}" for k, v in obs.items()))
    for k, v in obs.items():
        assert v <= bound[k], (case, k, v, bound[k])
    assert float(ref["aa"].norm(dim=-1).max()) < 2.5
    c = got_contact.cpu()
    assert bool(((c - c.round()).abs() <= bound["contact"]).all()) and set(c.round().unique().tolist()) == {0.0, 1.0}


def test_aioz_dataset_end_to_end(tmp_path):
    """AIOZDataset on a temporary tree: items of the reference's shapes and types, a picklable object, and a batch that
    diffusion(x, cond) accepts (one small model, no parity claim)."""
    from oracle import tcdiff_oracle as O
    from tcdiff_amd import AIOZDataset, DanceDecoder, GaussianDiffusion
    dn, S = 2, 60
    names = ["songA_slice0", "songA_slice1", "songB_slice0"]
    for split in ("train", "test"):
        base = tmp_path / "data" / split
        for sub in ("motions_sliced", "feats438", "wavs_sliced"):
            (base / sub).mkdir(parents=True)
        for k, n in enumerate(names):
            pos, q = R.synth_motion(1, dn if k < 2 else 3, S, 40 + k)
            with open(base / "motions_sliced" / (n + ".pkl"), "wb") as f:
                pickle.dump({"pos": pos[0].float().numpy(), "q": q[0].float().numpy()}, f)
            np.save(base / "feats438" / (n + ".npy"), O.synth_cond(k, S).numpy())
    train = AIOZDataset(str(tmp_path / "data"), str(tmp_path / "backup"), train=True, required_dancer_num=dn,
                        split_file=["songA", "songB"])
    assert len(train) == train.length == 2 and isinstance(train.normalizer, tio.Normalizer)
    assert type(train.data["pose"]) is np.ndarray and train.data["pose"].shape == (2, dn, S, 151)
    assert train.data["pose"].dtype == np.float32
    pose, feature, filename, wav = train[1]
    assert pose.shape == (dn, S, 151) and feature.shape == (2 * S + 1, 438) and feature.dtype == torch.float32
    assert filename.endswith(os.path.join("train", "feats438", "songA_slice1.npy"))
    assert wav.endswith(os.path.join("train", "wavs_sliced", "songA_slice1.wav"))
    test = AIOZDataset(str(tmp_path / "data"), str(tmp_path / "backup"), train=False, normalizer=train.normalizer,
                       required_dancer_num=dn, split_file=["songA", "songB"])
    assert test.normalizer is train.normalizer and os.path.exists(tmp_path / "backup" / "normalizer.pkl")
    back = pickle.loads(pickle.dumps(train))                      # TCDiff.py:343-344 pickles the dataset
    assert np.array_equal(back.data["pose"], train.data["pose"])
    # the last clip's rows normalised with the last clip's own fit: the same in both datasets
    assert np.array_equal(test.data["pose"][1], train.data["pose"][1])
    loader = torch.utils.data.DataLoader(train, batch_size=2)
    x, cond, fnames, wavs = next(iter(loader))
    assert x.shape == (2, dn, S, 151) and cond.shape == (2, 2 * S + 1, 438) and len(fnames) == 2
    sd = O.synth_state_dict(dn=dn, seq_len=S)
    model = DanceDecoder(nfeats=151, seq_len=S, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=F.gelu, required_dancer_num=dn)
    model.load_state_dict(sd)
    diff = GaussianDiffusion(model, S, 151, None, schedule="cosine", n_timestep=100, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=S).to(DEV).train()
    total, losses = diff(x.to(DEV), cond.to(DEV))
    assert len(losses) == 4 and bool(torch.isfinite(total))
