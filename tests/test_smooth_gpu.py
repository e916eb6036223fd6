"""The jitter scores and the rotation filter on the GPU (tcdiff_amd/smooth.py, csrc/smooth.hip) against the float64 restatement
tests/smooth_ref.py of include/tcdiff_smooth.h, and against what they are for: on a seeded noisy dance the jitter falls and the
joints come closer to the clean motion.  The joints are held to a forward kinematics written separately here (rotation matrices,
float64) of the float32 poses the launch returns.

Measured on an MI355X (profiles/smooth.txt): root positions equal bits on every case; rotations at most 1.0e-7 rad from the
restatement (bound 1e-6); joints at most 8.4e-7 m from the float64 FK (bound 1e-5); max_rot_change at most 2e-16 relative, every
other float64 statistic and score 0 away."""
import importlib
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import smooth_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import footlock as F
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS

S = importlib.import_module("tcdiff_amd.smooth")                   # the package's attribute of this name is the function
pytestmark = pytest.mark.gpu
DEV = "cuda"
ROT_BOUND, FK_BOUND = R.ROT_BOUND, R.FK_BOUND          # in tests/smooth_ref.py: tests/test_post_chain_gpu.py holds the chain to the same two
MASK_16_23 = sum(1 << j for j in range(16, 24))
# name -> (b, dn, T, keywords): all edge rows with no or one interior frame, the tile boundary, two tiles and a tail, the largest LDS
# footprint, the smallest window, two clips, one to three dancers, another root window, a mask
CASES = {"T9": (1, 2, 9, {}), "T10": (1, 1, 10, {}), "T64": (1, 3, 64, {}), "T65": (2, 2, 65, {}), "T130": (2, 3, 130, {}),
         "W63-T63": (1, 2, 63, dict(window=63)), "W63-T150": (1, 3, 150, dict(window=63)), "W3": (1, 2, 20, dict(window=3, polyorder=1)),
         "root21": (2, 3, 65, dict(root_window=21)), "mask16-23": (1, 2, 40, dict(joints_mask=MASK_16_23))}


# ---- a forward kinematics of its own: Rodrigues matrices, whole arrays at once ---------------------------------------------------------------
def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r, axis=-1)[..., None, None]
    Kx = np.zeros(r.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -r[..., 2], r[..., 1], r[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -r[..., 0], -r[..., 1], r[..., 0]
    small = th < 1e-6
    s = np.where(small, 1.0 - th ** 2 / 6, np.sin(th) / np.where(small, 1.0, th))
    c = np.where(small, 0.5 - th ** 2 / 24, (1 - np.cos(th)) / np.where(small, 1.0, th) ** 2)
    return np.eye(3) + s * Kx + c * (Kx @ Kx)


def fk64(q, pos):
    local = rodrigues(q)
    off = np.asarray(SMPL_OFFSETS, np.float32).astype(np.float64)
    P, W = [None] * 24, [None] * 24
    for j in range(24):
        p = SMPL_PARENTS[j]
        if p < 0:
            P[j], W[j] = np.asarray(pos, np.float64), local[..., j, :, :]
        else:
            P[j] = P[p] + W[p] @ off[j]
            W[j] = W[p] @ local[..., j, :, :]
    return np.stack(P, -2)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared cases are read-only


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a: S.Smooth, b: S.Smooth):
    flat = lambda s: list(s[:6]) + [v for side in (s.before, s.after) if side is not None for v in side.values()]
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(flat(a), flat(b))) and a[6:8] == b[6:8]


def relative(got, want):
    """the largest relative difference of two float64 arrays whose NaNs must coincide"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float((np.abs(got - want)[ok] / np.maximum(np.abs(want[ok]), 1e-300)).max())


def check_scores(got: dict, joints, what):
    """a smoothness dict off the device against the restatement's of the same float32 joints"""
    ref = R.smoothness(joints)
    assert list(got) == ["accel_mean", "jitter", "jitter_local", "root_jitter", "accel_max", "jitter_max", "accel_peak", "jitter_peak", "terms"]
    worst = 0.0
    for k in R.FLOATS:
        assert got[k].dtype == torch.float64 and tuple(got[k].shape) == ref[k].shape
        worst = max(worst, relative(got[k].cpu().numpy(), ref[k]))
    for k in R.INTS:
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), ref[k]), k
    print(f"[smooth] {what}: scores {worst:.1e} (relative) from the restatement, 0 expected (bound 1e-12)")
    assert worst <= 1e-12
    return worst


def check_against(out: S.Smooth, q, pos, dn, ref, what):
    """every output of one call against the restatement `ref` of the inputs q, pos (numpy float32)"""
    got_q, got_pos = out.q.cpu().numpy(), out.pos.cpu().numpy()
    assert got_q.shape == q.shape and got_pos.shape == pos.shape and got_q.dtype == got_pos.dtype == np.float32
    assert np.array_equal(got_pos.view(np.int32), ref["pos"].view(np.int32))                 # the root: equal bits
    keep = R.rows_of(ref["copied_q"] | ~np.array([(ref_mask(ref) >> j) & 1 == 1 for j in range(24)])[None, None, None])
    assert np.array_equal(got_q.view(np.int32)[keep], q.view(np.int32)[keep])                 # copied and masked-out joints: the input's words
    with np.errstate(invalid="ignore"):
        ang = R.angles(got_q.astype(np.float64), ref["q64"])
    err = float(ang[~keep].max()) if (~keep).any() else 0.0
    assert np.isfinite(ang[~keep]).all()
    joints = out.joints.cpu().numpy()
    b, T = q.shape[0], q.shape[1] // dn
    assert joints.shape == (b, dn, T, 24, 3) and joints.dtype == np.float32
    with np.errstate(invalid="ignore"):
        fk_err = np.abs(joints - fk64(R.frames_of(got_q, dn), R.frames_of(got_pos, dn)))
    fk_worst = float(np.nanmax(fk_err))
    st = R.stats(q, pos, got_q, got_pos, dn)                                                # of the float32 values as stored
    e_rot, e_pos = relative(out.max_rot_change.cpu().numpy(), st["max_rot_change"]), relative(out.max_pos_change.cpu().numpy(), st["max_pos_change"])
    print(f"[smooth] {what}: rotations {err:.2e} rad from the restatement (bound {ROT_BOUND:g}), joints {fk_worst:.2e} m from a float64 FK "
          f"(bound {FK_BOUND:g}), max_rot_change {e_rot:.1e} and max_pos_change {e_pos:.1e} (relative, bound 1e-12)")
    assert err <= ROT_BOUND and fk_worst <= FK_BOUND and e_rot <= 1e-12 and e_pos <= 1e-12
    assert out.max_rot_change.dtype == out.max_pos_change.dtype == torch.float64 and out.copied.dtype == torch.int32
    assert tuple(out.copied.shape) == (b, dn) and np.array_equal(out.copied.cpu().numpy(), ref["copied"])
    if out.before is not None:
        check_scores(out.after, joints, what + ", after")
        raw = input_joints(q, pos, dn, out, ref_mask(ref))                                                # Smooth does not carry them: the launcher, called again
        with np.errstate(invalid="ignore"):
            assert np.nanmax(np.abs(raw.cpu().numpy() - fk64(R.frames_of(q, dn), R.frames_of(pos, dn)))) <= FK_BOUND
        again = S.smoothness(raw)
        assert all(torch.equal(bits(out.before[k]), bits(again[k])) for k in again)
        check_scores(out.before, raw.cpu().numpy(), what + ", before")
    return err, fk_worst


def input_joints(q, pos, dn, out: S.Smooth, mask):
    """the launcher's `joints_in` of the call that gave `out`, with every other output held to `out`'s bits"""
    b, T = q.shape[0], q.shape[1] // dn
    tq, tpos = dev(q), dev(pos)
    ws = torch.empty(K.smooth_workspace(b, dn, T), dtype=torch.uint8, device=DEV)
    q_out, pos_out = torch.empty_like(tq), torch.empty_like(tpos)
    joints, joints_in = torch.empty(b, dn, T, 24, 3, device=DEV), torch.empty(b, dn, T, 24, 3, device=DEV)
    rot, shift = torch.empty(b, dn, dtype=torch.float64, device=DEV), torch.empty(b, dn, dtype=torch.float64, device=DEV)
    copied = torch.empty(b, dn, dtype=torch.int32, device=DEV)
    K.smooth(tq, tpos, b, dn, T, out.window[0], S._table_on(out.window[0], out.polyorder[0], tq.device), out.window[1],
             S._table_on(out.window[1], out.polyorder[1], tq.device), mask, SMPL_PARENTS, SMPL_OFFSETS, ws, q_out, pos_out, joints,
             joints_in, rot, shift, copied)
    for a, c in ((q_out, out.q), (pos_out, out.pos), (joints, out.joints), (rot, out.max_rot_change), (shift, out.max_pos_change), (copied, out.copied)):
        assert torch.equal(bits(a), bits(c))
    return joints_in


def ref_mask(ref):
    return ref.get("mask", R.ALL)


def reference(q, pos, dn, **kw):
    ref = R.smooth(q, pos, dn, **kw)
    ref["mask"] = kw.get("joints_mask", R.ALL)
    return ref


# ---- against the restatement, at the shapes at which the tiling and the edge rows can go wrong ---------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_smooth_against_the_restatement(name):
    b, dn, T, kw = CASES[name]
    _, _, q, pos = R.noisy_case(b=b, dn=dn, T=T, seed=11)
    tq, tpos = dev(q), dev(pos)
    q0, p0 = tq.clone(), tpos.clone()
    out = S.smooth(tq, tpos, dn=dn, **kw)
    assert isinstance(out, S.Smooth) and torch.equal(bits(tq), bits(q0)) and torch.equal(bits(tpos), bits(p0))      # the inputs are not written
    assert out.q.data_ptr() != tq.data_ptr() and out.window == (kw.get("window", 9), kw.get("root_window", kw.get("window", 9)))
    assert out.polyorder == (kw.get("polyorder", 3),) * 2
    check_against(out, q, pos, dn, reference(q, pos, dn, **kw), name)
    assert same_bits(out, S.smooth(tq, tpos, dn=dn, **kw))                                  # two calls, equal bits in every output
    bare = S.smooth(tq, tpos, dn=dn, measure=False, **kw)
    assert bare.before is None and bare.after is None and same_bits(bare, out._replace(before=None, after=None))
    if name == "mask16-23":
        assert torch.equal(bits(out.q[:, :, :16]), bits(tq[:, :, :16])) and not torch.equal(out.q[:, :, 16:], tq[:, :, 16:])
        assert torch.equal(bits(S.smooth(tq, tpos, dn=dn, joints_mask=range(16, 24), measure=False).q), bits(out.q))
    if name == "root21":
        assert not torch.equal(out.pos, S.smooth(tq, tpos, dn=dn, measure=False).pos)


def test_a_rotation_vector_that_flips_sign_is_filtered_across_the_flip():
    q, pos, ang, axis = R.flip_case()
    out = S.smooth(dev(q), dev(pos), dn=1)
    got = out.q.cpu().numpy().astype(np.float64)
    err = float(R.angles(got[0, :, 3], ang[:, None] * axis[None]).max())
    print(f"[smooth] sign flip: {err:.2e} rad from the clean rotation (bound 1e-3)")
    assert err <= 1e-3
    check_against(out, q, pos, 1, reference(q, pos, 1), "sign flip")


def test_non_finite_inputs_are_copied_through_and_nothing_else():
    b, dn, T = 2, 2, 40
    _, _, qn, pn = R.noisy_case(b=b, dn=dn, T=T, seed=12)
    q, pos = np.array(qn), np.array(pn)
    q[0, 20 * dn + 1, 5, 2] = np.nan                       # clip 0, dancer 1, frame 20 > W, joint 5
    pos[1, 11 * dn + 0, 1] = np.inf                        # clip 1, dancer 0, frame 11
    ref = reference(q, pos, dn)
    want_q = np.zeros((b, dn, T, 24), bool)
    want_q[0, 1, 16:25, 5] = True
    want_p = np.zeros((b, dn, T), bool)
    want_p[1, 0, 7:16] = True
    assert np.array_equal(ref["copied_q"], want_q) and np.array_equal(ref["copied_pos"], want_p)      # exactly the windows that hold them
    out = S.smooth(dev(q), dev(pos), dn=dn)
    check_against(out, q, pos, dn, ref, "non-finite")
    assert out.copied.cpu().tolist() == [[0, 9], [9, 0]]
    got_q, got_pos = out.q.cpu().numpy(), out.pos.cpu().numpy()
    assert np.array_equal(~np.isfinite(got_q), ~np.isfinite(q)) and np.array_equal(~np.isfinite(got_pos), ~np.isfinite(pos))
    fq, fp = R.frames_of(got_q, dn), R.frames_of(got_pos, dn)
    assert np.array_equal(fq.view(np.int32)[want_q], R.frames_of(q, dn).view(np.int32)[want_q])
    assert np.array_equal(fp.view(np.int32)[want_p], R.frames_of(pos, dn).view(np.int32)[want_p])
    assert not np.array_equal(fq[~want_q], R.frames_of(q, dn)[~want_q])
    for side in (out.before, out.after):
        assert all(bool(torch.isfinite(side[k]).all()) for k in R.FLOATS)
    assert bool(torch.isfinite(out.max_rot_change).all()) and bool(torch.isfinite(out.max_pos_change).all())


# ---- the scores ----------------------------------------------------------------------------------------------------------------------------------
def test_smoothness_reads_a_permuted_view_in_place():
    b, dn, T = 2, 3, 70
    _, _, q, pos = R.noisy_case(b=b, dn=dn, T=T, seed=13)
    J = fk64(q.reshape(b, T, dn, 24, 3), pos.reshape(b, T, dn, 3)).astype(np.float32)          # frame-major, as the export's launch writes it
    frame_major = dev(J)
    view = frame_major.permute(0, 2, 1, 3, 4)
    assert not view.is_contiguous() and tuple(view.shape) == (b, dn, T, 24, 3)
    a, c = S.smoothness(view), S.smoothness(view.contiguous())
    assert all(torch.equal(bits(a[k]), bits(c[k])) for k in a)
    check_scores(a, np.moveaxis(J, 1, 2), "a permuted view")
    at60 = S.smoothness(view, fps=60)
    assert np.allclose(at60["jitter"].cpu().numpy(), 8 * a["jitter"].cpu().numpy(), rtol=1e-12)
    from tcdiff_amd.metrics import summarize
    s = summarize(a)
    assert set(s) == set(a) and all(np.isfinite(v) for v in s.values())


def test_smoothness_of_hand_made_tracks_and_of_four_frames():
    P = np.zeros((1, 2, 8, 24, 3), np.float32)
    P[0, 0, 5, 7, 2] = P[0, 0, 5, 3, 2] = P[0, 0, 3, 9, 2] = 0.5      # three equal kinks: the lower frame, then the lower joint
    P[0, 1] = np.nan                                                  # a dancer without a finite term
    got = S.smoothness(dev(P))
    check_scores(got, P, "hand-made")
    assert got["accel_peak"][0, 0].tolist() == [3, 9] and got["accel_peak"][0, 1].tolist() == [-1, -1] and int(got["terms"][0, 1]) == 0
    assert bool(torch.isnan(got["jitter"][0, 1])) and bool(torch.isnan(got["accel_max"][0, 1]))
    _, _, q, pos = R.noisy_case(b=1, dn=1, T=4, seed=14)
    J4 = fk64(R.frames_of(q, 1), R.frames_of(pos, 1)).astype(np.float32)
    check_scores(S.smoothness(dev(J4)), J4, "T = 4")


# ---- what it is for ------------------------------------------------------------------------------------------------------------------------------
def test_the_jitter_falls_and_the_motion_comes_closer_to_the_clean_one():
    dn = 3
    qc, pc, qn, pn = R.noisy_case(b=1, dn=dn, T=150, seed=1)
    out = S.smooth(dev(qn), dev(pn), dn=dn)
    before, after = out.before["jitter"].cpu().numpy(), out.after["jitter"].cpu().numpy()
    clean = fk64(R.frames_of(qc, dn), R.frames_of(pc, dn))
    rms = lambda q, pos: np.sqrt(((fk64(R.frames_of(q, dn), R.frames_of(pos, dn)) - clean) ** 2).sum(-1).mean((0, 2, 3)))
    e0, e1 = rms(qn, pn), rms(out.q.cpu().numpy(), out.pos.cpu().numpy())
    print(f"[smooth] seeded noisy dance, per dancer: jitter {before.round(0).tolist()} -> {after.round(0).tolist()} m/s^3 (ratio "
          f"{(after / before).round(3).tolist()}, bound 0.35), rms joint error {e0.round(4).tolist()} -> {e1.round(4).tolist()} m")
    assert (after <= 0.35 * before).all() and (e1 < e0).all()
    assert bool((out.after["accel_mean"] < out.before["accel_mean"]).all()) and not out.copied.any()
    assert 0.0 < float(out.max_rot_change.max()) < 0.2 and 0.0 < float(out.max_pos_change.max()) < 0.03


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def _normalizer(scale, min_):
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_, n.scaler.min_ = scale.float(), min_.float()
    return n


DN = 2
NORM = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
NAMES = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]


@pytest.fixture(scope="module")
def diffusion():
    """the small model tests/test_footlock_gpu.py builds, built again here"""
    from oracle import tcdiff_oracle as O
    from tcdiff_amd import DanceDecoder, GaussianDiffusion
    seq = 60
    sd = O.synth_state_dict(dn=DN, seq_len=seq)
    model = DanceDecoder(nfeats=151, seq_len=seq, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=TF.gelu, required_dancer_num=DN)
    model.load_state_dict(sd)
    return GaussianDiffusion(model, seq, 151, None, schedule="cosine", n_timestep=100, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=seq).to(DEV).eval()


def _files(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


def _pickles(folder):
    out = []
    for name in E.fk_out_names("normal", 7, NAMES):
        with open(os.path.join(folder, name), "rb") as f:
            out.append(pickle.load(f))
    return out


def test_render_sample_hands_the_filtered_poses_to_the_correctors_and_every_writer(diffusion, tmp_path):
    x = torch.rand(2, 12 * DN, 151, generator=torch.Generator().manual_seed(5)) * 2 - 1
    x[:, ::3, :4] = 1.0                                                    # some rows declare every foot planted
    kw = dict(name=NAMES, required_dancer_num=DN)
    cls = type(diffusion)
    assert diffusion.smooth is False and cls.smooth is False

    def absent(self):
        raise AttributeError("smooth")
    Without = type("Without", (cls,), {"smooth": property(absent)})       # the class as it was before the attribute existed
    try:
        diffusion.__class__ = Without
        assert not hasattr(diffusion, "smooth")
        diffusion.render_sample(x, None, NORM, 7, None, fk_out=str(tmp_path / "fk_absent"), glb_out=str(tmp_path / "glb_absent"), **kw)
    finally:
        diffusion.__class__ = cls
    diffusion.render_sample(x, None, NORM, 7, None, fk_out=str(tmp_path / "fk0"), glb_out=str(tmp_path / "glb0"), **kw)
    assert _files(tmp_path / "fk0") == _files(tmp_path / "fk_absent") and _files(tmp_path / "glb0") == _files(tmp_path / "glb_absent")
    parents, offsets = diffusion._skeleton(torch.device(DEV))
    q, pos, poses, contacts = E.export_poses(x.to(DEV), NORM, "normal", DN, parents=parents, offsets=offsets)
    assert _files(tmp_path / "fk0") == _files(os.path.dirname(E.write_fk_out(str(tmp_path / "fkw"), "normal", 7, NAMES, q, pos, poses)[0]))
    for setting, skw in ((True, {}), (5, dict(window=5))):
        want = S.smooth(q, pos, dn=DN, parents=parents, offsets=offsets, **skw)
        assert not torch.equal(want.q, q) and not torch.equal(want.pos, pos)
        try:
            diffusion.smooth = setting
            diffusion.render_sample(x, None, NORM, 7, None, fk_out=str(tmp_path / f"fk_{setting}"), glb_out=str(tmp_path / f"glb_{setting}"), **kw)
        finally:
            del diffusion.smooth                                           # back to the class attribute
        for c, d in enumerate(_pickles(tmp_path / f"fk_{setting}")):
            assert np.array_equal(d["smpl_poses"], want.q[c].cpu().numpy().reshape(-1, 72)) and np.array_equal(d["smpl_trans"], want.pos[c].cpu().numpy())
            assert np.array_equal(d["full_pose"], want.joints[c].cpu().numpy())
        from tcdiff_amd.gltf import write_glb_out
        glb = write_glb_out(str(tmp_path / f"glbw_{setting}"), "normal", 7, NAMES, want.q, want.pos, DN, parents=parents, offsets=offsets)
        assert _files(tmp_path / f"glb_{setting}") == _files(os.path.dirname(glb[0])) != _files(tmp_path / "glb0")
    # with the foot lock as well: the lock acts on the filtered poses
    smoothed = S.smooth(q, pos, dn=DN, parents=parents, offsets=offsets, measure=False)
    locked = F.foot_lock(smoothed.q, smoothed.pos, contacts, dn=DN, parents=parents, offsets=offsets)
    assert int(locked.planted.sum()) > 0 and not torch.equal(locked.q, smoothed.q)
    try:
        diffusion.smooth = diffusion.foot_lock = True
        diffusion.render_sample(x, None, NORM, 7, None, fk_out=str(tmp_path / "fk_both"), **kw)
    finally:
        del diffusion.smooth, diffusion.foot_lock
    for c, d in enumerate(_pickles(tmp_path / "fk_both")):
        assert np.array_equal(d["smpl_poses"], locked.q[c].cpu().numpy().reshape(-1, 72)) and np.array_equal(d["smpl_trans"], smoothed.pos[c].cpu().numpy())
        assert np.array_equal(d["full_pose"], locked.joints[c].cpu().numpy())
    assert diffusion.smooth is False and diffusion.foot_lock is False
    diffusion.render_sample(x, None, NORM, 7, None, fk_out=str(tmp_path / "fk2"), **kw)
    assert _files(tmp_path / "fk2") == _files(tmp_path / "fk0")


def test_refusals_on_the_device():
    _, _, q, pos = R.noisy_case(b=1, dn=2, T=9, seed=11)
    with pytest.raises(L.TcdiffError, match="one device"):
        S.smooth(dev(q), dev(pos).cpu(), dn=2)
    with pytest.raises(L.TcdiffError, match="needs T >= 11, got T = 9"):
        S.smooth(dev(q), dev(pos), dn=2, window=11)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        S.smoothness(torch.zeros(1, 1, 6, 24, 3))
