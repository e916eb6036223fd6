"""The foot lock on the GPU (tcdiff_amd/footlock.py, csrc/footlock.hip) against the float64 restatement tests/footlock_ref.py of
include/tcdiff_footlock.h, and against what it is for: a forward kinematics written separately here (rotation matrices, float64) is
run on the float32 poses the launch returns, and the pinned joints must stand still.  Seeded synthetic motion, dn = 2: random poses
of sigma 0.3 rad and a root that drifts, so that planted feet slide by at least 5 mm a frame."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import footlock_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import footlock as F
from tcdiff_amd import kernels as K
from tcdiff_amd import io as tio
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS, SMPLSkeleton
from tcdiff_amd.metrics import motion_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
DN = R.DN
ROT_BOUND, PIN_BOUND = R.ROT_BOUND, R.PIN_BOUND          # with their reasons in tests/footlock_ref.py: tests/test_post_chain_gpu.py holds the chain to the same two
LEG_JOINTS = [1, 4, 7, 2, 5, 8]
OTHERS = [j for j in range(24) if j not in LEG_JOINTS]


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


def frames_of(a, dn=DN):
    """(b, T dn, ...) rows -> (b, dn, T, ...)"""
    a = np.asarray(a)
    return np.moveaxis(a.reshape((a.shape[0], a.shape[1] // dn, dn) + a.shape[2:]), 2, 1)


def rotation_error(got, ref64):
    """the largest relative rotation angle between the float32 output and the restatement's unrounded rotation vectors"""
    a, b = np.asarray(got, np.float64)[:, :, LEG_JOINTS].reshape(-1, 3), ref64[:, :, LEG_JOINTS].reshape(-1, 3)
    return max(R.angle_between(x, y) for x, y in zip(a, b))


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared cases are read-only


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a: F.FootLock, b: F.FootLock):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check_against(out: F.FootLock, ref, what):
    err = rotation_error(out.q.cpu().numpy(), ref["q64"])
    print(f"[footlock] {what}: largest rotation error against the restatement {err:.3e} rad (bound {ROT_BOUND:g})")
    assert err <= ROT_BOUND
    assert np.array_equal(out.planted.cpu().numpy(), ref["planted"]) and np.array_equal(out.clamped.cpu().numpy(), ref["clamped"])
    assert out.planted.dtype == out.clamped.dtype == torch.int32 and out.max_shift.dtype == torch.float64
    assert np.allclose(out.max_shift.cpu().numpy(), ref["max_shift"], rtol=1e-12, atol=0)
    return err


def check_purpose(out: F.FootLock, q, pos, ref, blend):
    """the pinned joints stand still, and nothing else moves"""
    got = out.q.cpu().numpy()
    P0, P1 = fk64(frames_of(q), frames_of(pos)), fk64(frames_of(got), frames_of(pos))
    joints = out.joints.cpu().numpy()
    assert joints.shape == P1.shape and np.abs(joints - P1).max() <= 1e-5 and np.isfinite(got).all()      # the float32 FK of the new poses
    T = P0.shape[2]
    worst = 0.0
    for leg, (h, k, a, e) in enumerate(R.LEGS):
        g, st = ref["g"][0, :, leg], ref["status"][0, :, leg]
        for d in range(DN):
            t = 0
            while t < T:
                if g[d, t] == 0:
                    t += 1
                    continue
                end = t
                while end + 1 < T and g[d, end + 1] == g[d, t]:
                    end += 1
                j = a if g[d, t] == 1 else e
                anchor = P0[0, d, t:end + 1, j].mean(0)                                 # the run's anchor, from the raw poses
                free = st[d, t:end + 1] != 2
                if free.any():
                    worst = max(worst, np.linalg.norm(P1[0, d, t:end + 1, j] - anchor, axis=-1)[free].max())
                step = np.linalg.norm(np.diff(joints[0, d, t:end + 1, j].astype(np.float64), axis=0), axis=-1)
                both = free[1:] & free[:-1]
                assert not both.any() or step[both].max() <= 1e-5
                if end > t:
                    assert np.linalg.norm(np.diff(P0[0, d, t:end + 1, j], axis=0), axis=-1).min() >= 5e-3      # the input slid
                t = end + 1
    assert worst <= PIN_BOUND, worst
    assert np.array_equal(got[:, :, OTHERS].view(np.int32), np.asarray(q)[:, :, OTHERS].view(np.int32))
    for leg, legj in enumerate(R.LEGS):
        for d in range(DN):
            planted = ref["g"][0, d, leg] != 0
            far = np.array([not planted[max(0, t - blend):t + blend + 1].any() for t in range(T)])
            a, b = frames_of(got)[0, d][far][:, list(legj[:3])], frames_of(q)[0, d][far][:, list(legj[:3])]
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    return worst


@pytest.fixture(scope="module")
def raw_joints():
    """the joints of the unlocked poses: foot_lock with every contact off copies the poses through"""
    def of(q, pos):
        T = q.shape[1] // DN
        out = F.foot_lock(dev(q), dev(pos), torch.zeros(1, DN, T, 4, device=DEV), dn=DN)
        assert torch.equal(bits(out.q), bits(dev(q)))
        return out.joints
    return of


# ---- against the restatement, at the shapes at which the scan can go wrong -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_foot_lock_against_the_restatement_and_its_purpose(name, raw_joints):
    q, pos, contacts, blend, ref = R.case(name)
    T = q.shape[1] // DN
    tq, tpos, tc = dev(q), dev(pos), dev(contacts)
    before = tpos.clone()
    out = F.foot_lock(tq, tpos, tc, dn=DN, blend=blend)
    assert isinstance(out, F.FootLock) and tuple(out.q.shape) == tuple(tq.shape) and tuple(out.joints.shape) == (1, DN, T, 24, 3)
    assert tuple(out.planted.shape) == tuple(out.clamped.shape) == tuple(out.max_shift.shape) == (1, DN, 2)
    assert torch.equal(bits(tpos), bits(before)) and out.q.data_ptr() != tq.data_ptr()
    check_against(out, ref, name)
    worst = check_purpose(out, q, pos, ref, blend)
    print(f"[footlock] {name}: pinned joints within {worst:.3e} m of their anchors (bound {PIN_BOUND:g})")
    raw = raw_joints(q, pos)
    assert torch.equal(bits(out.joints[:, :, :, [0, 1, 2, 3]]), bits(raw[:, :, :, [0, 1, 2, 3]]))          # pelvis, hips and spine: the same float32
    ours = SMPLSkeleton(device=DEV).forward(tq, tpos)                                      # the library's other FK launch agrees on the raw joints
    assert np.abs(frames_of(ours.cpu().numpy()) - raw.cpu().numpy()).max() <= 1e-5
    if name == "off":
        assert torch.equal(bits(out.q), bits(tq)) and not out.planted.any() and not out.clamped.any() and not out.max_shift.any()
    if name not in ("T1", "T2", "off"):
        locked, slid = (motion_metrics(j, tc)["contact_slide"] for j in (out.joints, raw))
        print(f"[footlock] {name}: contact_slide {locked.flatten().tolist()} against {slid.flatten().tolist()} raw")
        assert bool((locked < slid).all())
    assert same_bits(out, F.foot_lock(tq, tpos, tc, dn=DN, blend=blend))                  # two runs, equal bits
    nojoints = F.foot_lock(tq, tpos, tc, dn=DN, blend=blend, return_joints=False)
    assert nojoints.joints is None and torch.equal(bits(nojoints.q), bits(out.q))


def test_labels_from_the_motion_when_there_are_no_contacts():
    q, pos, ref = R.motion_case()
    assert ref["min_margin"] > 1e-6                                        # no displacement within 1e-6 m of `still`: a label cannot tie
    out = F.foot_lock(dev(q), dev(pos), None, dn=DN)
    check_against(out, ref, "motion labels")
    got = out.q.cpu().numpy()
    assert np.array_equal(got[:, :, OTHERS].view(np.int32), q[:, :, OTHERS].view(np.int32))
    P1 = fk64(frames_of(got), frames_of(pos))
    for leg, (h, k, a, e) in enumerate(R.LEGS):                            # every planted, unclamped frame stands on the restatement's anchor
        g, st = ref["g"][:, :, leg], ref["status"][:, :, leg]
        pin = np.where((g == 2)[..., None], P1[..., e, :], P1[..., a, :])
        free = (g != 0) & (st != 2)
        assert free.any() and np.linalg.norm(pin - ref["anchor"][:, :, leg], axis=-1)[free].max() <= PIN_BOUND


def test_a_target_beyond_reach():
    q, pos, contacts, ref = R.reach_case()
    out = F.foot_lock(dev(q), dev(pos), dev(contacts), dn=DN)
    check_against(out, ref, "beyond reach")
    got = out.q.cpu().numpy()
    assert np.isfinite(got).all() and bool(torch.isfinite(out.joints).all()) and bool(torch.isfinite(out.max_shift).all())
    assert int(out.clamped[0, 0, 0]) > 0 and int(out.clamped[0, 1, 1]) > 0 and float(out.max_shift.max()) > 0.4
    P0, P1 = fk64(frames_of(q), frames_of(pos)), fk64(frames_of(got), frames_of(pos))
    seen = 0
    for (c, d, leg, t), inf in ref["info"].items():
        if ref["status"][c, d, leg, t] != 2:
            continue
        seen += 1
        h, k, a, e = R.LEGS[leg]
        ch = R.chain(q[c, t * DN + d], pos[c, t * DN + d], leg)
        rmax = (ch["l1"] + ch["l2"]) * (1 - 1e-3)
        reach = P1[c, d, t, a] - P1[c, d, t, h]
        wanted = P0[c, d, t, a] + ref["d"][c, d, leg, t] - P1[c, d, t, h]                # towards where the anchor puts the ankle
        assert abs(np.linalg.norm(reach) - max(rmax, inf["rp"])) <= PIN_BOUND and inf["rp"] >= rmax - 1e-15
        assert np.linalg.norm(np.cross(reach, wanted / np.linalg.norm(wanted))) <= PIN_BOUND and reach @ wanted > 0
    assert seen == int(out.clamped.sum())


# ---- strides and bounds ------------------------------------------------------------------------------------------------------------------------
def test_contacts_are_read_through_their_strides():
    q, pos, contacts, blend, ref = R.case("T130-edges")
    T = q.shape[1] // DN
    frame_major = dev(np.ascontiguousarray(np.moveaxis(contacts, 1, 2)))               # (b, T, dn, 4), as the export's launch writes it
    view = frame_major.permute(0, 2, 1, 3)
    assert not view.is_contiguous() and tuple(view.shape) == (1, DN, T, 4)
    a = F.foot_lock(dev(q), dev(pos), view, dn=DN)
    b = F.foot_lock(dev(q), dev(pos), view.contiguous(), dn=DN)
    padded = torch.full((1, DN, T, 7), 9.0, device=DEV)                               # a wider buffer: channel stride 1, frame stride 7
    padded[..., :4] = dev(contacts)
    c = F.foot_lock(dev(q), dev(pos), padded[..., :4], dn=DN)
    assert same_bits(a, b) and same_bits(a, c)
    check_against(a, ref, "strided contacts")


def test_nothing_is_written_outside_the_outputs_and_the_workspace():
    q, pos, contacts, blend, ref = R.case("T65")
    T, N = 65, DN * 65
    nbytes = K.foot_lock_workspace(1, DN, T)
    assert nbytes == L.FOOTLOCK.constants["TC_FOOTLOCK_WS_PER_FRAME"] * N
    pad = 256

    def guarded(count, dtype, fill):
        whole = torch.full((count + 2 * pad,), fill, dtype=dtype, device=DEV)
        return whole, whole[pad:pad + count]
    ws_all, ws = guarded(nbytes, torch.uint8, 0xA5)
    q_all, q_out = guarded(N * 72, torch.float32, 7.5)
    j_all, joints = guarded(N * 72, torch.float32, 7.5)
    p_all, planted = guarded(DN * 2, torch.int32, -77)
    c_all, clamped = guarded(DN * 2, torch.int32, -77)
    m_all, shift = guarded(DN * 2, torch.float64, 7.5)
    K.foot_lock(dev(q), dev(pos), dev(contacts), 1, DN, T, 0.95, 0.01, blend, 1e-3, SMPL_PARENTS, SMPL_OFFSETS, ws, q_out.view(1, N, 24, 3),
                joints.view(1, DN, T, 24, 3), planted.view(1, DN, 2), clamped.view(1, DN, 2), shift.view(1, DN, 2))
    torch.cuda.synchronize()
    for whole, count, fill in ((ws_all, nbytes, 0xA5), (q_all, N * 72, 7.5), (j_all, N * 72, 7.5), (p_all, DN * 2, -77), (c_all, DN * 2, -77),
                               (m_all, DN * 2, 7.5)):
        assert bool((whole[:pad] == fill).all()) and bool((whole[pad + count:] == fill).all())
    want = F.foot_lock(dev(q), dev(pos), dev(contacts), dn=DN, blend=blend)
    got = F.FootLock(q_out.view(1, N, 24, 3), joints.view(1, DN, T, 24, 3), planted.view(1, DN, 2), clamped.view(1, DN, 2), shift.view(1, DN, 2))
    assert same_bits(got, want) and not bool((q_out == 7.5).any()) and not bool((joints == 7.5).any())


def test_clips_are_independent():
    """three clips in one call give each clip's own bits"""
    names = ["gaps", "ends", "blend0"]                                     # all T = 40; blend differs, so run them at blend 3
    cases = [R.case(n) for n in names]
    q, pos, contacts = (np.concatenate([c[i] for c in cases]) for i in range(3))
    out = F.foot_lock(dev(q), dev(pos), dev(contacts), dn=DN, blend=3)
    for i, c in enumerate(cases):
        one = F.foot_lock(dev(c[0]), dev(c[1]), dev(c[2]), dn=DN, blend=3)
        assert same_bits(F.FootLock(*(t[i:i + 1] for t in out)), one)
    check_against(F.FootLock(*(t[:1] for t in out)), cases[0][4], "three clips, the first")


def test_refusals_on_the_device():
    q, pos, contacts, blend, ref = R.case("T2")
    with pytest.raises(L.TcdiffError, match="one device"):
        F.foot_lock(dev(q), dev(pos).cpu(), dev(contacts), dn=DN)
    with pytest.raises(L.TcdiffError, match="one device"):
        F.foot_lock(dev(q), dev(pos), dev(contacts).cpu(), dn=DN)
    wrong = list(SMPL_PARENTS)
    wrong[8] = 2
    with pytest.raises(L.TcdiffError, match="unsupported"):
        F.foot_lock(dev(q), dev(pos), dev(contacts), dn=DN, parents=wrong)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def _normalizer(scale, min_):
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_, n.scaler.min_ = scale.float(), min_.float()
    return n


NORM = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
NAMES = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]


@pytest.fixture(scope="module")
def diffusion():
    """the small model tests/test_render_export_gpu.py builds, built again here"""
    from oracle import tcdiff_oracle as O
    from tcdiff_amd import DanceDecoder, GaussianDiffusion
    S = 60
    sd = O.synth_state_dict(dn=DN, seq_len=S)
    model = DanceDecoder(nfeats=151, seq_len=S, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=TF.gelu, required_dancer_num=DN)
    model.load_state_dict(sd)
    return GaussianDiffusion(model, S, 151, None, schedule="cosine", n_timestep=100, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=S).to(DEV).eval()


def _files(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


def test_render_sample_hands_the_locked_poses_to_every_writer(diffusion, tmp_path):
    x = torch.rand(2, 8 * DN, 151, generator=torch.Generator().manual_seed(5)) * 2 - 1
    x[:, ::3, :4] = 1.0                                                    # some rows declare every foot planted
    assert diffusion.foot_lock is False
    kw = dict(name=NAMES, required_dancer_num=DN)
    diffusion.render_sample(x, None, NORM, 7, None, fk_out=str(tmp_path / "fk0"), glb_out=str(tmp_path / "glb0"), **kw)
    parents, offsets = diffusion._skeleton(torch.device(DEV))
    q, pos, poses, contacts = E.export_poses(x.to(DEV), NORM, "normal", DN, parents=parents, offsets=offsets)
    assert _files(tmp_path / "fk0") == _files(os.path.dirname(E.write_fk_out(str(tmp_path / "fkw"), "normal", 7, NAMES, q, pos, poses)[0]))
    locked = F.foot_lock(q, pos, contacts, dn=DN, parents=parents, offsets=offsets)
    assert int(locked.planted.sum()) > 0 and not torch.equal(locked.q, q)
    assert torch.equal(bits(locked.joints[:, :, :, :4]), bits(poses[:, :, :, :4]))      # pelvis, hips, spine: the export's own float32
    try:
        diffusion.foot_lock = True
        diffusion.render_sample(x, None, NORM, 7, None, fk_out=str(tmp_path / "fk1"), glb_out=str(tmp_path / "glb1"), **kw)
    finally:
        del diffusion.foot_lock                                            # back to the class attribute
    assert diffusion.foot_lock is False
    names = sorted(os.listdir(tmp_path / "fk1"))
    assert names == sorted(os.listdir(tmp_path / "fk0")) and len(names) == 2
    for c, name in enumerate(E.fk_out_names("normal", 7, NAMES)):
        with open(tmp_path / "fk1" / name, "rb") as f:
            d = pickle.load(f)
        assert np.array_equal(d["smpl_poses"], locked.q[c].cpu().numpy().reshape(-1, 72)) and np.array_equal(d["smpl_trans"], pos[c].cpu().numpy())
        assert np.array_equal(d["full_pose"], locked.joints[c].cpu().numpy())
    from tcdiff_amd.gltf import write_glb_out
    want = write_glb_out(str(tmp_path / "glbw"), "normal", 7, NAMES, locked.q, pos, DN, parents=parents, offsets=offsets)
    assert _files(tmp_path / "glb1") == _files(os.path.dirname(want[0])) and _files(tmp_path / "glb1") != _files(tmp_path / "glb0")
    diffusion.render_sample(x, None, NORM, 7, None, fk_out=str(tmp_path / "fk2"), glb_out=str(tmp_path / "glb2"), **kw)
    assert _files(tmp_path / "fk2") == _files(tmp_path / "fk0") and _files(tmp_path / "glb2") == _files(tmp_path / "glb0")
