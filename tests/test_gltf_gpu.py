"""csrc/gltf.hip and tcdiff_amd/gltf.py on an MI355X against the numpy float64 restatement tests/gltf_ref.py.

times and trans bit for bit; quaternion components within 2^-23, one float32 ulp at 1: the most a last-bit difference of two
float64 sin / cos can move a value rounded once to float32.  A missed or extra sign flip is an error of up to 2, so the same bound
pins every sign; the restatement shows on its own inputs that no sign decision is a near-tie before anything is compared."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gltf_ref as G
from tcdiff_amd import _lib as L
from tcdiff_amd import export as E
from tcdiff_amd import gltf as X
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DN = 2


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a writable copy: the shared inputs are read-only)


def _rows(poses, trans):
    """(clips, T, dn, ...) numpy -> the (clips, T dn, 24, 3) / (clips, T dn, 3) device tensors export_poses returns"""
    clips, T, dn = poses.shape[:3]
    return _dev(poses).reshape(clips, T * dn, 24, 3), _dev(trans).reshape(clips, T * dn, 3)


@pytest.mark.parametrize("shape", G.GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_launch_against_the_restatement(shape):
    """T = 1, 2: a pass of one or two lanes; 63, 64, 65: one pass less a frame, exactly one, one and a frame; 150: three passes,
    three clips; 1125: eighteen passes"""
    clips, T, dn = shape
    poses, trans, want, info = G.seeded(*shape)
    got = X.animation_block(*_rows(poses, trans), dn)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (clips, G.floats(T, dn)) and got.is_contiguous()
    print(f"{shape}: {info['flips']} flips, nearest decision {info['margin']:.3e}")
    G.compare(got.cpu().numpy(), want, T, dn, str(shape))


def test_flips_at_the_pass_boundaries_and_the_special_cases():
    """flips at t = 63, 64, 65, 127 and 128 only, so the carry between passes decides alone; the zero vector at the root and
    elsewhere, theta = 1e-4, theta around 1e-3, theta = pi, an unwrapped theta = 4 at frame 0, a NaN in the middle of a channel.
    (A dot product of exactly 0 cannot be reached through rotation vectors: csrc/gltf_math.h's test takes it on the host,
    tests/test_gltf_cpu.py.)"""
    poses, trans, want, _ = G.crafted()
    got = X.animation_block(*_rows(poses, trans), 1).cpu().numpy()
    G.compare(got, want, 130, 1, "crafted")
    G.check_crafted(got)
    other, _ = G.block(poses, trans, 29.97)                               # another frame rate moves the times and nothing else
    got = X.animation_block(*_rows(poses, trans), 1, fps=29.97).cpu().numpy()
    G.compare(got, other, 130, 1, "crafted, 29.97 fps")
    assert not np.array_equal(other[:, :130], want[:, :130]) and np.array_equal(other[:, 130:], want[:, 130:], equal_nan=True)


@pytest.mark.parametrize("lead", [1, 3, 4])
def test_nothing_is_written_outside_the_block(lead):
    """the output between guard floats, at three alignments of its first byte (4, 12 and 16 bytes past an allocation)"""
    clips, T, dn = 2, 65, 2
    poses, trans, want, _ = G.seeded(clips, T, dn)
    q, p = _rows(poses, trans)
    n = clips * G.floats(T, dn)
    guard = np.float32(-1234.5)
    buf = torch.full((lead + n + 7,), float(guard), device=DEV)
    K.gltf_animation(q, p, clips, T, dn, 30.0, buf[lead:lead + n])
    host = buf.cpu().numpy()
    assert (host[:lead] == guard).all() and (host[lead + n:] == guard).all()
    G.compare(host[lead:lead + n].reshape(clips, -1), want, T, dn, f"guarded, {4 * lead} bytes in")
    assert not (host[lead:lead + n] == guard).any()                       # and every float of the block is written


def test_runs_repeat_on_any_stream_and_both_layouts_give_the_same_block():
    clips, T, dn = 1, 150, 3
    poses, trans, want, _ = G.seeded(3, T, dn)
    q, p = _rows(poses, trans)
    first = X.animation_block(q, p, dn)
    assert torch.equal(first.view(torch.int32), X.animation_block(q, p, dn).view(torch.int32))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = X.animation_block(q, p, dn)
    side.synchronize()
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    for c in range(3):                                                     # the pickles' 2-D layout, clip by clip
        flat = X.animation_block(q[c].reshape(T * dn, 72), p[c], dn)
        assert tuple(flat.shape) == (clips, G.floats(T, dn)) and torch.equal(flat[0].view(torch.int32), first[c].view(torch.int32))
    strided = torch.zeros(3, T * dn, 25, 3, device=DEV)                   # a view that is not contiguous is copied, not misread
    strided[:, :, :24] = q
    assert torch.equal(X.animation_block(strided[:, :, :24], p, dn).view(torch.int32), first.view(torch.int32))
    with pytest.raises(L.TcdiffError, match="MI355X"):
        X.animation_block(q, p.cpu(), dn)


# ---- through the pose export to files and back -----------------------------------------------------------------------------------
def _normalizer(scale, min_):
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_, n.scaler.min_ = scale.float(), min_.float()
    return n


NORM = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
NAMES = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]
LONG_NAME = ["data/test/features/gLH_sBM_c01_d16_mLH2_ch04_slice0.npy"]


def _samples(b, S=8, seed=5):
    return torch.rand(b, S * DN, 151, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _joints_of_file(path, dn):
    with open(path, "rb") as f:
        gltf, binary = G.read_glb(f.read())
    world, times = G.evaluate(gltf, binary)
    return G.joints_of(gltf, world, dn, X.JOINT_NAMES), times, gltf


def test_end_to_end_the_files_joints_are_the_exports(tmp_path):
    """samples -> export_poses -> write_glb -> the reader and evaluator of tests/gltf_ref.py: the file's joints are full_pose
    turned to Y-up within 2e-5 m, the export's own bound on its joints (tests/export_ref.py BOUNDS["joints"] = 1e-5) plus the
    1e-5 the quaternions' rounding can move a hand (tests/test_gltf_cpu.py)"""
    S = 8
    q, pos, poses, _ = E.export_poses(_samples(2).to(DEV), NORM, "normal", DN)
    paths = [str(tmp_path / "a.glb"), str(tmp_path / "b.glb")]
    assert X.write_glb(paths, q, pos, DN) == paths
    for c, path in enumerate(paths):
        got, times, gltf = _joints_of_file(path, DN)
        want = G.to_y_up(poses[c].cpu().numpy().astype(np.float64))
        err = float(np.abs(got - want).max())
        print(f"clip {c}: the file's joints against full_pose, largest difference {err:.3e} m (bound 2e-5)")
        assert got.shape == (DN, S, 24, 3) and err <= 2e-5
        assert np.array_equal(times, (np.arange(S) / 30.0).astype(np.float32)) and len(gltf["skins"]) == DN
    one = X.write_glb(str(tmp_path / "one.glb"), q[1:], pos[1:], DN)
    assert one == [str(tmp_path / "one.glb")] and open(one[0], "rb").read() == open(paths[1], "rb").read()
    assert X.write_glb(paths[:1], q, pos, DN, body=False) == paths[:1] and "meshes" not in _joints_of_file(paths[0], DN)[2]
    with pytest.raises(L.TcdiffError, match="single path"):
        X.write_glb(str(tmp_path / "two.glb"), q, pos, DN)
    with pytest.raises(L.TcdiffError, match="3 paths"):
        X.write_glb(paths + [str(tmp_path / "c.glb")], q, pos, DN)
    assert not (tmp_path / "two.glb").exists() and not (tmp_path / "c.glb").exists()


def test_long_mode_is_one_file_of_the_whole_song_and_convert_fk_out_rewrites_it(tmp_path):
    x3 = _samples(3, seed=6).to(DEV)
    q, pos, full, none = E.export_poses(x3, NORM, "long", DN)
    assert none is None and tuple(q.shape) == (1, 16 * DN, 24, 3)
    written = X.write_glb_out(str(tmp_path / "glb"), "long", 3, LONG_NAME, q, pos, DN)
    assert written == [str(tmp_path / "glb" / "3_gLH_sBM_c01_d16_mLH2_ch04.glb")] and os.listdir(tmp_path / "glb") == [os.path.basename(written[0])]
    got, times, _ = _joints_of_file(written[0], DN)
    assert got.shape == (DN, 16, 24, 3) and len(times) == 16
    assert float(np.abs(got - G.to_y_up(full[0].cpu().numpy().astype(np.float64))).max()) <= 2e-5
    # a pickle written earlier, converted later: the same bytes
    pkl, = E.write_fk_out(str(tmp_path / "fk"), "long", 3, LONG_NAME, q, pos, full)
    out = X.convert_fk_out(pkl)
    assert out == pkl[:-4] + ".glb" and open(out, "rb").read() == open(written[0], "rb").read()
    assert X.convert_fk_out(pkl, str(tmp_path / "elsewhere.glb"), body=False) == str(tmp_path / "elsewhere.glb")
    qn, posn, posesn, _ = E.export_poses(_samples(2).to(DEV), NORM, "normal", DN)
    pkls = E.write_fk_out(str(tmp_path / "fk"), "normal", 7, NAMES, qn, posn, posesn)
    glbs = X.write_glb_out(str(tmp_path / "glb7"), "normal", 7, NAMES, qn, posn, DN)
    assert [os.path.basename(g) for g in glbs] == ["7_0_gBR_sBM_c01_d04_mBR0_ch01_slice3.glb", "7_1_wav_gLO_slice12.glb"]
    for pk, gl in zip(pkls, glbs):
        assert open(X.convert_fk_out(pk), "rb").read() == open(gl, "rb").read()
    assert X.write_glb_out(str(tmp_path / "glb1"), "normal", 7, NAMES[:1], qn, posn, DN) == [str(tmp_path / "glb1" / os.path.basename(glbs[0]))]


@pytest.fixture(scope="module")
def diffusion():
    """the small model tests/test_render_export_gpu.py builds, built again here"""
    from oracle import tcdiff_oracle as O
    from tcdiff_amd import DanceDecoder, GaussianDiffusion
    S = 60
    sd = O.synth_state_dict(dn=DN, seq_len=S)
    model = DanceDecoder(nfeats=151, seq_len=S, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=F.gelu, required_dancer_num=DN)
    model.load_state_dict(sd)
    return GaussianDiffusion(model, S, 151, None, schedule="cosine", n_timestep=100, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=S).to(DEV).eval()


def test_render_sample_writes_glb_out_and_exports_once(diffusion, tmp_path, monkeypatch):
    calls = []
    real = E.export_poses
    monkeypatch.setattr(E, "export_poses", lambda *a, **k: calls.append(1) or real(*a, **k))
    x = _samples(2)
    ret = diffusion.render_sample(x, None, NORM, 7, None, name=NAMES, required_dancer_num=DN, glb_out=str(tmp_path / "glb"))
    assert ret is x and len(calls) == 1
    assert sorted(os.listdir(tmp_path / "glb")) == ["7_0_gBR_sBM_c01_d04_mBR0_ch01_slice3.glb", "7_1_wav_gLO_slice12.glb"]
    q, pos, _, _ = real(x.to(DEV), NORM, "normal", DN)
    parents, offsets = diffusion._skeleton(torch.device(DEV))             # the model's skeleton, as render_sample hands it on
    want = X.write_glb([str(tmp_path / "w0.glb"), str(tmp_path / "w1.glb")], q, pos, DN, parents=parents, offsets=offsets)
    for name, w in zip(X.glb_out_names("normal", 7, NAMES), want):
        assert open(tmp_path / "glb" / name, "rb").read() == open(w, "rb").read()
    del calls[:]                                                           # with fk_out and draw_out too: still one export
    x3 = _samples(3, seed=6)
    ret = diffusion.render_sample(x3, None, NORM, 3, None, fk_out=str(tmp_path / "fk"), mode="long", required_dancer_num=DN,
                                  render_len=4, name=LONG_NAME, glb_out=str(tmp_path / "long"), draw_out=str(tmp_path / "draw"))
    assert ret is x3 and len(calls) == 1
    assert os.listdir(tmp_path / "long") == ["3_gLH_sBM_c01_d16_mLH2_ch04.glb"] and os.listdir(tmp_path / "fk") == ["3_gLH_sBM_c01_d16_mLH2_ch04.pkl"]
    assert os.listdir(tmp_path / "draw") == ["3_gLH_sBM_c01_d16_mLH2_ch04.png"]
    assert _joints_of_file(tmp_path / "long" / "3_gLH_sBM_c01_d16_mLH2_ch04.glb", DN)[0].shape == (DN, 16, 24, 3)
    del calls[:]                                                           # without a normalizer: nothing to export, no directory
    assert diffusion.render_sample(x, None, required_dancer_num=DN, glb_out=str(tmp_path / "none")) is x
    assert not calls and not (tmp_path / "none").exists()
