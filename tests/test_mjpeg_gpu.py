"""GPU checks of the Motion-JPEG path: ``encode_jpeg`` (csrc/mjpeg.hip) against the bytes of the numpy restatement
tests/mjpeg_ref.py of include/tcdiff_mjpeg.h -- the encoder is integer arithmetic, so every comparison is an equality -- on the
shared frames, across the workgroup size, through strides, between sentinels; then the path end to end: ``draw_dance`` ->
``encode_jpeg`` -> ``write_avi`` with sound, ``write_draw_out(format="avi")``, ``render_sample`` with ``draw_format = "avi"``, the
clips' music as ``clip_audio`` finds it, and the default PNG output unchanged."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mjpeg_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import draw as D
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd import video as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DN = 2


def gpu(frames, quality, sub):
    """(bytes, offsets) of encode_jpeg on a numpy array or a tensor"""
    t = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV) if isinstance(frames, np.ndarray) else frames
    j = V.encode_jpeg(t, quality, sub)
    assert j.is_cuda and j.data.dtype == torch.uint8 and j.offsets.dtype == torch.int64 and (j.width, j.height) == tuple(t.shape[-2:-4:-1])
    host = j.cpu()
    assert not host.is_cuda and j.cpu() is host
    return host.data.numpy().tobytes(), host.offsets.numpy()


def assert_decodes_like_pillow_s_own(frame, stream, quality, sub, what):
    ours, theirs = R.psnr_pair(frame, stream, quality, sub)
    assert ours >= theirs - R.PSNR_MARGIN, (what, ours, theirs)


@pytest.mark.parametrize("name", R.CASES)
def test_encode_jpeg_gives_the_restatement_s_bytes(name):
    for quality in R.QUALITIES:
        for sub in R.SUBS:
            want, want_off, _ = R.expected(name, quality, sub)
            got, got_off = gpu(R.case(name), quality, sub)
            assert np.array_equal(got_off, want_off), (name, quality, sub, got_off, want_off)
            assert got == want, (name, quality, sub)


@pytest.mark.parametrize("sub", R.SUBS)
def test_an_interval_wider_than_the_workgroup_and_longer_than_the_window(sub):
    frames = R.wide_frame(V.THREADS)
    assert frames.shape[2] // 8 * 3 > V.THREADS                            # one interval holds more blocks than a workgroup has threads
    want, want_off = R.encode_all(frames, 100, sub)
    assert want_off[1] > 2 * L.MJPEG.constants["TC_MJPEG_WINDOW"]           # and more bytes than two windows
    got, got_off = gpu(frames, 100, sub)
    assert np.array_equal(got_off, want_off) and got == want


def test_views_are_read_in_place_through_their_strides():
    rng = np.random.default_rng(17)
    big = torch.from_numpy(rng.integers(0, 256, (3, 24, 44, 3), dtype=np.uint8)).to(DEV)
    crop = big[:, 3:20, 5:38]
    assert not crop.is_contiguous() and tuple(crop.shape) == (3, 17, 33, 3)
    want = R.encode_all(crop.cpu().numpy(), 90, "420")
    for frames in (crop, crop.contiguous()):
        got = gpu(frames, 90, "420")
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
    base = torch.from_numpy(rng.integers(0, 256, (3, 2, 17, 33, 3), dtype=np.uint8)).to(DEV)
    batch = base.permute(1, 0, 2, 3, 4)                                    # (b, T, ...) = (2, 3, ...) with the leading strides swapped
    assert batch.stride(0) != 3 * batch.stride(1)
    want = R.encode_all(batch.cpu().numpy().reshape(6, 17, 33, 3), 90, "444")
    for frames in (batch, batch.contiguous(), batch.contiguous().reshape(6, 17, 33, 3), batch[:, :1], batch[:1]):
        got = gpu(frames, 90, "444")
        if frames.shape[:2] == (2, 1):
            assert got[0] == b"".join(want[0][want[1][i]:want[1][i + 1]] for i in (0, 3))
        elif frames.shape[0] == 1:
            assert got[0] == want[0][:want[1][3]] and np.array_equal(got[1], want[1][:4])
        else:
            assert got[0] == want[0] and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("ws_at, data_at", [(8, 3), (64, 16)])
def test_nothing_is_written_outside_data_and_workspace(ws_at, data_at):
    name, quality, sub = "33x17", 100, "420"
    frames = torch.from_numpy(R.case(name)).to(DEV)
    N, H, W, _ = frames.shape
    want, want_off, _ = R.expected(name, quality, sub)
    need = K.mjpeg_workspace(N, H, W, V.SUBSAMPLING[sub])
    ws_buf = torch.full((need + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    workspace = ws_buf[ws_at:ws_at + need]
    offsets_buf = torch.full((N + 3,), -7, dtype=torch.int64, device=DEV)
    K.mjpeg_plan(frames, quality, V.SUBSAMPLING[sub], workspace, offsets_buf[1:N + 2])
    assert offsets_buf[0] == -7 and offsets_buf[-1] == -7 and np.array_equal(offsets_buf[1:-1].cpu().numpy(), want_off)
    total = int(want_off[-1])
    data_buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    K.mjpeg_write(N, H, W, quality, V.SUBSAMPLING[sub], workspace, data_buf[data_at:data_at + total])
    torch.cuda.synchronize()
    assert (ws_buf[:ws_at] == 0xA5).all() and (ws_buf[ws_at + need:] == 0xA5).all()
    assert (data_buf[:data_at] == 0xA5).all() and (data_buf[data_at + total:] == 0xA5).all()
    assert data_buf[data_at:data_at + total].cpu().numpy().tobytes() == want
    short = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=DEV)   # too small a buffer: the last interval is not written
    K.mjpeg_write(N, H, W, quality, V.SUBSAMPLING[sub], workspace, short[data_at:data_at + total - 1])
    torch.cuda.synchronize()
    assert (short[:data_at] == 0xA5).all() and (short[data_at + total - 2:] == 0xA5).all()
    with pytest.raises(L.TcdiffError, match="misaligned"):
        K.mjpeg_plan(frames, quality, V.SUBSAMPLING[sub], ws_buf[3:3 + need], offsets_buf[1:N + 2])
    with pytest.raises(L.TcdiffError, match="invalid argument"):
        K.mjpeg_plan(frames, quality, V.SUBSAMPLING[sub], workspace[:need - 1], offsets_buf[1:N + 2])


def test_a_second_run_gives_equal_bytes_and_seven_frames_line_up():
    frames, quality, sub = R.case("seven"), 90, "420"
    first, second = gpu(frames, quality, sub), gpu(frames, quality, sub)
    assert first[0] == second[0] and np.array_equal(first[1], second[1])
    data, off = first
    assert off[0] == 0 and (np.diff(off) > R.HEADER_BYTES).all() and off[-1] == len(data)
    j = V.encode_jpeg(torch.from_numpy(frames).to(DEV), quality, sub)
    assert len(j) == 7 and j.frames() == [data[off[i]:off[i + 1]] for i in range(7)] and j.frame(-1) == j.frame(6)
    with pytest.raises(L.TcdiffError, match="frame"):
        j.frame(7)
    for i, frame in enumerate(frames):
        stream = data[off[i]:off[i + 1]]
        assert stream[:2] == b"\xff\xd8" and stream[-2:] == b"\xff\xd9"
        assert_decodes_like_pillow_s_own(frame, stream, quality, sub, i)
    want, want_off = R.encode_all(frames, quality, sub)
    assert data == want and np.array_equal(off, want_off)


def dance(b=1, dn=2, T=5, seed=11):
    g = torch.Generator().manual_seed(seed)
    joints = torch.randn(b, dn, T, 24, 3, generator=g) * 0.4 + torch.tensor([0.0, 0.0, 1.0])
    return joints.to(DEV)


def test_draw_encode_and_mux_end_to_end(tmp_path):
    joints = dance()
    frames = D.draw_dance(joints, width=48, height=40)
    assert tuple(frames.shape) == (1, 5, 40, 48, 3)
    jpeg = V.encode_jpeg(frames, quality=90)
    sr, sound = 8000, R.tone(1600)                                         # 0.2 s of sound on 5 / 30 s of video
    path = V.write_avi(tmp_path / "clip.avi", jpeg, fps=30, audio=sound, sample_rate=sr)
    pcm = V.pcm16(sound).reshape(-1, 1)
    avi = R.check_avi(path, jpeg.frames(), 48, 40, Fraction(30), pcm, sr)
    video = [c[3] for c in avi["movi"] if c[0] == b"00dc"]
    assert len(video) == 5 and avi["streams"][1][0]["dwLength"] == 5 * sr // 30
    host = frames[0].cpu().numpy()
    for t, stream in enumerate(video):
        assert R.decode(stream).size == (48, 40)
        assert_decodes_like_pillow_s_own(host[t], stream, 90, "420", t)
    written = D.write_draw_out(tmp_path / "out", "normal", 3, ["music/clip.npy"], joints, None, width=48, height=40, format="avi",
                               audio=[(sound, sr)])
    assert written == [str(tmp_path / "out" / "e3_b0_clip.avi")]
    with open(path, "rb") as f, open(written[0], "rb") as g:
        assert f.read() == g.read()
    with pytest.raises(L.TcdiffError, match="audio tracks"):
        D.write_draw_out(tmp_path / "out", "normal", 3, ["music/clip.npy"], joints, None, width=48, height=40, format="avi", audio=[])


def test_clip_audio_is_the_reference_s_stitch(tmp_path):
    """vis.py:299-310 in a few lines of numpy, on three tiny files"""
    sounds = [R.tone(40, seed=k) for k in range(3)]
    names = [str(tmp_path / f"song_slice{k}.npy") for k in range(3)]
    for k, s in enumerate(sounds):
        R.write_wav(tmp_path / f"song_slice{k}.wav", s, sr=8000)
    read = [np.rint(np.clip(s, -1, 1) * 32767).astype(np.int16).astype(np.float32) / 32768 for s in sounds]          # soundfile's int16 -> float32
    normal = V.clip_audio(names, "normal")
    assert len(normal) == 3
    for (got, sr), want in zip(normal, read):
        assert sr == 8000 and got.dtype == np.float32 and np.array_equal(got, want)
    ll, half = 40, 20
    total = np.zeros(ll + half * 2, np.float32)
    total[:ll] = read[0]
    idx = ll
    for a in read[1:]:
        total[idx:idx + half] = a[half:]
        idx += half
    (got, sr), = V.clip_audio(names, "long")
    assert sr == 8000 and np.array_equal(got, total)
    (moved, _), = V.clip_audio(["/nowhere/" + os.path.basename(n) for n in names], "long", folder=tmp_path)
    assert np.array_equal(moved, total)


# ---- render_sample ---------------------------------------------------------------------------------------------------------------------
def _normalizer(scale, min_):
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_, n.scaler.min_ = scale.float(), min_.float()
    return n


@pytest.fixture(scope="module")
def diffusion():
    """the small model tests/test_draw_gpu.py builds, built again here"""
    from oracle import tcdiff_oracle as O
    from tcdiff_amd import DanceDecoder, GaussianDiffusion
    S = 60
    sd = O.synth_state_dict(dn=DN, seq_len=S)
    model = DanceDecoder(nfeats=151, seq_len=S, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=F.gelu, required_dancer_num=DN)
    model.load_state_dict(sd)
    return GaussianDiffusion(model, S, 151, None, schedule="cosine", n_timestep=100, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=S).to(DEV).eval()


def test_render_sample_writes_avi_files_with_the_clips_music(diffusion, tmp_path, monkeypatch):
    diff = diffusion
    assert diff.draw_format == "png"
    g = torch.Generator().manual_seed(5)
    norm = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
    S, sr = 4, 8000
    x = torch.rand(2, S * DN, 151, generator=g) * 2 - 1
    (tmp_path / "music").mkdir()
    names = [str(tmp_path / "music" / "gBR_sBM_c01_d04_mBR0_ch01_slice3.npy"), str(tmp_path / "music" / "npy_gLO_slice12.npy")]
    sounds = [R.tone(2000, seed=k) for k in range(2)]
    R.write_wav(os.path.splitext(names[0])[0] + ".wav", sounds[0], sr)
    monkeypatch.setattr(diff, "draw_format", "avi")
    # a missing .wav raises before any sampling: the sampler is not reached and no directory is made
    called = []
    monkeypatch.setattr(diff, "_render_samples", lambda shape, *a, **k: called.append(shape) or (shape if torch.is_tensor(shape) else x))
    with pytest.raises(L.TcdiffError, match="npy_gLO_slice12.wav does not exist"):
        diff.render_sample((2, S * DN, 151), None, norm, 7, None, name=names, required_dancer_num=DN, draw_out=str(tmp_path / "draw"))
    assert not called and not (tmp_path / "draw").exists()
    R.write_wav(os.path.splitext(names[1])[0] + ".wav", sounds[1], sr)
    ret = diff.render_sample(x, None, norm, 7, None, name=names, required_dancer_num=DN, draw_out=str(tmp_path / "draw"))
    assert ret is x and len(called) == 1                                   # the samples returned are those without draw_out
    assert sorted(os.listdir(tmp_path / "draw")) == ["e7_b0_gBR_sBM_c01_d04_mBR0_ch01_slice3.avi", "e7_b1_npy_gLO_slice12.avi"]
    want = D.draw_samples(x.to(DEV), norm, DN).cpu().numpy()
    for num, f in enumerate(sorted(os.listdir(tmp_path / "draw"))):
        with open(tmp_path / "draw" / f, "rb") as fh:
            avi = R.walk_avi(fh.read())
        video = [c[3] for c in avi["movi"] if c[0] == b"00dc"]
        assert len(video) == S and len(avi["streams"]) == 2 and avi["avih"][8:10] == (480, 480)
        for t in (0, S - 1):
            assert_decodes_like_pillow_s_own(want[num, t], video[t], 90, "420", (f, t))
        sound = np.frombuffer(b"".join(c[3] for c in avi["movi"] if c[0] == b"01wb"), "<i2")
        keep = S * sr // 30
        in_file = np.rint(np.clip(sounds[num], -1, 1) * 32767).astype(np.int16)          # what write_wav stored; it is read back as v / 32768
        assert np.array_equal(sound, V.pcm16(in_file.astype(np.float32) / 32768)[:keep])
        assert np.abs(sound.astype(int) - in_file[:keep]).max() <= 1
    # sound=False: one stream, and no .wav is looked for
    os.remove(os.path.splitext(names[1])[0] + ".wav")
    diff.render_sample(x, None, norm, 8, None, name=names, sound=False, required_dancer_num=DN, draw_out=str(tmp_path / "mute"))
    for f in sorted(os.listdir(tmp_path / "mute")):
        assert f.startswith("e8_b") and f.endswith(".avi")
        with open(tmp_path / "mute" / f, "rb") as fh:
            avi = R.walk_avi(fh.read())
        assert len(avi["streams"]) == 1 and all(c[0] == b"00dc" for c in avi["movi"])
    # the .wav files of another folder, by basename
    monkeypatch.setattr(diff, "draw_audio_folder", str(tmp_path / "elsewhere"))
    (tmp_path / "elsewhere").mkdir()
    for k in range(2):
        R.write_wav(tmp_path / "elsewhere" / (os.path.splitext(os.path.basename(names[k]))[0] + ".wav"), sounds[k], sr)
    diff.render_sample(x[:1], None, norm, 9, None, name=names, required_dancer_num=DN, draw_out=str(tmp_path / "moved"))
    assert os.listdir(tmp_path / "moved") == ["e9_b0_gBR_sBM_c01_d04_mBR0_ch01_slice3.avi"]
    monkeypatch.setattr(diff, "draw_format", "gif")
    with pytest.raises(L.TcdiffError, match="draw_format"):
        diff.render_sample(x, None, norm, 7, None, name=names, required_dancer_num=DN, draw_out=str(tmp_path / "draw"))


def test_the_default_output_is_still_the_same_png(diffusion, tmp_path):
    diff = diffusion
    g = torch.Generator().manual_seed(6)
    norm = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
    x = torch.rand(1, 3 * DN, 151, generator=g) * 2 - 1
    assert diff.draw_format == "png" and type(diff).draw_format == "png"
    diff.render_sample(x, None, norm, 2, None, name=["a/clip.npy"], required_dancer_num=DN, draw_out=str(tmp_path / "draw"))
    assert os.listdir(tmp_path / "draw") == ["e2_b0_clip.png"]
    frames = D.draw_samples(x.to(DEV), norm, DN)
    D.write_apng(tmp_path / "direct.png", frames[0].cpu(), fps=30)
    with open(tmp_path / "draw" / "e2_b0_clip.png", "rb") as f, open(tmp_path / "direct.png", "rb") as h:
        assert f.read() == h.read()
