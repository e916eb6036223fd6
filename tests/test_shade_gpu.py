"""tcr_mesh_vertices / tcr_mesh_raster (csrc/shade.hip) and tcdiff_amd/shade.py on an MI355X against the numpy float64 restatement
tests/shade_ref.py, which is written from the picture's definition in include/tcdiff_shade.h.

Vertices.  `screen` is three float32 fused multiply-adds: within 4 * 2^-24 * sum |terms| of the exact value, the bound draw_ref
derives and shade_ref.project returns per value.  `normals`: kernel and restatement evaluate the same float64 expressions in the
same order, so before the store they differ by float64 rounding only: the sum s of deg <= 8 cross products carries at most
(deg + 3) u64 sum |products|, and on a mesh whose faces around a vertex point the same way sum |products| <= 16 |s|, so a component of
s / len is good to about 200 u64 = 2e-14; the one float32 rounding at the store adds at most half an ulp, 2^-24 |n_c|.  Bound:
2^-24 |n_c| + 2^-40, where 2^-40 = 9e-13 stands for the float64 part with a factor of 40 to spare.

Raster, fed the restatement's own float32 screen and normals: both sides work in float64 (u = 2^-53) on identical inputs, and the
operations are IEEE, so the bytes are expected to be equal; the margins below say where a tie could make them differ.  Screen
coordinates of every triangle that comes near the image are below M = 4096 (asserted).  For a pixel inside a triangle's box grown by
one pixel, with L the box's longer side, |p - vertex| <= L + 1 and |d| = the edge's length:
  delta_edge.  E = dx (py - p.y) - dy (px - p.x): dx, dy and the two differences one rounding each, the products one more (relative
    3 u of at most |d| (L + 1) each), the difference one of at most 2 |d| (L + 1): |error of E| <= 8 u |d| (L + 1), which is
    8 u (L + 1) <= 8 u (2 M + 1) = 7.3e-12 pixels of distance from the edge's line.  Both sides: 1.5e-11; delta_edge = 1e-10.
    A pixel further than that from every edge line near it has the signs of all E_i, and with them coverage and area != 0, decided.
  delta_z.  z = sum w_i z_i, w_i = E_i / area, area = twice the triangle's area = (longest edge) x (smallest altitude h).  Each w_i
    carries (8 u |d| (L + 1) + 3 (the same)) / area <= 32 u (L + 1) / h, the three products, two sums and the division 6 u more:
    |error of z| <= Z (96 (L + 1) / h + 6) u <= 100 u Z r with r = max (L + 1) / h over the triangles that can cover a clear pixel
    (an altitude below delta_edge cannot) and Z = max |z|.  Both sides: delta_z = 200 u Z r, computed per case from its inputs.
  delta_level.  The interpolated normal with weights of sum 1, nhat = sum w_i n_i, carries 3 * 32 u r / 4 + 4 u per component
    <= 24 u r + 4 u; k = ambient + (1 - ambient) |nhat . l| / |nhat| moves by at most twice that over |nhat|, plus 6 u for its own
    operations; a channel is 255 k at most.  Both sides: delta_level = 255 * 2 * (48 u r + 20 u) / |nhat|, per case and pixel.
Asserted: every clear pixel equal; every pixel that is not clear the uncovered value or within one level of one of the
restatement's candidates at that pixel; and, on the restatement alone before the GPU is touched, clear pixels at least 98 % of the
pixels inside any triangle's grown box (tests/test_shade_cpu.py prints the shares: 1.0000 on six cases, 0.9979 on `wild`, whose
zero-area triangle lies on a line through the image, and 0.9956 on `equal-depth`).  In the equal-depth case
the two depths of a pixel are the same operations on the same values, equal bits without any rounding argument: delta_z = 0 there.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import draw_ref
import shade_ref as R
import skin_ref as S
from tcdiff_amd import _lib as L
from tcdiff_amd import body as B
from tcdiff_amd import draw as D
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd import shade as SH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLEAR_SHARE = 0.98
CHUNK = 256                  # the kernel's chunk (TC_SHADE_CHUNK): the crowded tile holds R.CROWD = 640 triangles, more than twice that
SENTINEL = 0xA5


def _t(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype, order="C")).to(DEV)                    # a copy: the cached cases are read-only


# ---- tcr_mesh_vertices ---------------------------------------------------------------------------------------------------------
def _mesh_vertices(verts, faces, view, screen=True, normals=True):
    P, V, _ = verts.shape
    start, listed = R.adjacency(faces, V)
    out = [torch.full((P, V, 3), -1234.5, device=DEV) for _ in range(2)]
    K.mesh_vertices(_t(verts), _t(faces), _t(start), _t(listed), P, V, len(faces), np.asarray(view).reshape(-1).tolist(),
                    out[0] if screen else None, out[1] if normals else None)
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def test_vertices_against_the_float64_restatement():
    verts, faces = R.scene()
    verts = verts.reshape(-1, 70, 3)
    lone = np.concatenate([verts, np.full((len(verts), 1, 3), 0.25, np.float32)], 1)             # vertex 70: no face names it
    view = R.camera(100, 76, 2.5)
    want_s, bound = R.project(lone, view)
    want_n = R.normals(lone, faces, R.adjacency(faces, 71))
    assert L.SHADE.constants["TC_SHADE_CHUNK"] == CHUNK
    got_s, got_n = _mesh_vertices(lone, faces, view)
    ratio = np.abs(got_s.astype(np.float64) - want_s) / bound
    err = np.abs(got_n.astype(np.float64) - want_n) / (2.0 ** -24 * np.abs(want_n) + 2.0 ** -40)
    print(f"[shade] screen: worst error / bound {ratio.max():.3f}; normals: worst error / bound {err.max():.3f}, "
          f"{int((got_n != want_n.astype(np.float32)).sum())} of {got_n.size} differ from the rounded restatement")
    assert (ratio <= 1.0).all() and (err <= 1.0).all()
    assert (got_n[:, 70] == 0).all() and np.abs(np.linalg.norm(got_n[:, :70].astype(np.float64), axis=-1) - 1).max() < 2e-7
    # either output alone: the other buffer keeps its fill, the one written has the same bits
    only_s, kept_n = _mesh_vertices(lone, faces, view, normals=False)
    kept_s, only_n = _mesh_vertices(lone, faces, view, screen=False)
    assert np.array_equal(only_s, got_s) and np.array_equal(only_n, got_n) and (kept_n == -1234.5).all() and (kept_s == -1234.5).all()


# ---- tcr_mesh_raster -----------------------------------------------------------------------------------------------------------
def _style(d):
    st = dict(R.STYLE, **d)
    return SH.make_shade_style(background=st["background"], ambient=st["ambient"], light=st["light"])


def _raster_in_sentinels(c, offset):
    """runs the raster with `frames` placed `offset` bytes into a larger buffer of sentinel bytes; returns the frames (b, T, H, W, 3)
    after checking that no sentinel changed"""
    b, T, dn, W, H = (c[k] for k in ("b", "T", "dn", "W", "H"))
    V, nF = c["screen"].shape[2], len(c["faces"])
    n = b * T * H * W * 3
    buf = torch.full((offset + n + 4096,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    scratch = torch.empty(SH.scratch_bytes(b, T, dn, nF) // 4, dtype=torch.int32, device=DEV)
    K.mesh_raster(_t(c["screen"]), _t(c["normals"]), _t(c["faces"]), b, T, dn, V, nF, W, H, _t(c["colors"], np.uint8), len(c["colors"]),
                  _style(c["style"]), None if c["under"] is None else _t(c["under"]), scratch, buf.data_ptr() + offset)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:offset] == SENTINEL).all() and (host[offset + n:] == SENTINEL).all(), "bytes outside frames were written"
    return host[offset:offset + n].reshape(b, T, H, W, 3)


@pytest.mark.parametrize("name", R.CASES)
def test_raster_on_the_restatement_s_vertices(name):
    """33x17: partial tiles both ways, with `under`; 32x32: exactly one tile, another page, ambient 0; 100x76: 4 x 3 tiles; crowded:
    640 triangles in one tile, more than twice the chunk of 256; wild: a triangle larger than the image, triangles off each of the
    four sides, a zero-area and a repeated-index triangle, a NaN, an infinite and a 1e30 vertex (all draw nothing); one and five
    dancers, the latter with two colours; equal-depth: two dancers on the same triangles, the lower g shows"""
    c = R.case(name)
    ref = R.frames_of(name)
    xy = c["screen"].reshape(-1, 3)[:, :2]
    with np.errstate(invalid="ignore"):
        near = xy[np.isfinite(xy).all(1) & (np.abs(xy).max(1) < 1e29)]    # (the vertex 1e30 away belongs to a triangle off the image)
    assert np.abs(near).max() < R.MAX_COORD
    for clip, t, m, d in ref:                                             # on the restatement alone, before the GPU runs
        assert R.clear_share(m, d) >= CLEAR_SHARE, (name, clip, t)
    got = _raster_in_sentinels(c, 64)
    for clip, t, m, d in ref:
        unclear, differ = R.check(got[clip, t], m, d, (name, clip, t))
        print(f"[shade] {name} clip {clip} frame {t}: {int((m['winner'] >= 0).sum())} covered pixels, {unclear} not clear, {differ} differ")
    if name == "wild":
        shown = {tuple(p) for p in got[0, 0].reshape(-1, 3).tolist()}
        assert len(shown) > 2 and (255, 255, 255) not in shown            # the oversized triangle fills the image, shaded
    if name == "equal-depth":
        m = ref[0][2]
        assert np.array_equal(got[0, 0][m["winner"] >= 0], R.to_bytes(m["values"])[m["winner"] >= 0]) and m["winner"].max() == 1
    assert np.array_equal(got, _raster_in_sentinels(c, 64))               # same input, same bits
    assert np.array_equal(got, _raster_in_sentinels(c, 7))                # byte stores off the 4-byte boundary: the same picture


# ---- tcdiff_amd/shade.py ---------------------------------------------------------------------------------------------------------
DN = 2


def _lattice_body():
    """the synthetic SMPL model of skin_ref on the lattice's 70 vertices and 120 faces"""
    verts, faces = R.lattice(10, 7, seed=3, cz=0.0)
    m = S.make_model(70, 3, seed=6, smpl_tree=True)
    m["v_template"] = verts.astype(np.float64)
    m["f"] = faces.astype(np.uint32)
    return B.load_body_model(m, device=DEV)


def _check_frames(frames, screen, normals, faces, dn, W, H, what, **kw):
    b, T = frames.shape[:2]
    for clip in range(b):
        for t in range(T):
            rows = slice(t * dn, (t + 1) * dn)
            under = kw.get("under")
            m = R.raster(screen[clip, rows], normals[clip, rows], faces, W, H, kw.get("colors", R.PALETTE), kw["style"],
                         None if under is None else under[clip, t])
            z = np.abs(screen[clip, rows, :, 2])
            unclear, differ = R.check(frames[clip, t], m, R.deltas(m, float(z.max())), (what, clip, t))
            print(f"[shade] {what} clip {clip} frame {t}: {int((m['winner'] >= 0).sum())} covered, {unclear} not clear, {differ} differ")
            assert (m["winner"] >= 0).sum() > 50


def test_draw_bodies_on_gpu_skinned_vertices_and_its_keywords():
    body = _lattice_body()
    W, H, T = 64, 48, 2
    poses, trans = S.poses_of(T * DN, seed=2)
    trans = (trans * np.float32([0.4, 0.4, 0.0]) + np.float32([0, 0, 1])).astype(np.float32)
    vertices = B.skin(body, _t(poses)[None], _t(trans)[None])
    view = D.camera(W, H)
    im = body.images(DEV)
    screen, normals = torch.empty_like(vertices), torch.empty_like(vertices)
    K.mesh_vertices(vertices, im["faces"], im["adj_start"], im["adj_faces"], T * DN, 70, 120, view.reshape(-1).tolist(), screen, normals)
    assert torch.equal(SH.vertex_normals(body, vertices).view(torch.int32), normals.view(torch.int32))
    s, n = screen.cpu().numpy(), normals.cpu().numpy()
    faces = body.faces.astype(np.int32)
    head = -view[2, :3].astype(np.float64)
    head /= np.linalg.norm(head)
    head /= np.linalg.norm(head)                                          # draw_bodies normalises, and make_shade_style once more
    frames = SH.draw_bodies(body, vertices, DN, width=W, height=H)
    assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (1, T, H, W, 3)
    _check_frames(frames.cpu().numpy(), s, n, faces, DN, W, H, "draw_bodies", style=dict(ambient=0.35, light=tuple(head)))
    assert torch.equal(frames, SH.draw_bodies(body, vertices, DN, width=W, height=H))
    # every keyword reaches the kernel: another camera, palette, page, ambient term and light, and a picture below
    view2 = D.camera(W, H, elev=10.0, azim=-60.0, span=3.0)
    K.mesh_vertices(vertices, im["faces"], im["adj_start"], im["adj_faces"], T * DN, 70, 120, view2.reshape(-1).tolist(), screen, None)
    under = torch.randint(0, 256, (1, T, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(DEV)
    kw = dict(view=view2, colors=[(250, 10, 10)], background=(1, 2, 3), ambient=0.1, light=(3.0, 0.0, 4.0))
    other = SH.draw_bodies(body, vertices, DN, width=W, height=H, under=under, **kw)
    _check_frames(other.cpu().numpy(), screen.cpu().numpy(), n, faces, DN, W, H, "keywords", colors=kw["colors"],
                  style=dict(background=(1, 2, 3), ambient=0.1, light=(0.6, 0.0, 0.8)), under=under.cpu().numpy())
    plain = SH.draw_bodies(body, vertices, DN, width=W, height=H, **kw)
    covered = (plain != torch.tensor([1, 2, 3], dtype=torch.uint8, device=DEV)).any(-1)
    assert torch.equal(plain[covered], other[covered]) and torch.equal(other[~covered], under[~covered]) and (~covered).any()
    same_view = SH.draw_bodies(body, vertices, DN, width=W, height=H, elev=10.0, azim=-60.0, span=3.0, colors=kw["colors"],
                               background=(1, 2, 3), ambient=0.1, light=(3.0, 0.0, 4.0))
    assert torch.equal(same_view, plain)


def test_argument_refusals():
    body = _lattice_body()
    v = torch.zeros(1, 2 * DN, 70, 3, device=DEV)
    ok = SH.draw_bodies(body, v, DN, width=16, height=8)
    assert tuple(ok.shape) == (1, 2, 8, 16, 3) and (ok == 255).all()      # every triangle has zero area: the page
    for bad in (dict(dn=3), dict(width=0), dict(height=40000), dict(colors=[(1, 2)]), dict(view=np.zeros((4, 3))), dict(ambient=2.0),
                dict(light=(0, 0, 0)), dict(background=(0, 0, 256)), dict(under=torch.zeros(1, 2, 8, 16, 3, device=DEV)),
                dict(under=torch.zeros(1, 2, 8, 17, 3, dtype=torch.uint8, device=DEV)), dict(under=torch.zeros(1, 2, 8, 16, 3, dtype=torch.uint8))):
        kw = dict(dict(dn=DN, width=16, height=8), **bad)
        with pytest.raises(L.TcdiffError):
            SH.draw_bodies(body, v, kw.pop("dn"), **kw)
    with pytest.raises(L.TcdiffError):
        SH.draw_bodies(body, v[:, :, :69], DN)
    with pytest.raises(L.TcdiffError):
        SH.vertex_normals(body, v.cpu())
    c = R.case("one-dancer")
    args = dict(screen=_t(c["screen"]), normals=_t(c["normals"]), faces=_t(c["faces"]), b=1, T=2, dn=1, V=70, F=120, W=33, H=17,
                colors=_t(c["colors"], np.uint8), n_colors=5, style=_style({}), under=None,
                scratch=torch.empty(SH.scratch_bytes(1, 2, 1, 120) // 4, dtype=torch.int32, device=DEV), frames=torch.empty(1, 2, 17, 33, 3, dtype=torch.uint8, device=DEV))
    K.mesh_raster(**args)
    for change in (dict(screen=None), dict(normals=None), dict(faces=None), dict(colors=None), dict(style=None), dict(frames=None),
                   dict(scratch=None), dict(scratch=torch.empty(SH.scratch_bytes(1, 2, 1, 120) // 4 - 1, dtype=torch.int32, device=DEV)), dict(n_colors=0), dict(T=0)):
        with pytest.raises(L.TcdiffError):
            K.mesh_raster(**{**args, **change})
    with pytest.raises(L.TcdiffError, match="unsupported"):
        K.mesh_raster(**{**args, "W": 40000})
    torch.cuda.synchronize()


# ---- render_sample(..., draw_out=dir) with diffusion.body = model; write_draw_out(..., body=model) ---------------------------------
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
    seq = 60
    sd = O.synth_state_dict(dn=DN, seq_len=seq)
    model = DanceDecoder(nfeats=151, seq_len=seq, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=F.gelu, required_dancer_num=DN)
    model.load_state_dict(sd)
    return GaussianDiffusion(model, seq, 151, None, schedule="cosine", n_timestep=100, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=seq).to(DEV).eval()


def test_render_sample_draws_the_bodies_it_was_given(diffusion, tmp_path):
    """render_sample's parameter list is pinned (tests/test_gltf_cpu.py, tests/test_draw_cpu.py), so the body is the attribute
    ``diffusion.body``; write_draw_out takes it as the keyword ``body=`` with export_poses' q and pos"""
    body = B.load_body_model(S.make_model(40, 3, seed=2, smpl_tree=True), device=DEV)
    g = torch.Generator().manual_seed(5)
    norm = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
    frames_n = 6
    x = torch.rand(2, frames_n * DN, 151, generator=g) * 2 - 1
    names = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]
    kw = dict(name=names, required_dancer_num=DN)
    files = D.draw_out_names("normal", 7, names)
    want = SH.draw_body_samples(x.to(DEV), norm, DN, body).cpu().numpy()
    stick = D.draw_samples(x.to(DEV), norm, DN).cpu().numpy()
    assert want.shape == (2, frames_n, 480, 480, 3) and (want != stick).any(-1).mean() > 0.002
    assert diffusion.body is None
    # no body: today's bytes, the stick picture through write_apng; body=None on write_draw_out likewise
    assert diffusion.render_sample(x, None, norm, 7, None, draw_out=str(tmp_path / "plain"), **kw) is x
    q, pos, poses, contacts = E.export_poses(x.to(DEV), norm, "normal", DN)
    D.write_draw_out(str(tmp_path / "none"), "normal", 7, names, poses, contacts, body=None, q=q, pos=pos)
    for num, f in enumerate(files):
        D.write_apng(tmp_path / "direct.png", stick[num])
        today = (tmp_path / "direct.png").read_bytes()
        assert (tmp_path / "none" / f).read_bytes() == today and (tmp_path / "plain" / f).read_bytes() == today
    with pytest.raises(L.TcdiffError, match="q and pos"):
        D.write_draw_out(str(tmp_path / "bad"), "normal", 7, names, poses, contacts, body=body)
    written = D.write_draw_out(str(tmp_path / "keyword"), "normal", 7, names, poses, contacts, body=body, q=q, pos=pos)
    assert [os.path.basename(w) for w in written] == files
    diffusion.body = body
    try:
        ret = diffusion.render_sample(x, None, norm, 7, None, draw_out=str(tmp_path / "bodies"), **kw)
        assert ret is x                                                   # the samples, as without a body
        assert sorted(os.listdir(tmp_path / "bodies")) == sorted(files)
        for num, f in enumerate(files):
            got, info = draw_ref.decode_apng(tmp_path / "bodies" / f)
            assert np.array_equal(got, want[num]), f
            assert info == dict(plays=0, delays=[(1, 30)] * frames_n, n_frames=frames_n)
            assert (tmp_path / "keyword" / f).read_bytes() == (tmp_path / "bodies" / f).read_bytes()
        # a body without draw_out draws nothing; long mode: one song, its first render_len frames
        assert diffusion.render_sample(x, None, norm, 7, None, **kw) is x and not (tmp_path / "render").exists()
        x3 = torch.rand(3, 8 * DN, 151, generator=g) * 2 - 1
        diffusion.render_sample(x3, None, norm, 3, None, mode="long", required_dancer_num=DN, render_len=5,
                                name=["data/test/features/gLH_sBM_c01_d16_mLH2_ch04_slice0.npy"], draw_out=str(tmp_path / "long"))
    finally:
        diffusion.body = None
    assert os.listdir(tmp_path / "long") == ["3_gLH_sBM_c01_d16_mLH2_ch04.png"]
    got, info = draw_ref.decode_apng(tmp_path / "long" / "3_gLH_sBM_c01_d16_mLH2_ch04.png")
    # (the song's first 5 frames drawn as a clip of 5, as write_draw_out cuts it: a foot marker's last frame has no next frame)
    q, pos, full, none = E.export_poses(x3.to(DEV), norm, "long", DN)
    assert none is None and tuple(full.shape) == (1, DN, 16, 24, 3)
    want = SH.draw_body_poses(body, q[:, :5 * DN], pos[:, :5 * DN], full[:, :, :5], None, DN)
    assert info["n_frames"] == 5 and np.array_equal(got, want[0].cpu().numpy())
    assert tuple(SH.draw_body_samples(x3.to(DEV), norm, DN, body, mode="long", width=64, height=48).shape) == (1, 16, 48, 64, 3)
