"""tcdiff_draw_project / tcdiff_draw_raster (csrc/draw.hip) and tcdiff_amd/draw.py on an MI355X against the numpy float64
restatement tests/draw_ref.py, which is written from the picture's definition in include/tcdiff_hip.h.

Projection.  The kernel evaluates row . (X, Y, Z, 1) as three float32 fused multiply-adds, each rounding at most 2^-24 of a
partial sum that is itself at most sum |terms| (1 + 2^-23): within 3 * 2^-24 * sum |terms| (1 + 2^-22) < 4 * 2^-24 * sum |terms| of
the exact value, which is the bound the restatement returns per value.  `order` and `planted` must be equal, no exclusions:
`decisions_clear` (tests/test_draw_cpu.py) shows that no depth pair is closer than both bounds and no planted decision is within
1e-6 / 1e-9 of its threshold on the seeded inputs.

Raster: the per-layer error delta_r.  The kernel works in float64 (u = 2^-53) on float32 inputs; |coordinates| < M = 4096 (asserted
on the inputs).  Per pixel and primitive, with e = p - a, d = b - a, |e|, |d| <= 2 sqrt2 M:
  d, e: one rounding each; |d|^2 three, 1 / |d|^2 one more (relative 5 u); e . d: absolute 4 u (|ex dx| + |ey dy|) <= 4 sqrt2 u |e| |d|;
  parameter (e . d) * inv: its error times |d| is at most (4 sqrt2 + 6) u |e| < 12 u |e| (the clamp to [0, 1] is 1-Lipschitz);
  e - param * d: two more roundings per component, so each component of p - q is within 12 u |e| + 2 u (|e| + |d|) + u 2 M < 48 u M,
  the vector within 68 u M; the square root of the sum of squares: relative 3 u of a distance <= 4 M: 80 u M in all;
  (hw + 0.5) - dist: hw + 0.5 is exact, one rounding: 84 u M; min(., 1) * alpha: coverage within 84 u M + u;
  c += cov * (src - c): |src - c| <= 255, three roundings: 255 (84 u M + u) + 3 * 255 u = 255 u (84 M + 4) = 9.8e-9 levels.
An error already in c passes through a layer with the factor 1 - cov <= 1, a primitive whose exact coverage is 0 by more than
1e-6 (it does not "touch") computes exactly 0, and c + 0.5 adds 256 u.  The restatement does the same operations in float64 with
at most the same error, so delta_r = 2e-8 levels per touching layer covers both sides.  float32 in the kernel would give
~0.1 levels per layer and an equality test of nothing; that is why the kernel blends in float64.
A pixel is clear when every channel of the restatement's unrounded value is at least n_touch * delta_r from a rounding boundary
(x.5).  Asserted: every pixel within 1 level, every clear pixel equal, and -- on the restatement alone, before the GPU is
touched -- clear pixels at least 90 % of the touched ones (the restatement gives 98.8 % on the 33 x 17 image with its grid, where a few grid
pixels are exact ties, and 100 % on the other five cases).

End to end (draw_dance on the float32 joints against raster(project(.)) in float64 throughout): coverage is 1-Lipschitz in an
endpoint's position, so delta = n_touch * (255 * B + delta_r) with B the largest projection bound |(bound_x, bound_y)| of any
joint or trail point of the clip.  At 100 x 76 B = 4.8e-5 pixels, delta = 0.0121 levels per touching layer, and the restatement
gives a clear share of 94.2 % with contacts and 94.7 % without on frames 0, 1 and 59."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import draw_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import draw as D
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTA_R = 2e-8
CLEAR_SHARE = 0.90
BIG = (1, 5, 60)
FRAMES = [0, 1, 59]
SENTINEL = 0xA5
_projected = {}


def _ref_projection(shape, W, H, with_contacts=True):
    key = (shape, W, H, with_contacts)
    if key not in _projected:
        joints, contacts = R.synth(*shape)
        view = R.camera(W, H)
        assert R.decisions_clear(joints, contacts if with_contacts else None, view), "a decision of the reference is a near-tie"
        _projected[key] = (view, R.project(joints, contacts if with_contacts else None, view))
    return _projected[key]


def _gpu_project(joints, contacts, view, **kw):
    b, dn, T = joints.shape[:3]
    pts = torch.full((b, T, dn, 24, 3), float("nan"), device=DEV)
    trail = torch.full((b, T, dn, 2), float("nan"), device=DEV)
    order = torch.full((b, T, dn), -1, dtype=torch.int32, device=DEV)
    planted = torch.full((b, T, dn, 4), 7, dtype=torch.uint8, device=DEV)
    K.draw_project(joints, contacts, np.asarray(view).reshape(-1).tolist(), kw.get("floor", 0.0), kw.get("up", 2),
                   kw.get("contact_threshold", 0.95), kw.get("still", 0.01), pts, trail, order, planted)
    torch.cuda.synchronize()
    return pts.cpu().numpy(), trail.cpu().numpy(), order.cpu().numpy(), planted.cpu().numpy()


def _compare_projection(got, want, what):
    pts, trail, order, planted = got
    for name, g, w, bound in (("pts", pts, want["pts"], want["pts_bound"]), ("trail", trail, want["trail"], want["trail_bound"])):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name)
        ratio = np.abs(g.astype(np.float64) - w) / bound
        print(f"[draw] {what} {name}: worst error / bound {ratio.max():.3f}")
        assert (ratio <= 1.0).all(), (what, name, float(ratio.max()))
    assert np.array_equal(order, want["order"]), what
    assert np.array_equal(planted, want["planted"]), what


@pytest.mark.parametrize("with_contacts", [True, False], ids=["contacts", "displacement"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_projection_against_the_float64_restatement(shape, with_contacts):
    view, want = _ref_projection(shape, 100, 76, with_contacts)
    joints, contacts = (torch.from_numpy(a).to(DEV) for a in R.synth(*shape))
    _compare_projection(_gpu_project(joints, contacts if with_contacts else None, view), want, (shape, with_contacts))


def test_projection_reads_a_frame_major_buffer_in_place_and_other_parameters():
    shape = (2, 3, 5)
    view, want = _ref_projection(shape, 100, 76)
    joints, contacts = (torch.from_numpy(a).to(DEV) for a in R.synth(*shape))
    jv = joints.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)          # (b, T, dn, 24, 3) storage
    cv = contacts.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not jv.is_contiguous() and not cv.is_contiguous()
    first = _gpu_project(joints, contacts, view)
    for a, c in zip(_gpu_project(jv, cv, view), first):
        assert np.array_equal(a, c)
    _compare_projection(first, want, "permuted view")
    # a floor above 0, a lower contact threshold and a larger `still`
    j, c = R.synth(*shape)
    kw = dict(floor=0.25, contact_threshold=0.5, still=0.05)
    assert R.decisions_clear(j, c, view, **kw) and R.decisions_clear(j, None, view, **kw)
    _compare_projection(_gpu_project(joints, contacts, view, **kw), R.project(j, c, view, **kw), kw)
    _compare_projection(_gpu_project(joints, None, view, **kw), R.project(j, None, view, **kw), kw)


def _style(d):
    st = L.DrawStyle()
    for k, v in dict(R.STYLE, **d).items():
        setattr(st, k, (L.C.c_ubyte * 3)(*v) if isinstance(v, tuple) else v)
    return st


def _raster_in_sentinels(p32, W, H, style, static, offset, colors=R.PALETTE, parents=R.PARENTS):
    """runs the raster with `frames` placed `offset` bytes into a larger buffer of sentinel bytes; returns the frames (b, T, H, W, 3)
    after checking that no sentinel changed"""
    pts, trail, order, planted = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in p32)
    b, T, dn = order.shape
    n = b * T * H * W * 3
    buf = torch.full((offset + n + 4096,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    seg = None if static is None else torch.from_numpy(static).to(DEV)
    pal = torch.tensor(colors, dtype=torch.uint8, device=DEV)
    K.draw_raster(pts, trail, order, planted, b, dn, T, W, H, parents, seg, 0 if static is None else len(static), pal, len(colors),
                  _style(style), buf.data_ptr() + offset)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:offset] == SENTINEL).all() and (host[offset + n:] == SENTINEL).all(), "bytes outside frames were written"
    return host[offset:offset + n].reshape(b, T, H, W, 3)


def _check_picture(got, values, touch, delta, what):
    """got (n, H, W, 3) uint8 against the restatement's unrounded values: all within a level, the clear ones equal"""
    want = R.to_bytes(values)
    clear = R.clear_mask(values, touch, delta)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64)).max(-1)
    print(f"[draw] {what}: {int((touch > 0).sum())} touched pixels, {int((diff > 0).sum())} differ, "
          f"{int((diff[clear] > 0).sum())} of them clear, worst {int(diff.max())} level(s)")
    assert diff.max() <= 1, what
    assert (diff[clear] == 0).all(), what


def _assert_clear_share(values, touch, delta, what):
    touched = touch > 0
    share = float((R.clear_mask(values, touch, delta) & touched).sum() / touched.sum())
    print(f"[draw] {what}: clear share {share:.4f} of {int(touched.sum())} touched pixels")
    assert share >= CLEAR_SHARE, (what, share)


RASTER_CASES = [
    (100, 76, {}, True, 64),                                  # rows of a multiple of 4 pixels on a 4-byte boundary: dword stores
    (100, 76, {"trail_len": 7}, True, 7),                     # the same rows off the boundary: byte stores
    (100, 76, {"markers": 0}, False, 64),                     # n_static = 0
    (33, 17, {}, True, 64),                                   # partial tiles in both directions
    (33, 17, {"trail_len": 7, "markers": 0}, False, 3),
    (32, 32, {}, True, 64),                                   # exactly one tile
]


@pytest.mark.parametrize("W,H,style,grid,offset", RASTER_CASES,
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) or "default" if isinstance(v, dict) else str(v))
def test_raster_on_the_restatement_s_projection(W, H, style, grid, offset):
    """the raster alone, fed the restatement's float32 pts / trail / order / planted; frame 59 has 430 primitives (+ 10 grid
    lines): more than one chunk of 256"""
    view, p = _ref_projection(BIG, W, H)
    p32 = (p["pts"].astype(np.float32), p["trail"].astype(np.float32), p["order"], p["planted"])
    assert np.abs(p32[0][..., :2]).max() < R.MAX_COORD and np.abs(p32[1]).max() < R.MAX_COORD
    static = R.grid(view) if grid else None
    assert len(R.primitives(p32[0][0], p32[1][0], p32[2][0], p32[3][0], 59, static, style)) > 256 or style.get("trail_len")
    values, touch = R.raster(p32[0][0], p32[1][0], p32[2][0], p32[3][0], W, H, FRAMES, static, style)
    _assert_clear_share(values, touch, DELTA_R, (W, H, style))               # on the restatement alone, before the GPU runs
    got = _raster_in_sentinels(p32, W, H, style, static, offset)
    _check_picture(got[0, FRAMES], values, touch, DELTA_R, (W, H, style, grid))
    again = _raster_in_sentinels(p32, W, H, style, static, offset)
    assert np.array_equal(got, again)                                        # same input, same bits
    if offset != 64:                                                         # dword and byte stores write the same picture
        assert np.array_equal(got, _raster_in_sentinels(p32, W, H, style, static, 64))


def test_raster_skips_what_is_not_a_dancer_or_not_finite():
    """an `order` entry outside [0, dn) and a NaN / infinite joint draw nothing and fault nothing; other palettes wrap"""
    W, H = 33, 17
    view, p = _ref_projection((2, 3, 5), W, H)
    pts, trail = p["pts"].astype(np.float32), p["trail"].astype(np.float32)
    order, planted = p["order"].copy(), p["planted"]
    order[0, 2, 0], order[1, 4, 2] = -5, 3
    pts[0, 1, 1, 4, 0], pts[1, 3, 0, 20, 1], trail[1, 2, 1, 0] = np.nan, np.inf, -np.inf
    colors = ((10, 20, 30), (200, 100, 0))
    got = _raster_in_sentinels((pts, trail, order, planted), W, H, {}, None, 5, colors)
    for c in range(2):
        values, touch = R.raster(pts[c], trail[c], order[c], planted[c], W, H, range(5), None, {}, colors)
        _check_picture(got[c], values, touch, DELTA_R, f"clip {c} with holes")


def test_draw_dance_end_to_end():
    W, H = 100, 76
    joints, contacts = R.synth(*BIG)
    for with_contacts in (True, False):
        view, p = _ref_projection(BIG, W, H, with_contacts)
        assert np.array_equal(D.camera(W, H), view) and np.array_equal(D.floor_grid(view), R.grid(view))
        B = max(float(np.hypot(p["pts_bound"][..., 0], p["pts_bound"][..., 1]).max()),
                float(np.hypot(p["trail_bound"][..., 0], p["trail_bound"][..., 1]).max()))
        delta = 255 * B + DELTA_R
        values, touch = R.raster(p["pts"][0], p["trail"][0], p["order"][0], p["planted"][0], W, H, FRAMES, R.grid(view))
        print(f"[draw] end to end: B {B:.2e} pixels, delta {delta:.4f} levels per touching layer")
        _assert_clear_share(values, touch, delta, ("end to end", with_contacts))
        frames = D.draw_dance(torch.from_numpy(joints).to(DEV), torch.from_numpy(contacts).to(DEV) if with_contacts else None,
                              width=W, height=H)
        assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (1, 60, H, W, 3)
        _check_picture(frames[0, FRAMES].cpu().numpy(), values, touch, delta, ("end to end", with_contacts))
        assert torch.equal(frames, D.draw_dance(torch.from_numpy(joints).to(DEV),
                                                torch.from_numpy(contacts).to(DEV) if with_contacts else None, width=W, height=H))
    # the keyword arguments reach the kernel: no grid, no markers, a short trail, another palette and page
    kw = dict(grid=False, markers=False, trail_len=7, colors=[(0, 0, 0), (255, 255, 0)], background=(10, 20, 30), line_width=3.0)
    view, p = _ref_projection(BIG, W, H, True)
    style = dict(markers=0, trail_len=7, background=(10, 20, 30), line_hw=1.5, trail_hw=0.75, marker_radius=3.0)
    values, touch = R.raster(p["pts"][0], p["trail"][0], p["order"][0], p["planted"][0], W, H, FRAMES, None, style, kw["colors"])
    frames = D.draw_dance(torch.from_numpy(joints).to(DEV), torch.from_numpy(contacts).to(DEV), width=W, height=H, **kw)
    _check_picture(frames[0, FRAMES].cpu().numpy(), values, touch, 255 * B + DELTA_R, kw)


def test_argument_refusals():
    b, dn, T, W, H = 1, 2, 3, 16, 8
    joints = torch.zeros(b, dn, T, 24, 3, device=DEV)
    pts, trail = torch.zeros(b, T, dn, 24, 3, device=DEV), torch.zeros(b, T, dn, 2, device=DEV)
    order, planted = torch.zeros(b, T, dn, dtype=torch.int32, device=DEV), torch.zeros(b, T, dn, 4, dtype=torch.uint8, device=DEV)
    pal = torch.zeros(5, 3, dtype=torch.uint8, device=DEV)
    frames = torch.zeros(b, T, H, W, 3, dtype=torch.uint8, device=DEV)
    view = R.camera(W, H).reshape(-1).tolist()
    ok = dict(joints=joints, contacts=None, view=view, floor=0.0, up=2, contact_threshold=0.95, still=0.01, pts=pts, trail=trail,
              order=order, planted=planted)
    K.draw_project(**ok)
    for change in (dict(view=None), dict(pts=None), dict(trail=None), dict(order=None), dict(planted=None), dict(up=3)):
        with pytest.raises(L.TcdiffError):
            K.draw_project(**{**ok, **change})
    lib = L.load()
    js = (L.C.c_long * 3)(*joints.stride()[:3])
    vw = (L.C.c_float * 12)(*view)
    args = lambda **kw: [kw.get("joints", joints.data_ptr()), kw.get("js", js), None, None, kw.get("b", b), kw.get("dn", dn),
                         kw.get("T", T), vw, 0.0, 2, 0.95, 0.01, pts.data_ptr(), trail.data_ptr(), order.data_ptr(),
                         planted.data_ptr(), K.stream()]
    assert lib.tcdiff_draw_project(*args()) == 0
    for kw in (dict(joints=None), dict(js=None), dict(b=0), dict(dn=0), dict(T=0)):
        assert lib.tcdiff_draw_project(*args(**kw)) == -1, kw
    a = args()
    a[2] = joints.data_ptr()                                  # contacts without their strides
    assert lib.tcdiff_draw_project(*a) == -1
    st = _style({})
    ok = dict(pts=pts, trail=trail, order=order, planted=planted, b=b, dn=dn, T=T, W=W, H=H, parents=R.PARENTS, static_segs=None,
              n_static=0, colors=pal, n_colors=5, style=st, frames=frames)
    K.draw_raster(**ok)
    torch.cuda.synchronize()
    bad = [dict(pts=None), dict(trail=None), dict(order=None), dict(planted=None), dict(parents=None), dict(colors=None),
           dict(style=None), dict(frames=None), dict(b=0), dict(dn=0), dict(T=0), dict(W=0), dict(H=0), dict(n_colors=0),
           dict(n_static=-1), dict(n_static=2), dict(parents=[0] * 23 + [24]), dict(parents=[0, -1] + [0] * 22),
           dict(style=_style({"line_hw": -1.0})), dict(style=_style({"trail_alpha": 1.5})), dict(style=_style({"static_alpha": -0.5})),
           dict(style=_style({"marker_radius": float("nan")}))]
    for change in bad:
        with pytest.raises(L.TcdiffError):
            K.draw_raster(**{**ok, **change})
    with pytest.raises(L.TcdiffError, match="unsupported"):
        K.draw_raster(**{**ok, "T": 65536})
    with pytest.raises(L.TcdiffError, match="one device|MI355X only"):
        D.draw_dance(joints, torch.zeros(b, dn, T, 4))
    with pytest.raises(L.TcdiffError, match="colors"):
        D.draw_dance(joints, colors=[(1, 2)])
    with pytest.raises(L.TcdiffError, match="view"):
        D.draw_dance(joints, view=np.zeros((4, 3)))
    torch.cuda.synchronize()


# ---- draw_samples and render_sample(..., draw_out=...) --------------------------------------------------------------------------
DN = 2


def _normalizer(scale, min_):
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_, n.scaler.min_ = scale.float(), min_.float()
    return n


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
    diff = GaussianDiffusion(model, S, 151, None, schedule="cosine", n_timestep=100, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=S).to(DEV).eval()
    cond = torch.stack([O.synth_cond(c, S) for c in range(2)])
    return diff, cond, S


def test_render_sample_draws_what_it_exported(diffusion, tmp_path):
    from tcdiff_amd import export as E
    diff, _, _ = diffusion
    g = torch.Generator().manual_seed(5)
    norm = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
    S = 8
    x = torch.rand(2, S * DN, 151, generator=g) * 2 - 1
    names = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]
    ret = diff.render_sample(x, None, norm, 7, str(tmp_path / "render"), name=names, required_dancer_num=DN,
                             draw_out=str(tmp_path / "draw"))
    assert ret is x
    assert sorted(os.listdir(tmp_path / "draw")) == ["e7_b0_gBR_sBM_c01_d04_mBR0_ch01_slice3.png", "e7_b1_npy_gLO_slice12.png"]
    assert not (tmp_path / "render").exists()                 # render_out still draws nothing
    want = D.draw_samples(x.to(DEV), norm, DN).cpu().numpy()
    assert want.shape == (2, S, 480, 480, 3) and want.min() < 255
    for num, f in enumerate(D.draw_out_names("normal", 7, names)):
        got, info = R.decode_apng(tmp_path / "draw" / f)
        assert np.array_equal(got, want[num]), f
        assert info == dict(plays=0, delays=[(1, 30)] * S, n_frames=S)
    # long mode: 3 half-overlapping windows are one song of 16 frames, of which the first render_len are drawn; with fk_out too
    x3 = torch.rand(3, S * DN, 151, generator=g) * 2 - 1
    diff.render_sample(x3, None, norm, 3, None, fk_out=str(tmp_path / "fk"), mode="long", required_dancer_num=DN, render_len=10,
                       name=["data/test/features/gLH_sBM_c01_d16_mLH2_ch04_slice0.npy"], draw_out=str(tmp_path / "long"))
    assert os.listdir(tmp_path / "long") == ["3_gLH_sBM_c01_d16_mLH2_ch04.png"]
    assert os.listdir(tmp_path / "fk") == ["3_gLH_sBM_c01_d16_mLH2_ch04.pkl"]
    _, _, full, none = E.export_poses(x3.to(DEV), norm, "long", DN)
    assert none is None and tuple(full.shape) == (1, DN, 16, 24, 3)
    got, info = R.decode_apng(tmp_path / "long" / "3_gLH_sBM_c01_d16_mLH2_ch04.png")
    assert info["n_frames"] == 10 and np.array_equal(got, D.draw_dance(full[:, :, :10])[0].cpu().numpy())
    assert tuple(D.draw_samples(x3.to(DEV), norm, DN, mode="long", width=64, height=48).shape) == (1, 16, 48, 64, 3)


def test_render_sample_returns_the_same_samples_with_and_without_draw_out(diffusion, tmp_path):
    diff, cond, S = diffusion
    shape = (2, S * DN, 151)
    norm = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
    torch.manual_seed(7)
    want = diff.render_sample(shape, cond, norm, 1, None, name=["a/b.npy", "a/c.npy"], required_dancer_num=DN)
    assert not (tmp_path / "none").exists()
    torch.manual_seed(7)
    got = diff.render_sample(shape, cond, norm, 1, None, name=["a/b.npy", "a/c.npy"], required_dancer_num=DN,
                             draw_out=str(tmp_path / "draw"))
    assert torch.equal(got, want)
    assert sorted(os.listdir(tmp_path / "draw")) == ["e1_b0_b.png", "e1_b1_c.png"]
    # draw_out without a normalizer: nothing to draw, no directory
    assert diff.render_sample(want, cond, required_dancer_num=DN, draw_out=str(tmp_path / "none")) is want
    assert not (tmp_path / "none").exists()
    frames, _ = R.decode_apng(tmp_path / "draw" / "e1_b1_c.png")
    assert np.array_equal(frames, D.draw_samples(want.to(DEV), norm, DN)[1].cpu().numpy())
