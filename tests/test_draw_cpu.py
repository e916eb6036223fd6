"""The float64 restatement of the stick-figure frames (tests/draw_ref.py) on pictures that can be checked by hand, the camera
against known points, the seeded inputs the GPU tests use, the animated-PNG writer against a decoder written here, and the host
side of tcdiff_amd/draw.py.  No GPU."""
import inspect

import numpy as np
import pytest
import torch

import draw_ref as R
import tcdiff_amd
from tcdiff_amd import _lib as L
from tcdiff_amd import draw as D

IMAGES = [(100, 76), (33, 17), (32, 32)]                  # the GPU tests' images: two that are no multiple of the tile, one tile


# ---- hand-checkable pictures -------------------------------------------------------------------------------------------------
def _seg(ax, ay, bx, by, hw, alpha=1.0, rgb=(0, 0, 0)):
    return (float(ax), float(ay), float(bx), float(by), float(hw), float(alpha), rgb)


def test_horizontal_segment_through_pixel_centres():
    """a black segment from (3.5, 5.5) to (8.5, 5.5) on white.  Half-width 1: coverage clamp(1.5 - dist, 0, 1) is 1 on row 5,
    0.5 on rows 5 +- 1 (the ramp is one pixel wide about the edge at distance hw) and 0 on rows 5 +- 2.  Half-width 1.75: clamp(2.25 - dist, 0, 1) puts rows 5 +- 2 on the ramp at 0.25, and the
    ends are discs about a and b"""
    c, touch = R.paint([_seg(3.5, 5.5, 8.5, 5.5, 1.0)], 12, 11)
    img = R.to_bytes(c)
    assert (img[5, 3:9] == 0).all() and (c[5, 3:9] == 0).all()                    # distance 0: full coverage
    assert (c[4, 3:9] == 127.5).all() and (c[6, 3:9] == 127.5).all() and (img[4, 3:9] == 128).all()      # distance 1 = hw: half
    assert (img[3, 3:9] == 255).all() and (img[7, 3:9] == 255).all()             # distance 2 >= 1.5
    assert (touch[4:7, 3:9] == 1).all() and touch[0, 0] == 0
    c, _ = R.paint([_seg(3.5, 5.5, 8.5, 5.5, 1.75)], 12, 11)
    assert (c[3:8, 3:9][[1, 2, 3]] == 0).all()
    assert np.allclose(c[3, 3:9], 255 * 0.75, atol=1e-12) and np.allclose(c[7, 3:9], 255 * 0.75, atol=1e-12)      # 2.25 - 2 = 0.25
    assert R.to_bytes(c)[3, 4, 0] == 191                                         # 191.25 -> 191
    # the ends are discs: left of a = (3.5, 5.5) the distance is to a itself
    assert np.allclose(c[5, 2], 0.0)                                             # distance 1 along the row
    assert np.allclose(c[5, 1], 255 * 0.75, atol=1e-12)                          # distance 2: coverage 0.25
    assert np.allclose(c[5, 0], 255.0)                                           # distance 3
    assert np.allclose(c[4, 1], 255 * (1 - (2.25 - np.hypot(2.0, 1.0))), atol=1e-12)      # off the end, diagonally
    assert np.allclose(c[3, 1], 255.0)                                           # (2, 2) away: 2.83 > 2.25 -- a square cap would cover it
    assert np.allclose(c[3, 10], 255.0) and np.allclose(c[5, 10], 255 * 0.75, atol=1e-12)      # the same about b


def test_zero_length_segment_is_a_disc_and_alpha_scales_coverage():
    c, touch = R.paint([_seg(5.5, 5.5, 5.5, 5.5, 2.0, 0.5, (255, 0, 0))], 11, 11)
    Y, X = np.meshgrid(np.arange(11) + 0.5, np.arange(11) + 0.5, indexing="ij")
    cov = np.clip(2.5 - np.hypot(X - 5.5, Y - 5.5), 0, 1) * 0.5
    assert np.allclose(c[..., 0], 255.0) and np.allclose(c[..., 1], 255 - 255 * cov, atol=1e-12)
    assert np.array_equal(touch > 0, np.hypot(X - 5.5, Y - 5.5) < 2.5 + R.TOUCH_MARGIN)
    assert c[5, 5, 1] == 127.5 and R.to_bytes(c)[5, 5, 1] == 128                  # (uint8)(c + 0.5)


def test_later_primitive_is_on_top():
    red, blue = (255, 0, 0), (0, 0, 255)
    a = _seg(1.5, 5.5, 9.5, 5.5, 1.0, 1.0, red)
    b = _seg(5.5, 1.5, 5.5, 9.5, 1.0, 1.0, blue)
    assert tuple(R.to_bytes(R.paint([a, b], 11, 11)[0])[5, 5]) == blue
    assert tuple(R.to_bytes(R.paint([b, a], 11, 11)[0])[5, 5]) == red
    c, touch = R.paint([a, b], 11, 11)
    assert touch[5, 5] == 2 and tuple(R.to_bytes(c)[5, 2]) == red and tuple(R.to_bytes(c)[2, 5]) == blue
    # a half-transparent layer mixes with what is under it: c += cov * (src - c)
    c, _ = R.paint([a, _seg(5.5, 1.5, 5.5, 9.5, 1.0, 0.25, blue)], 11, 11)
    assert np.allclose(c[5, 5], [255 * 0.75, 0, 255 * 0.25])


def test_paint_order_of_a_frame():
    """static segments, then trails by dancer index (trail_len limits them), then bodies by the painter's order"""
    T, dn = 4, 2
    pts = np.arange(T * dn * 24 * 3, dtype=np.float64).reshape(T, dn, 24, 3)
    trail = np.arange(T * dn * 2, dtype=np.float64).reshape(T, dn, 2)
    order = np.array([[1, 0]] * T)
    planted = np.zeros((T, dn, 4), np.uint8)
    planted[3, 1, 2] = 1
    st = np.array([[0, 0, 1, 1]], np.float32)
    prims = R.primitives(pts, trail, order, planted, 3, st)
    assert len(prims) == 1 + dn * 3 + dn * 27
    assert prims[0][6] == R.STYLE["static_rgb"]
    assert [p[6] for p in prims[1:7]] == [R.PALETTE[0]] * 3 + [R.PALETTE[1]] * 3
    assert prims[1][:4] == (*trail[0, 0], *trail[1, 0]) and prims[6][:4] == (*trail[2, 1], *trail[3, 1])
    body = prims[7:]
    assert all(p[6] == R.PALETTE[1] for p in body[:23]) and all(p[6] == R.PALETTE[0] for p in body[27:50])
    assert body[0][:4] == (*pts[3, 1, 1, :2], *pts[3, 1, 0, :2]) and body[22][:4] == (*pts[3, 1, 23, :2], *pts[3, 1, 21, :2])
    assert [p[6] for p in body[23:27]] == [R.STYLE["free_rgb"]] * 2 + [R.STYLE["planted_rgb"], R.STYLE["free_rgb"]]
    assert body[25][:2] == body[25][2:4] == tuple(pts[3, 1, 10, :2])
    assert len(R.primitives(pts, trail, order, planted, 3, None, dict(trail_len=2, markers=0))) == dn * 2 + dn * 23
    assert len(R.primitives(pts, trail, order, planted, 0, None)) == dn * 27      # frame 0 has no trail
    # five dancers at frame 59: more than one chunk of 256
    assert 5 * 23 + 20 + 5 * 59 == 430


# ---- camera --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", [R.camera, lambda *a, **k: D.camera(*a, **k)], ids=["restatement", "draw.py"])
def test_camera_on_known_points(cam):
    W, H, span, elev = 100, 76, 4.0, 40.0
    m = cam(W, H).astype(np.float64)
    assert m.shape == (3, 4) and cam(W, H).dtype == np.float32
    s = min(W, H) / span
    at = lambda p: m @ np.array([*p, 1.0])
    c = at((0.0, 0.0, 1.0))
    assert np.allclose(c, [W / 2, H / 2, 0.0], atol=1e-4)                       # the centre lands in the middle
    px = at((1.0, 0.0, 1.0))
    assert np.allclose(px - c, [s, 0.0, 0.0], atol=1e-4)                        # +x goes right, by s pixels per metre
    pz = at((0.0, 0.0, 2.0))
    assert np.allclose(pz[:2] - c[:2], [0.0, -s * np.cos(np.radians(elev))], atol=1e-4)      # +up moves up by s cos(elev)
    py = at((0.0, 1.0, 1.0))                                                    # azim -90 looks along +y: +y is farther and higher
    assert py[2] > c[2] and np.allclose(py[2] - c[2], np.cos(np.radians(elev)), atol=1e-6)
    assert np.allclose(py[:2] - c[:2], [0.0, -s * np.sin(np.radians(elev))], atol=1e-4)
    assert pz[2] < c[2]                                                         # seen from above: higher is nearer
    top = cam(W, H, elev=90.0, azim=-90.0).astype(np.float64)                   # straight down: the floor plane undistorted
    assert np.allclose(top @ [1.0, 1.0, 0.0, 1.0] - top @ [0.0, 0.0, 0.0, 1.0], [s, -s, 0.0], atol=1e-4)
    # another up axis: the same picture of the cyclically renamed point
    y_up = cam(W, H, center=(0.0, 1.0, 0.0), up=1).astype(np.float64)
    assert np.allclose(y_up @ [0.4, 1.7, 0.3, 1.0], at((0.3, 0.4, 1.7)), atol=1e-4)


def test_camera_and_grid_of_draw_py_are_the_restatement_s():
    for W, H in IMAGES + [(480, 480)]:
        v = D.camera(W, H)
        assert np.allclose(v, R.camera(W, H), rtol=0, atol=1e-5)
        g = D.floor_grid(v)
        assert g.shape == (10, 4) and g.dtype == np.float32 and np.allclose(g, R.grid(v), rtol=0, atol=1e-4)
    g = D.floor_grid(D.camera(100, 100, elev=90.0), span=4.0).astype(np.float64)
    assert sorted(set(np.round(g[:5, 0]).tolist())) == [0.0, 25.0, 50.0, 75.0, 100.0]      # a line every metre over the span


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seeded_inputs_have_no_near_ties(shape):
    joints, contacts = R.synth(*shape)
    assert joints.dtype == np.float32 and joints.shape == shape + (24, 3) and contacts.shape == shape + (4,)
    for W, H in IMAGES:
        v = R.camera(W, H)
        assert R.decisions_clear(joints, contacts, v) and R.decisions_clear(joints, None, v), (shape, W, H)


def test_seeded_inputs_hold_the_cases_they_are_for():
    joints, contacts = R.synth(1, 5, 60)
    W, H = 100, 76
    p = R.project(joints, contacts, R.camera(W, H))
    assert len({tuple(o) for o in p["order"][0]}) > 3                           # the painter's order changes along the clip
    assert np.array_equal(joints[0, 0, :, 22], joints[0, 0, :, 20])             # a bone of zero length
    assert (joints[0, 2] == joints[0, 2, :1]).all()                             # a dancer who stands still
    last = p["pts"][0, :, 4]
    assert last[-1, :, 0].max() < 0 and last[-1, :, 1].max() < 0 and 0 < last[0, 0, 0] < W      # out past the left and the top
    assert np.abs(p["pts"][..., :2]).max() < R.MAX_COORD
    free = R.project(joints, None, R.camera(W, H))["planted"]
    assert 0.2 < free.mean() < 0.95 and 0.2 < p["planted"].mean() < 0.8         # planted decisions go both ways
    assert (free[0, :, 2] == 1).all() and (free[0, -1] == 1).all()
    assert not R.decisions_clear(joints, np.full_like(contacts, 0.95), R.camera(W, H))
    tie = joints.copy()
    tie[0, 1] = tie[0, 0]
    assert not R.decisions_clear(tie, contacts, R.camera(W, H))                 # two dancers at one depth


# ---- APNG ----------------------------------------------------------------------------------------------------------------------
decode_apng = R.decode_apng          # the decoder lives next to the restatement: the GPU tests read render_sample's files with it


@pytest.mark.parametrize("T", [1, 3])
def test_write_apng_round_trip(T, tmp_path):
    g = np.random.default_rng(T)
    frames = g.integers(0, 256, (T, 5, 7, 3), dtype=np.uint8)                   # 5 rows of 7 pixels
    path = D.write_apng(tmp_path / "a.png", frames, fps=30)
    got, info = decode_apng(path)
    assert got.shape == (T, 5, 7, 3) and np.array_equal(got, frames)
    assert info == dict(plays=0, delays=[(1, 30)] * T, n_frames=T)              # 1 / fps seconds, looping forever
    _, info = decode_apng(D.write_apng(tmp_path / "b.png", torch.from_numpy(frames), fps=12.5))
    assert info["delays"] == [(2, 25)] * T
    for bad in (frames.astype(np.int32), frames[0], frames[..., :2]):
        with pytest.raises(L.TcdiffError):
            D.write_apng(tmp_path / "c.png", bad)
    with pytest.raises(L.TcdiffError):
        D.write_apng(tmp_path / "c.png", frames, fps=0)
    assert not (tmp_path / "c.png").exists()


# ---- the host side of draw.py -------------------------------------------------------------------------------------------------
def test_public_names():
    for name in ("camera", "draw_dance", "draw_samples", "write_apng"):
        assert name in tcdiff_amd.__all__ and getattr(tcdiff_amd, name) is getattr(D, name)
    for sym in ("tcdiff_draw_project", "tcdiff_draw_raster"):
        assert sym in L.EXPORTS
    sig = inspect.signature(tcdiff_amd.GaussianDiffusion.render_sample)
    assert sig.parameters["draw_out"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["draw_out"].default is None
    assert list(sig.parameters)[-1] == "draw_out"                               # the positional arguments are untouched
    assert np.array_equal(np.asarray(D.PALETTE), np.asarray(R.PALETTE)) and list(D.SMPL_PARENTS) == R.PARENTS


def test_draw_dance_refuses_off_the_gpu_and_bad_arguments():
    joints = torch.zeros(1, 2, 3, 24, 3)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        D.draw_dance(joints)
    with pytest.raises(L.TcdiffError, match="MI355X only"):
        D.draw_samples(torch.zeros(1, 6, 151), None, 2)
    with pytest.raises(L.TcdiffError, match="float32"):
        D.draw_dance(joints.double())
    with pytest.raises(L.TcdiffError, match="must be"):
        D.draw_dance(torch.zeros(1, 2, 3, 24, 2))
    with pytest.raises(L.TcdiffError, match="contiguous"):
        D.draw_dance(torch.zeros(1, 2, 3, 3, 24).transpose(-1, -2))
    with pytest.raises(L.TcdiffError, match="must be"):
        D.draw_dance(joints, torch.zeros(1, 2, 4, 4))
    with pytest.raises(L.TcdiffError, match="empty"):
        D.draw_dance(torch.zeros(1, 0, 3, 24, 3))
    with pytest.raises(L.TcdiffError):
        D.camera(0, 10)
    with pytest.raises(L.TcdiffError):
        D.camera(10, 10, up=3)
    for kw in (dict(line_width=-1.0), dict(trail_alpha=1.5), dict(background=(0, 0, 256)), dict(marker_radius=1e9)):
        with pytest.raises(L.TcdiffError):
            D.make_style(**kw)
    st = D.make_style(line_width=6.0, trail_len=7, markers=False)
    assert (st.line_hw, st.trail_hw, st.marker_radius, st.trail_len, st.markers) == (3.0, 1.5, 6.0, 7, 0)
    assert tuple(st.background) == (255, 255, 255) and tuple(st.planted_rgb) == (255, 0, 0)
    ref = D.make_style()                                                        # the defaults are the restatement's STYLE
    for k, v in R.STYLE.items():
        got = getattr(ref, k)
        assert (tuple(got) if isinstance(v, tuple) else got) == pytest.approx(v), k


def test_file_names_render_sample_would_write():
    names = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]
    assert D.draw_out_names("normal", 7, names) == ["e7_b0_gBR_sBM_c01_d04_mBR0_ch01_slice3.png", "e7_b1_npy_gLO_slice12.png"]
    assert D.draw_out_names("ctrl", 7, names[:1]) == ["e7_b0_gBR_sBM_c01_d04_mBR0_ch01_slice3.png"]
    assert D.draw_out_names("long", 3, ["data/test/features/gLH_sBM_c01_d16_mLH2_ch04_slice0.npy"]) == ["3_gLH_sBM_c01_d16_mLH2_ch04.png"]
    with pytest.raises(L.TcdiffError):
        D.draw_out_names("normal", 1, None)
