"""The choreography planner on the GPU (tcdiff_amd/choreo.py, csrc/choreo.hip) against the float64 restatement tests/choreo_ref.py of
include/tcdiff_choreo.h: every float32 output equal bits, every float64 report equal, every integer equal -- these are float64
operations in a stated order, so there is no tolerance -- and the round trip that ties it to the pipeline: a plan's x_0 written into
channels 4 and 5 of normalised samples, exported, and measured against the plan.

Measured on an MI355X (profiles/choreo.txt): every output equal on every case; the round trip comes back within 2.7e-7 m, where the
bound derived from the chain's float32 roundings is 1.2e-6 m."""
import numpy as np
import pytest
import torch

import choreo_ref as R
from tcdiff_amd import _lib as L
from tcdiff_amd import choreo as CH
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd.export import export_poses
from tcdiff_amd.group_metrics import pairs
from tcdiff_amd.metrics import summarize

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOATS32, FLOATS64 = ("traj", "x_0"), ("speed_max", "path_length", "dist_min")
INTS = ("status", "clamped", "speed_peak", "too_fast", "dist_min_frame", "too_close")
NORM = ([0.4, 0.55], [0.1, -0.2])          # scale_ and min_ of the two columns: waypoints within 3 m reach beyond [-1, 1] now and then
# (b, dn, frames, K), keys per dancer?, a normaliser?  A frame, a straight line, a tile boundary, the users' clip, LDS filled to the key
# limit across a tile boundary, the users' song (five tiles); one dancer has no pair
CASES = {"1x1x1-K1": ((1, 1, 1, 1), False, False), "1x1x2-K2": ((1, 1, 2, 2), True, True), "2x3x65-K3": ((2, 3, 65, 3), True, True),
         "1x3x150-K6": ((1, 3, 150, 6), False, True), "1x2x257-K256": ((1, 2, 257, 256), False, False), "1x3x1200-K40": ((1, 3, 1200, 40), True, True)}


class Norm:
    """a normaliser of n columns whose columns `cols` carry NORM"""
    def __init__(self, n, cols):
        scale, mn = torch.ones(n), torch.zeros(n)
        scale[list(cols)], mn[list(cols)] = torch.tensor(NORM[0]), torch.tensor(NORM[1])
        self.scaler = type("S", (), dict(scale_=scale, min_=mn))()


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cases are not changed


def check_plan(got: CH.Plan, ref, what):
    """every output of one call against the restatement: bits, NaNs included"""
    for k in FLOATS32:
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == np.float32 and g.shape == ref[k].shape
        assert np.array_equal(np.isnan(g), np.isnan(ref[k])) and np.array_equal(g.view(np.int32)[~np.isnan(g)], ref[k].view(np.int32)[~np.isnan(g)]), (what, k)
    for k in FLOATS64:
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == np.float64 and g.shape == ref[k].shape and np.array_equal(g, ref[k], equal_nan=True), (what, k, g, ref[k])
    for k in INTS:
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == np.int32 and g.shape == ref[k].shape and np.array_equal(g, ref[k]), (what, k, g, ref[k])


def reference(keys, points, frames, counts, norm, **kw):
    return R.plan(keys, points, frames, counts, scale=NORM[0] if norm else None, min_=NORM[1] if norm else None, **kw)


# ---- plan against the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_plan_against_the_restatement(name):
    (b, dn, frames, nk), per_dancer, norm = CASES[name]
    keys, points, counts = R.case(b, dn, frames, nk, seed=frames + nk, per_dancer=per_dancer)
    key0 = keys[0, 0] if per_dancer else keys
    assert key0[0] == 0 and (nk == 1 or counts[0, 0] == nk - 1 and np.isnan(points[0, 0, nk - 1]).all())   # keys at frame 0; NaN in the padding
    assert nk == 1 or (keys[..., -1] == frames - 1).all()                                                  # and at the last frame
    ref = reference(keys, points, frames, counts, norm, min_distance=1.0, max_speed=2.0)
    assert not ref["status"].any() and np.isfinite(ref["traj"]).all()                                     # the NaN of the padding was not read
    got = CH.plan(dev(keys), dev(points), frames, counts=dev(counts), normalizer=Norm(151, (4, 5)) if norm else None, min_distance=1.0, max_speed=2.0)
    assert got.columns == ((4, 5) if norm else None) and tuple(got.dist_min.shape) == (b, len(pairs(dn))) and tuple(got.x_0.shape) == (b, frames * dn, 3)
    check_plan(got, ref, name)
    print(f"[choreo] {name}: every output equal to the restatement's; clamped {ref['clamped'].tolist()}, too_fast {ref['too_fast'].tolist()}, "
          f"too_close {ref['too_close'].tolist()}, speed_max {np.round(ref['speed_max'], 2).tolist()} m/s")
    again = CH.plan(keys, points, frames, counts=counts, normalizer=Norm(3, (0, 1)) if norm else None, min_distance=1.0, max_speed=2.0)      # numpy: copied up
    assert again.columns == ((0, 1) if norm else None)
    check_plan(again, ref, name + ", from numpy, the 3-column normaliser")                                 # and the same input gives the same bits
    if norm:
        first = again.x_0.view(b, frames, dn, 3).permute(0, 2, 1, 3)[..., :2]                              # the layout of rollout's first window
        assert np.array_equal(first.cpu().numpy().view(np.int32), np.moveaxis(ref["x_0"].reshape(b, frames, dn, 3), 1, 2)[..., :2].view(np.int32))


def test_a_bad_dancer_is_nan_and_leaves_the_others_alone():
    b, dn, frames, nk = 1, 5, 70, 4
    keys, points, counts = R.case(b, dn, frames, nk, seed=21, per_dancer=True, short=False)
    clean = CH.plan(keys, points, frames, normalizer=Norm(151, (4, 5)))
    keys[0, 1, 2] = keys[0, 1, 1]                              # a repeated key
    keys[0, 2, 3] = frames                                     # a key equal to frames
    points[0, 3, 1, 0] = np.inf                                # an infinite point
    got = CH.plan(keys, points, frames, normalizer=Norm(151, (4, 5)))
    assert got.status.tolist() == [[0, 1, 1, 2, 0]]
    check_plan(got, reference(keys, points, frames, None, True), "statuses")
    x0 = lambda p: p.x_0.view(b, frames, dn, 3)
    assert bool(torch.isnan(got.traj[0, 1:4]).all()) and bool(torch.isnan(x0(got)[:, :, 1:4, :2]).all()) and not x0(got)[..., 2].any()
    for d in (0, 4):                                           # the good dancers' bits are what they are without the bad ones
        assert torch.equal(got.traj[0, d].view(torch.int32), clean.traj[0, d].view(torch.int32))
        assert torch.equal(x0(got)[:, :, d].view(torch.int32), x0(clean)[:, :, d].view(torch.int32))
        for k in ("clamped", "speed_max", "speed_peak", "too_fast", "path_length"):
            assert torch.equal(getattr(got, k)[0, d], getattr(clean, k)[0, d]), k
    order = pairs(dn)
    for p, (i, j) in enumerate(order):                         # the pair reports leave the NaN frames out: no frame is left
        if {i, j} & {1, 2, 3}:
            assert bool(torch.isnan(got.dist_min[0, p])) and int(got.dist_min_frame[0, p]) == -1 and int(got.too_close[0, p]) == 0
    p04 = order.index((0, 4))
    assert torch.equal(got.dist_min[0, p04], clean.dist_min[0, p04]) and torch.equal(got.dist_min_frame[0, p04], clean.dist_min_frame[0, p04])
    counts[0, 0] = 0                                           # a count outside 1 .. K
    assert CH.plan(keys, points, frames, counts=counts).status.tolist() == [[1, 1, 1, 2, 0]]


def test_the_clamp_holds_x0_at_one_and_counts_the_frames():
    data = torch.zeros(2, 151)
    data[0, 4:6], data[1, 4:6] = -1.0, 1.0                     # fitted on a narrow range: one metre either side
    nrm = tio.Normalizer(data)
    keys = [0, 10, 20, 30]
    points = np.float32([[[[0, 0], [2.5, 0], [2.5, -3], [0.5, 0.5]]]])          # the second and third waypoints lie outside it
    got = CH.plan(keys, points, 31, normalizer=nrm)
    scale, mn = nrm.scaler.scale_[[4, 5]].tolist(), nrm.scaler.min_[[4, 5]].tolist()
    ref = R.plan(keys, points, 31, scale=scale, min_=mn)
    check_plan(got, ref, "clamp")
    x0, traj = got.x_0.view(31, 3).cpu().numpy(), got.traj[0, 0].cpu().numpy()
    outside = (np.abs(ref["traj64"][0, 0]) > 1.0)
    assert np.array_equal(np.abs(x0[:, :2]) == 1.0, outside | (np.abs(ref["traj64"][0, 0]) == 1.0)) and np.abs(x0).max() == 1.0
    assert int(got.clamped[0, 0]) == int(outside.any(1).sum()) > 10
    assert traj[10, 0] == 2.5 and traj[20, 1] == -3.0                                                      # traj, in metres, is not clamped


def test_ties_go_to_the_lower_frame():
    # dancer 0 moves 1 m in 4 frames, holds, and moves 1 m again, dancer 1 the same one metre to the side.  The two moves mirror each
    # other and every value is a dyadic rational that float32 holds exactly, so the first step of the first move and the last step of
    # the second are equal; and every frame ties in distance
    keys = [0, 4, 8, 12]
    points = np.float32([[[[0, 0], [1, 0], [1, 0], [2, 0]], [[0, 1], [1, 1], [1, 1], [2, 1]]]])
    got = CH.plan(keys, points, 13, min_distance=1.5, max_speed=1.0)
    ref = R.plan(keys, points, 13, min_distance=1.5, max_speed=1.0)
    check_plan(got, ref, "ties")
    steps = R.dist(ref["traj"][0, 0, :-1], ref["traj"][0, 0, 1:])
    peak = int(got.speed_peak[0, 0])
    assert (steps == steps.max()).sum() >= 2 and peak == int(np.flatnonzero(steps == steps.max())[0])      # two frames share the largest speed
    assert float(got.dist_min[0, 0]) == 1.0 and int(got.dist_min_frame[0, 0]) == 0 and int(got.too_close[0, 0]) == 13
    far = CH.plan([0, 4, 8, 12], np.float32([[[[0, 0], [1, 0], [1, 0], [2, 0]], [[0, 2], [1, 1], [1, 3], [2, 1]]]]), 13)
    assert float(far.dist_min[0, 0]) == 1.0 and int(far.dist_min_frame[0, 0]) == 4                         # frames 4 and 12 tie: the lower


# ---- trajectory_error ----------------------------------------------------------------------------------------------------------------------------
def check_error(got, joints, traj, up, what):
    ref = R.trajectory_error(joints, traj, up)
    assert list(got) == ["traj_err_mean", "traj_err_max", "traj_err_final", "traj_err_peak", "traj_frames"]
    for k, v in got.items():
        g = v.cpu().numpy()
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape and np.array_equal(g, ref[k], equal_nan=True), (what, k, g, ref[k])
    return ref


@pytest.mark.parametrize("T", [1, 130])
def test_trajectory_error_of_a_known_offset(T):
    b, dn = 2, 3
    g = np.random.default_rng(T)
    traj = g.uniform(-2, 2, (b, dn, T, 2)).astype(np.float32)
    frame_major = np.zeros((b, T, dn, 24, 3), np.float32)      # as the export's launch writes it
    frame_major[..., 0, 0] = np.moveaxis(traj[..., 0], 1, 2) + np.float32(0.03)
    frame_major[..., 0, 1] = np.moveaxis(traj[..., 1], 1, 2) - np.float32(0.04)
    frame_major[..., 0, 2] = 0.9
    frame_major[..., 1:, :] = g.normal(size=(b, T, dn, 23, 3))                                             # the other joints do not count
    if T > 1:
        frame_major[1, 77, 2, 0, 1] = np.nan                   # a frame that is counted out
        frame_major[0, T - 1, 1, 0, 0] = np.inf                # and a last frame: the final error is that of the frame before it
        frame_major[0, 5, 0, 0, 2] = np.nan                    # the up component is not read
    view = dev(frame_major).permute(0, 2, 1, 3, 4)
    assert (T == 1 or not view.is_contiguous()) and tuple(view.shape) == (b, dn, T, 24, 3)
    got = CH.trajectory_error(view, dev(traj))
    joints = np.moveaxis(frame_major, 1, 2)
    ref = check_error(got, joints, traj, 2, f"T = {T}")
    err = got["traj_err_mean"].cpu().numpy()
    print(f"[choreo] trajectory_error T = {T}: mean {err.min():.9f} .. {err.max():.9f} m for an offset of 3 and 4 cm")
    # the closed form: 5 cm, up to the float32 rounding of traj + 0.03 at a magnitude below 4 (2^-22 a component)
    for k in ("traj_err_mean", "traj_err_max", "traj_err_final"):
        assert np.abs(got[k].cpu().numpy() - 0.05).max() <= 2 * 2.0 ** -22, k
    want = np.full((b, dn), T, np.int32)
    if T > 1:
        want[1, 2] -= 1
        want[0, 1] -= 1
    assert np.array_equal(ref["traj_frames"], want)
    s = summarize(got)
    assert set(s) == set(got) and abs(s["traj_err_mean"] - 0.05) < 1e-6
    if T > 1:                                                  # another up axis: the floor is x and z
        other = CH.trajectory_error(view, dev(traj), up=1)
        check_error(other, joints, traj, 1, "up = 1")
        lost = CH.trajectory_error(dev(np.full((1, 1, 3, 24, 3), np.nan, np.float32)), dev(np.zeros((1, 1, 3, 2), np.float32)))
        assert int(lost["traj_frames"]) == 0 and int(lost["traj_err_peak"]) == -1 and bool(torch.isnan(lost["traj_err_mean"]))


# ---- the round trip: plan -> x_0 -> samples -> export_poses -> trajectory_error ------------------------------------------------------------
def test_the_plan_comes_back_through_the_exporter():
    b, dn, S, nk = 2, 3, 150, 6
    g = torch.Generator().manual_seed(7)
    nrm = tio.Normalizer(torch.randn(500, 151, generator=g) * 2.0)                                         # columns 4, 5 reach about 6 m either side
    keys, points, _ = R.case(b, dn, S, nk, seed=33, short=False)                                           # waypoints within 3 m: nothing is clamped
    p = CH.plan(keys, points, S, normalizer=nrm)
    assert not p.status.any() and not p.clamped.any() and p.columns == (4, 5)
    samples = torch.zeros(b, S * dn, 151, device=DEV)
    samples[..., 4:6] = p.x_0[..., :2]
    _, pos, poses, _ = export_poses(samples, nrm, "normal", dn)
    got = CH.trajectory_error(poses, p.traj)
    check_error(got, poses.cpu().numpy(), p.traj.cpu().numpy(), 2, "round trip")
    # The bound, per channel, with u = 2^-24, s = scale_, m = min_, v the float64 path value and |v| <= V = the largest waypoint
    # (PCHIP does not overshoot):
    #   the plan stores x = fl(v s + m), |v s + m| <= 1:                    |x - (v s + m)| <= u
    #   the exporter forms a = fl(x - m) and r = fl(a / s):                 r = ((x - m) / s) (1 + e1)(1 + e2), |e| <= u
    #   so |r - v| <= u / s + (V + u / s)(2 u + u^2), and traj = fl(v):     |traj - v| <= u V
    # trajectory_error's own float64 operations add 1e-15.  The two channels combine as sqrt(Ex^2 + Ey^2).
    u, V = 2.0 ** -24, float(np.abs(points).max())
    E = [u / s + (V + u / s) * (2 * u + u * u) + u * V for s in nrm.scaler.scale_[[4, 5]].tolist()]
    bound = float(np.hypot(*E)) + 1e-15
    worst = float(got["traj_err_max"].max())
    print(f"[choreo] round trip through export_poses: traj_err_max {worst:.3e} m, mean {float(got['traj_err_mean'].mean()):.3e} m "
          f"(bound {bound:.3e} m from the float32 roundings of the chain)")
    assert worst <= bound and int(got["traj_frames"].min()) == S
    assert torch.equal(poses[:, :, :, 0], pos.view(b, S, dn, 3).permute(0, 2, 1, 3))                       # the root is joint 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    keys, points, counts = R.case(1, 2, 20, 3, seed=2)
    with pytest.raises(L.TcdiffError, match="runs on MI355X only"):
        CH.plan(dev(keys), torch.from_numpy(points), 20)                                                   # a host tensor
    with pytest.raises(L.TcdiffError, match="runs on MI355X only"):
        CH.plan(torch.from_numpy(keys), dev(points), 20)
    buf = torch.zeros(1, 40, 3, device=DEV)
    inside = buf.view(-1)[:12].view(1, 2, 3, 2)                                                            # points that live inside out
    with pytest.raises(L.TcdiffError, match="out overlaps the points"):
        CH.plan(keys, inside, 20, out=buf)
    out = torch.empty(1, 40, 3, device=DEV)
    p = CH.plan(keys, dev(points), 20, counts=counts, out=out)
    assert p.x_0 is out and bool(torch.isfinite(out).all())
    with pytest.raises(L.TcdiffError, match="trajectory_error runs on MI355X only"):
        CH.trajectory_error(torch.zeros(1, 2, 20, 24, 3), p.traj)
    # misaligned float64 outputs, at the launcher: a float64 report 4 bytes off
    f64 = lambda: torch.empty(1, 2, dtype=torch.float64, device=DEV)
    i32 = lambda: torch.empty(1, 2, dtype=torch.int32, device=DEV)
    off = lambda: torch.empty(5, dtype=torch.float32, device=DEV)[1:]
    assert off().data_ptr() % 8 == 4
    args = lambda **kw: [kw.get(k, make()) for k, make in (("status", i32), ("clamped", i32), ("speed_max", f64), ("speed_peak", i32), ("too_fast", i32),
                                                           ("path_length", f64), ("dist_min", f64), ("dist_min_frame", i32), ("too_close", i32))]
    traj, x0 = torch.empty(1, 2, 20, 2, device=DEV), torch.empty(1, 40, 3, device=DEV)
    for name in ("speed_max", "path_length", "dist_min"):
        with pytest.raises(L.TcdiffError, match="tcc_plan: misaligned"):
            K.choreo_plan(dev(points), dev(keys), None, 20, 30.0, None, None, 0.5, 3.0, traj, x0, *args(**{name: off()}))
    J = torch.zeros(1, 2, 20, 24, 3, device=DEV)
    for k in range(3):
        outs = [off() if i == k else f64() for i in range(3)] + [i32(), i32()]
        with pytest.raises(L.TcdiffError, match="tcc_trajectory_error: misaligned"):
            K.trajectory_error(J, traj, 2, *outs)
