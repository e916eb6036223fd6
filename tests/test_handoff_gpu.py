"""The Navigator -> sampler hand-off on the MI355X: navigator.smooth_x0 / rollout_x0 (csrc/handoff.hip) against
io.kalman_smooth_batch fed float64 and the layout restatement of tests/handoff_ref.py.

Bound (tests/handoff_ref.py, derived, not measured): the kernel runs the yardstick's float64 recursion and rounds once to float32,
so per element |got - want64| <= 2^-24 |want64| (1 + 2^-20) + 1e-12.  Every comparison covers every element.  Un-normalised
outputs are held bit for bit to io.Normalizer.unnormalize applied in float32 to the kernel's own float32 x_0."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handoff_ref as HR  # noqa: E402
import navigator_ref as R  # noqa: E402
from tcdiff_amd import TrajDecoder  # noqa: E402
from tcdiff_amd import io as IO  # noqa: E402
from tcdiff_amd import navigator as N  # noqa: E402
from tcdiff_amd._lib import TcdiffError  # noqa: E402

DEV = "cuda"
OTHER = dict(dt=0.5, process_noise_std=0.1, measurement_noise_std=0.3)


def dev(xy):
    return torch.from_numpy(np.ascontiguousarray(xy)).to(DEV)


def held(got, want64, what):
    ok, worst = HR.within_bound(got.cpu().numpy(), want64)
    print(f"{what}: worst |got - want64| / bound = {worst:.3f}")
    assert tuple(got.shape) == want64.shape and got.dtype == torch.float32
    assert ok, (what, worst)


def reordered(x0, b, dn, frames):
    """channels 0, 1 of x_0 (b, frames * dn, 3) as (b, dn, frames, 2)"""
    return x0[..., :2].reshape(b, frames, dn, 2).permute(0, 2, 1, 3)


@pytest.mark.parametrize("frames", [1, 2, 3, 151])
def test_frames(frames):
    b, dn = 3, 2
    xy = HR.walks(b, dn, frames, seed=10 + frames)
    got = N.smooth_x0(dev(xy))
    held(got, HR.want_x0(xy), f"frames {frames}")
    if frames == 1:
        # The first-frame update has gain ~ 1, but the state starts AT the first sample: the residual is zero and the update
        # returns that sample exactly.  "The update, not the raw sample" therefore cannot be told apart at frames == 1 (a kernel
        # that skipped the update there would pass); frames 2, 3 and 151 do tell, through frame 0's velocity update.
        assert np.array_equal(got.cpu().numpy(), HR.x0_layout(xy))


@pytest.mark.parametrize("b,dn", [(1, 1), (3, 2), (13, 5), (2, 33)])
def test_tails_and_axes(b, dn):
    xy = HR.walks(b, dn, 7, seed=100 + b)
    x0, sm = N.smooth_x0(dev(xy), return_smoothed=True)
    want = HR.want_x0(xy)
    held(x0, want, f"b {b} dn {dn}")
    assert tuple(sm.shape) == (b, dn, 7, 2) and torch.equal(sm, reordered(x0, b, dn, 7))


def test_long_mode():
    """900 frames: where a float32 state would leave the bound"""
    xy = HR.walks(2, 3, 900, seed=3, step=0.02, noise=0.05)
    held(N.smooth_x0(dev(xy)), HR.want_x0(xy), "long")


def test_other_parameters_then_the_default_ones_again():
    xy = HR.walks(3, 2, 40, seed=4)
    x = dev(xy)
    first = N.smooth_x0(x)
    held(first, HR.want_x0(xy), "default")
    other = N.smooth_x0(x, **OTHER)
    held(other, HR.want_x0(xy, **OTHER), "dt 0.5, q 0.1, r 0.3")
    assert not torch.equal(first, other)
    again = N.smooth_x0(x)                                      # a gain table keyed wrongly would return `other`
    held(again, HR.want_x0(xy), "default again")
    assert torch.equal(again, first)


def test_strided_inputs_are_read_in_place():
    g = torch.Generator().manual_seed(5)
    x = (0.3 * torch.randn(3, 2, 20, 151, generator=g)).cumsum(2).to(DEV)
    picked = x[:, :, :, [4, 5]]
    view = x[..., 4:6]
    assert not view.is_contiguous() and view.stride() == (2 * 20 * 151, 20 * 151, 151, 1)
    want = N.smooth_x0(picked.contiguous(), return_smoothed=True)
    held(want[0], HR.want_x0(picked.cpu().numpy()), "contiguous copy")
    permuted = picked.permute(2, 0, 3, 1).contiguous().permute(1, 3, 0, 2)          # storage order (frames, b, 2, dn)
    assert permuted.shape == picked.shape and permuted.stride() == (2 * 2, 1, 3 * 2 * 2, 2)
    for name, t in (("x[:, :, :, [4, 5]]", picked), ("x[..., 4:6]", view), ("permuted", permuted)):
        got = N.smooth_x0(t, return_smoothed=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name


def _normalizer(b, dn, frames, seed):
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(b, dn * frames, 3, generator=g) * torch.tensor([2.0, 0.5, 1.5]) + torch.tensor([0.3, -0.2, 0.7])
    return IO.Normalizer(data)


def test_out_filled_with_nan_is_written_everywhere():
    b, dn, frames = 3, 2, 9
    xy = HR.walks(b, dn, frames, seed=6)
    out = torch.full((b, frames * dn, 3), float("nan"), device=DEV)
    x0, sm = N.smooth_x0(dev(xy), out=out, return_smoothed=True)
    assert x0 is out and bool(torch.isfinite(out).all())
    assert bool((out[..., 2] == 0).all())
    assert torch.equal(sm, reordered(out, b, dn, frames))
    held(out, HR.want_x0(xy), "out=")
    nrm = _normalizer(b, dn, frames, 61)
    out.fill_(float("nan"))
    x0, sm = N.smooth_x0(dev(xy), out=out, return_smoothed=True, normalizer=nrm)
    assert x0 is out and bool(torch.isfinite(out).all())
    z = (torch.zeros((), dtype=torch.float32) - nrm.scaler.min_[2]) / nrm.scaler.scale_[2]
    assert z.dtype == torch.float32 and float(z) != 0.0 and bool((out[..., 2].cpu() == z).all())
    assert torch.equal(sm, reordered(out, b, dn, frames))
    for bad in (torch.zeros(b, frames * dn, 2, device=DEV), torch.zeros(b, dn * frames, 3, device=DEV, dtype=torch.float64),
                torch.zeros(b, frames * dn, 3), torch.zeros(b, frames * dn + 1, 3, device=DEV)):
        with pytest.raises(TcdiffError):
            N.smooth_x0(dev(xy), out=bad)


def test_normalizer_is_unnormalize_of_the_kernels_own_x0():
    b, dn, frames = 3, 2, 31
    xy = 3.0 * HR.walks(b, dn, frames, seed=7)                  # partly outside [-1, 1]: the clamp works
    nrm = _normalizer(b, dn, frames, 71)
    plain = N.smooth_x0(dev(xy))
    a = plain[..., :2].abs()
    assert bool((a > 1).any()) and bool((a < 1).any())
    got, sm = N.smooth_x0(dev(xy), normalizer=nrm, return_smoothed=True)
    want = nrm.unnormalize(plain.cpu())
    assert want.dtype == torch.float32 and torch.equal(got.cpu(), want)
    assert torch.equal(sm, reordered(got, b, dn, frames))
    held(plain, HR.want_x0(xy), "before un-normalising")


def build(layers, window):
    m = TrajDecoder(nfeats=2, trans_layer=layers, window_size=window)
    m.load_state_dict(R.synth_state_dict(m), strict=True)
    return m.to(DEV).eval()


def test_rollout_x0():
    name, layers, window, step, dn, b, cond_len = min((c for c in R.CASES if not c[0].startswith("forward")),
                                                      key=lambda c: c[1] * c[2] * c[4] * c[5] * c[6])
    m = build(layers, window)
    x, cond = R.synth_inputs(name, window, dn, b, cond_len)
    x, cond = x.to(DEV), cond.to(DEV)
    traj = N.rollout(m, x, cond, step=step)
    frames = traj.shape[2]
    assert frames > window
    want = N.smooth_x0(traj, return_smoothed=True)
    got = N.rollout_x0(m, x, cond, step=step, return_smoothed=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    held(got[0], HR.want_x0(traj.cpu().numpy()), f"rollout_x0 ({name})")
    assert torch.equal(N.rollout_x0(m, x, cond, step=step, **OTHER), N.smooth_x0(traj, **OTHER))
    nrm = _normalizer(b, dn, frames, 81)                                           # the keywords reach the hand-off launch
    out = torch.full((b, frames * dn, 3), float("nan"), device=DEV)
    want_n = N.smooth_x0(traj, normalizer=nrm, return_smoothed=True)
    got_n = N.rollout_x0(m, x, cond, step=step, normalizer=nrm, out=out, return_smoothed=True)
    assert got_n[0] is out and torch.equal(out, want_n[0]) and torch.equal(got_n[1], want_n[1])
    assert torch.equal(out.cpu(), nrm.unnormalize(want[0].cpu()))
    with pytest.raises(TcdiffError):
        N.rollout_x0(m, x, cond, step=step, out=torch.zeros(b, frames * dn, 2, device=DEV))
    short = N.rollout_x0(m, x, cond[:, :(window + step) * 2 - 1], step=step)      # too short for one window
    assert torch.equal(short, N.smooth_x0(x[:, :, :window]))
    held(short, HR.want_x0(x[:, :, :window].cpu().numpy()), "the first window alone")


def test_determinism_and_refusals():
    xy = HR.walks(13, 5, 7, seed=8)
    x = dev(xy)
    assert torch.equal(N.smooth_x0(x), N.smooth_x0(x))
    for bad in (x.double(), x.half(), x[..., 0], torch.zeros(3, 2, 7, 3, device=DEV), torch.zeros(0, 2, 7, 2, device=DEV), x.cpu()):
        with pytest.raises(TcdiffError):
            N.smooth_x0(bad)
    with pytest.raises(TcdiffError):
        N.smooth_x0(x, normalizer=IO.Normalizer(torch.randn(4, 5)))
    flat = torch.zeros(13 * 5 * 7 * 3, device=DEV)                           # out= on top of the input
    src = flat[:13 * 5 * 7 * 2].view(13, 5, 7, 2)
    with pytest.raises(TcdiffError, match="overlap"):
        N.smooth_x0(src, out=flat.view(13, 7 * 5, 3))


def test_rollout_x0_feeds_the_sampler():
    """rollout_x0 -> ddim_sample(x_0=) on the configuration of tests/test_navigator_gpu.py's hand-off test: channels 4, 5 of the
    sample are those io.x0_from_navigator gives, to that test's tolerance (e == 0.0)"""
    import torch.nn.functional as F
    from oracle import tcdiff_oracle as O
    from tcdiff_amd import DanceDecoder, GaussianDiffusion
    dn, S, window, step = 2, 60, 40, 10
    m = build(2, window)
    x, cond = R.synth_inputs("e2e", window, dn, 1, 2 * S + 1)
    x, cond = (0.4 * x).to(DEV), cond.to(DEV)
    x0_host = IO.x0_from_navigator(N.rollout(m, x, cond, step=step))
    x0 = N.rollout_x0(m, x, cond, step=step)
    assert x0.shape == (1, S * dn, 3)
    model = DanceDecoder(nfeats=151, seq_len=S, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=F.gelu, required_dancer_num=dn, compute_dtype="f32")
    model.load_state_dict(O.synth_state_dict(dn=dn, seq_len=S))
    diff = GaussianDiffusion(model, S, 151, None, schedule="cosine", n_timestep=1000, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=S).to(DEV).eval()
    sample = diff.ddim_sample((1, S * dn, 151), cond, x_0=x0)
    assert bool(torch.isfinite(sample).all())
    e = float((sample[..., 4:6].cpu() - x0_host[..., :2].cpu()).abs().max())
    print(f"sample channels 4, 5 vs io.x0_from_navigator: {e:.3e}")
    assert e == 0.0
