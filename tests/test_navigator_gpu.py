"""Dance-Beat Navigator on the MI355X: the HIP kernels (tcdiff_amd/navigator.py, csrc/navigator.hip) against the float64
restatement of tests/navigator_ref.py on every golden case -- per stage for the first window and on the predicted frames of the
rollout (the copied first window is exact by construction and excluded).

Metric: max|got - f64| / max|f64|.  Bound: 8 x the same metric of the reference's own fp32 CPU run against its float64 run, per
case and stage, read from tests/golden/navigator.npz; a stage's yardstick is floored at 2^-24 (half an fp32 ulp of the stage's top
magnitude).  8 x: the yardstick is one draw of fp32 rounding in one summation order; the kernels sum in another order through
about 40 chained products, and the device's erf / exp / tanh are a few ulp against libm's one."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navigator_ref as R  # noqa: E402
from tcdiff_amd import TrajDecoder  # noqa: E402
from tcdiff_amd import navigator as N  # noqa: E402
from tcdiff_amd._lib import TcdiffError  # noqa: E402

DEV = "cuda"
FACTOR, FLOOR = 8.0, 2.0 ** -24
torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "navigator.npz"))


def build(layers, window):
    m = TrajDecoder(nfeats=2, trans_layer=layers, window_size=window)
    sd = R.synth_state_dict(m)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval(), sd


def case(name):
    return next(c for c in R.CASES if c[0] == name)


@pytest.mark.parametrize("c", R.CASES, ids=[c[0] for c in R.CASES])
def test_kernels_against_float64_within_eight_reference_fp32_errors(gold, c):
    name, layers, window, step, dn, b, cond_len = c
    m, sd = build(layers, window)
    sd64 = R.to(sd, torch.float64)
    x, cond = R.synth_inputs(name, window, dn, b, cond_len)
    taps, taps64 = {}, {}
    if name.startswith("forward"):
        got = m(x.to(DEV), cond.to(DEV), taps=taps)
        want = R.forward(sd64, x.double(), cond.double(), layers, taps=taps64)
        pred_got, pred_want = got, want
    else:
        got = N.rollout(m, x.to(DEV), cond.to(DEV), step=step, taps=taps)
        want = R.rollout(sd64, x.double(), cond.double(), layers, window, step, taps=taps64)
        assert torch.equal(got[:, :, :window].cpu(), x[:, :, :window])             # the copied first window
        pred_got, pred_want = got[:, :, window:], want[:, :, window:]
    assert tuple(got.shape) == tuple(want.shape) == gold[f"{name}.out64"].shape
    pairs = window + step if not name.startswith("forward") else cond_len // 2
    rows = {"lstm": (taps["lstm"], taps64["lstm"]), "music": (taps["music"][:, :pairs], taps64["music"]),
            "blocks": (taps["blocks"], taps64["blocks"])}
    fails = []
    for st, (g, w) in rows.items():
        e, bound = R.rel_err(g, w), FACTOR * max(float(gold[f"{name}.{st}.yardstick"]), FLOOR)
        print(f"{name} {st:7s}: {e:.3e}   bound {bound:.3e}   (reference fp32: {float(gold[f'{name}.{st}.yardstick']):.3e})")
        if not e <= bound:
            fails.append((st, e, bound))
    for i in range(layers):
        print(f"{name} block {i}: {R.rel_err(taps['blocks'][i], taps64['blocks'][i]):.3e}")
    e, bound = R.rel_err(pred_got, pred_want), FACTOR * max(float(gold[f"{name}.out_yardstick"]), FLOOR)
    print(f"{name} output : {e:.3e}   bound {bound:.3e}   (reference fp32: {float(gold[f'{name}.out_yardstick']):.3e})")
    if not e <= bound:
        fails.append(("output", e, bound))
    assert not fails, fails


def test_lstm_runs_over_the_clip_axis():
    """clip 1 alone and clip 1 inside a batch differ (the reference's nn.LSTM without batch_first), and both match float64"""
    name, layers, window, step, dn, b, cond_len = case("even")
    m, sd = build(layers, window)
    x, cond = R.synth_inputs(name, window, dn, b, cond_len)
    music = cond[:, :(window + step) * 2]
    both = m(x.to(DEV), music.to(DEV)).cpu()
    alone = m(x[1:2].to(DEV), music[1:2].to(DEV)).cpu()
    d = float((both[1] - alone[0]).abs().max())
    print(f"clip 1 in a batch vs alone: {d:.3e}")
    assert d > 1e-5
    sd64 = R.to(sd, torch.float64)
    assert R.rel_err(alone, R.forward(sd64, x[1:2].double(), music[1:2].double(), layers)) < 1e-5
    assert R.rel_err(both, R.forward(sd64, x.double(), music.double(), layers)) < 1e-5
    assert torch.equal(both[0], m(x[:1].to(DEV), music[:1].to(DEV)).cpu()[0])      # clip 0 depends on nothing before it


def test_unused_mask_and_traj_emb_do_not_matter_and_weight_changes_are_seen():
    name, layers, window, step, dn, b, cond_len = case("odd")
    m, _ = build(layers, window)
    x, cond = R.synth_inputs(name, window, dn, b, cond_len)
    x, cond = x.to(DEV), cond.to(DEV)
    base = N.rollout(m, x, cond, step=step)
    again = N.rollout(m, x, cond, step=step)
    assert torch.equal(base, again)                                                # two rollouts in a row: bit-identical
    with torch.no_grad():
        for blk in m.trans_extractor.blocks:
            blk.attn.mask.zero_()
        m.trans_extractor.traj_emb.weight.normal_()
        m.trans_extractor.traj_emb.bias.normal_()
    assert torch.equal(base, N.rollout(m, x, cond, step=step))
    with torch.no_grad():
        m.Decoder[6].bias.add_(0.25)                                               # in place: the packed weights must follow
    moved = N.rollout(m, x, cond, step=step)
    assert torch.equal(moved[:, :, :window], base[:, :, :window])
    first = (moved[:, :, window:window + step] - base[:, :, window:window + step] - 0.25).abs().max()
    assert float(first) < 1e-6
    assert not torch.equal(moved[:, :, window + step:], base[:, :, window + step:])


@pytest.mark.parametrize("name", ["even", "odd"])
def test_rollout_equals_a_loop_over_forward_bit_for_bit(name):
    """the hoisted music front (all pairs of the song once) against per-window recomputation; odd and even cond lengths"""
    name, layers, window, step, dn, b, cond_len = case(name)
    m, _ = build(layers, window)
    x, cond = R.synth_inputs(name, window, dn, b, cond_len)
    x, cond = x.to(DEV), cond.to(DEV)
    got = N.rollout(m, x, cond, step=step)
    loop = R.rollout(None, x, cond, layers, window, step, per_window=lambda cur, music: m(cur, music))
    assert got.shape == loop.shape and torch.equal(got, loop)
    short = N.rollout(m, x, cond[:, :(window + step) * 2 - 1], step=step)         # too short for one window
    assert torch.equal(short, x[:, :, :window])


def test_shapes_the_reference_refuses():
    m, _ = build(2, 20)
    with pytest.raises(TcdiffError, match="max_len"):
        m(torch.zeros(1, 26, 20, 2, device=DEV), torch.zeros(1, 50, 438, device=DEV))
    with pytest.raises(TcdiffError):
        m(torch.zeros(1, 2, 20, 2, device=DEV), torch.zeros(1, 30, 438, device=DEV))          # 15 pairs < seq
    with pytest.raises(TcdiffError, match="train_traj"):
        m(torch.zeros(1, 2, 20, 2, device=DEV, requires_grad=True), torch.zeros(1, 50, 438, device=DEV))
    out = m(torch.zeros(1, 25, 20, 2, device=DEV), torch.zeros(1, 50, 438, device=DEV))      # exactly 500 positions run
    assert out.shape == (1, 25, 20, 2) and bool(torch.isfinite(out).all())


def test_rollout_feeds_the_sampler():
    """rollout -> io.x0_from_navigator -> ddim_sample(x_0=): the sample's channels 4, 5 are the smoothed trajectory"""
    import torch.nn.functional as F
    from oracle import tcdiff_oracle as O
    from tcdiff_amd import DanceDecoder, GaussianDiffusion, io
    dn, S, window, step = 2, 60, 40, 10
    m, _ = build(2, window)
    x, cond = R.synth_inputs("e2e", window, dn, 1, 2 * S + 1)
    traj = N.rollout(m, (0.4 * x).to(DEV), cond.to(DEV), step=step)                      # stays inside the sampler's [-1, 1]
    assert traj.shape == (1, dn, S, 2)
    x0 = io.x0_from_navigator(traj)
    assert x0.shape == (1, S * dn, 3)
    model = DanceDecoder(nfeats=151, seq_len=S, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=F.gelu, required_dancer_num=dn, compute_dtype="f32")
    model.load_state_dict(O.synth_state_dict(dn=dn, seq_len=S))
    diff = GaussianDiffusion(model, S, 151, None, schedule="cosine", n_timestep=1000, predict_epsilon=False, loss_type="l2",
                             guidance_weight=2, cond_drop_prob=0.25, seq_len=S).to(DEV).eval()
    sample = diff.ddim_sample((1, S * dn, 151), cond.to(DEV), x_0=x0)
    assert bool(torch.isfinite(sample).all())
    e = float((sample[..., 4:6].cpu() - x0[..., :2].cpu()).abs().max())
    print(f"sample channels 4, 5 vs smoothed trajectory: {e:.3e}")
    assert e == 0.0
