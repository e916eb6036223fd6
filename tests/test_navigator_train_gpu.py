"""Training the Dance-Beat Navigator on the MI355X: TrajTrainer's output and gradients (csrc/navigator.hip train-mode forward,
csrc/navigator_train.hip backward) against the float64 restatement of tests/navigator_train_ref.py under the same masks.

Metric: max|got - f64| / max|f64| per group (lstm, music_projection, cond_emb, every block, Decoder, the whole flat gradient) and for
the output.  Bound: 8 x the same metric of the restatement run in float32 on the CPU against its own float64 run -- same case,
masks and groups, computed here; 8 x is the margin tests/test_navigator_gpu.py grants for another fp32 summation order.

The two music row ranges: where rows [0, seq) and [pairs - seq, pairs) overlap (cases A, B, C) their contributions must ADD; a
missing add shows as an error of order one in the `music_projection` group, which is the check that catches it.  Case D (no overlap)
additionally reads the trainer's workspace of music_projection's output gradient -- an internal, read on purpose because nothing
public shows it -- to see that the rows between the ranges stay exactly zero."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navigator_ref as R  # noqa: E402
import navigator_train_ref as TR  # noqa: E402
from tcdiff_amd import TrajDecoder, TrajTrainer  # noqa: E402
from tcdiff_amd._lib import TcdiffError  # noqa: E402

DEV = "cuda"
FACTOR = 8.0
SEED = (1234567, 7654321)
torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


def setup(case):
    name, layers, window, dn, b, frames, p = case
    net = TrajDecoder(nfeats=2, trans_layer=layers, window_size=window)
    sd = R.synth_state_dict(net)
    net.load_state_dict(sd, strict=True)
    x, cond = R.synth_inputs("train." + name, window, dn, b, frames)
    target = TR.synth_target(name, b, dn, window)
    return net.to(DEV).eval(), sd, x, cond, target


def grads_of(net):
    return {k: p.grad for k, p in net.named_parameters()}


_ref = {}


def reference(case):
    """(float64 loss / output / grads, fp32-CPU loss / output / grads) of the restatement under SEED's masks, once per case"""
    name, layers, window, dn, b, frames, p = case
    if name not in _ref:
        net = TrajDecoder(nfeats=2, trans_layer=layers, window_size=window)
        sd = R.synth_state_dict(net)
        x, cond = R.synth_inputs("train." + name, window, dn, b, frames)
        target = TR.synth_target(name, b, dn, window)
        keep = TR.masks(SEED, p, layers, b, dn * window)
        r64 = TR.loss_and_grads(R.to(sd, torch.float64), x.double(), cond.double(), target.double(), layers, keep, p)
        r32 = TR.loss_and_grads(R.to(sd, torch.float32), x, cond, target, layers, keep, p)
        _ref[name] = (r64, r32)
    return _ref[name]


@pytest.mark.parametrize("case", TR.CASES, ids=[c[0] for c in TR.CASES])
def test_output_and_gradients_against_float64_within_eight_fp32_cpu_errors(case):
    name, layers, window, dn, b, frames, p = case
    net, sd, x, cond, target = setup(case)
    (l64, o64, g64), (l32, o32, g32) = reference(case)
    trainer = TrajTrainer(net, dropout=p)
    out = trainer(x.to(DEV), cond.to(DEV), seed=SEED)
    assert out.shape == (b, dn, window, 2) and out.grad_fn is not None
    loss = TR.loss_fn(out, target.to(DEV))
    loss.backward()
    got = grads_of(net)
    assert got["trans_extractor.traj_emb.weight"] is None and got["trans_extractor.traj_emb.bias"] is None
    fails = []
    e, bound = R.rel_err(out, o64), FACTOR * R.rel_err(o32, o64)
    print(f"{name} output          : {e:.3e}   bound {bound:.3e}")
    if not e <= bound:
        fails.append(("output", e, bound))
    errs, yard = TR.group_errors(got, g64), TR.group_errors(g32, g64)
    for grp in sorted(errs):
        bound = FACTOR * yard[grp]
        print(f"{name} {grp:16s}: {errs[grp]:.3e}   bound {bound:.3e}   (fp32 CPU: {yard[grp]:.3e})")
        if not errs[grp] <= bound:
            fails.append((grp, errs[grp], bound))
    for l in range(3):                                           # both LSTM biases receive the gate gradient's row sum
        assert torch.equal(got[f"lstm.bias_ih_l{l}"], got[f"lstm.bias_hh_l{l}"])
    if b == 1:                                                   # h0 = 0 and one time step
        for l in range(3):
            assert float(got[f"lstm.weight_hh_l{l}"].abs().max()) == 0.0
    pairs = frames // 2
    # gradient of music_projection's output rows (b, pairs, 64): both row ranges receive one, the rows between them none
    g_mp = next(iter(trainer._plans.values()))["g_mp"].view(b, pairs, 64)
    assert bool((g_mp[:, :window].abs().amax(dim=2) > 0).all())
    assert bool((g_mp[:, pairs - window:].abs().amax(dim=2) > 0).all())
    if pairs > 2 * window:                                       # rows between the two ranges get no gradient
        assert float(g_mp[:, window:pairs - window].abs().max()) == 0.0
    assert not fails, fails


def test_same_seed_same_bits_other_seed_other_bits_and_p0_is_the_eval_forward():
    case = TR.CASES[0]
    name, layers, window, dn, b, frames, p = case
    net, sd, x, cond, target = setup(case)
    x, cond, target = x.to(DEV), cond.to(DEV), target.to(DEV)
    trainer = TrajTrainer(net, dropout=p)

    def run(seed):
        net.zero_grad(set_to_none=True)
        out = trainer(x, cond, seed=seed)
        TR.loss_fn(out, target).backward()
        return out.detach().clone(), {k: g.clone() for k, g in grads_of(net).items() if g is not None}
    o1, g1 = run(SEED)
    o2, g2 = run(SEED)
    o3, g3 = run((SEED[0] + 1, SEED[1]))
    assert torch.equal(o1, o2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    assert not torch.equal(o1, o3) and not torch.equal(g1["Decoder.0.weight"], g3["Decoder.0.weight"])
    torch.manual_seed(5)
    a = trainer(x, cond)                                         # seed=None: two words from torch's generator
    torch.manual_seed(5)
    assert torch.equal(a, trainer(x, cond))
    assert not torch.equal(a, trainer(x, cond))
    plain = TrajTrainer(net, dropout=0.0)(x, cond, seed=SEED)
    assert torch.equal(plain.detach(), net(x, cond))


def test_grad_accumulates_like_torch():
    case = TR.CASES[0]
    name, layers, window, dn, b, frames, p = case
    net, sd, x, cond, target = setup(case)
    x, cond, target = x.to(DEV), cond.to(DEV), target.to(DEV)
    trainer = TrajTrainer(net, dropout=p)
    TR.loss_fn(trainer(x, cond, seed=SEED), target).backward()
    first = {k: g.clone() for k, g in grads_of(net).items() if g is not None}
    TR.loss_fn(trainer(x, cond, seed=SEED), target).backward()  # no zero_grad
    for k, g in first.items():
        now = dict(net.named_parameters())[k].grad
        assert torch.allclose(now, 2 * g, rtol=1e-6, atol=0), k
    with pytest.raises(TcdiffError, match="train_traj"):
        trainer(x.clone().requires_grad_(), cond)
    out = trainer(x, cond, seed=SEED)
    trainer(x, cond, seed=SEED)                                  # a second forward: the first one's activations are gone
    with pytest.raises(TcdiffError, match="outstanding"):
        TR.loss_fn(out, target).backward()


def test_five_adamw_steps_follow_the_float64_trajectory_and_both_paths_see_new_weights():
    case = TR.CASES[0]
    name, layers, window, dn, b, frames, p = case
    net, sd, x, cond, target = setup(case)
    trainer = TrajTrainer(net, dropout=p)
    opt = torch.optim.AdamW(net.parameters(), lr=2e-3, betas=(0.5, 0.9), weight_decay=1e-6)
    xd, cd, td = x.to(DEV), cond.to(DEV), target.to(DEV)
    keep = TR.masks(SEED, p, layers, b, dn * window)

    def cpu_run(dtype):
        leaf = {k: (v.to(dtype).clone().requires_grad_(True) if TR.is_param(k) else v.to(dtype)) for k, v in sd.items()}
        o = torch.optim.AdamW([v for k, v in leaf.items() if TR.is_param(k)], lr=2e-3, betas=(0.5, 0.9), weight_decay=1e-6)
        losses = []
        for _ in range(5):
            loss = TR.loss_fn(TR.forward(leaf, x.to(dtype), cond.to(dtype), layers, keep, p), target.to(dtype))
            o.zero_grad()
            loss.backward()
            o.step()
            losses.append(float(loss.detach()))
        return losses, leaf
    l64, _ = cpu_run(torch.float64)
    l32, _ = cpu_run(torch.float32)
    got = []
    for i in range(5):
        loss = TR.loss_fn(trainer(xd, cd, seed=SEED), td)
        opt.zero_grad()
        loss.backward()
        opt.step()
        got.append(float(loss.detach()))
        if i == 0:                                               # the in-place step is seen by the trainer and by the module
            now = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
            want_t = TR.forward(now, x.double(), cond.double(), layers, keep, p)
            want_e = TR.forward(now, x.double(), cond.double(), layers)
            old_e = TR.forward(R.to(sd, torch.float64), x.double(), cond.double(), layers)
            moved = R.rel_err(old_e, want_e)
            e_t, e_e = R.rel_err(trainer(xd, cd, seed=SEED), want_t), R.rel_err(net(xd, cd), want_e)
            print(f"after one step: weights moved the output by {moved:.3e}; trainer {e_t:.3e}, module {e_e:.3e}")
            assert moved > 1e-3 and e_t < 1e-5 and e_e < 1e-5
    print("gpu ", got, "\nf64 ", l64, "\nfp32", l32)
    assert got[-1] < got[0]
    for g, w, y in zip(got, l64, l32):
        assert abs(g - w) / abs(w) <= FACTOR * max(abs(y - w) / abs(w), 2.0 ** -24)
