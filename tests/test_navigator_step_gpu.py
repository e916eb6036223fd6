"""The Navigator's loss head and optimizer on the MI355X (csrc/navigator_step.hip; navigator.traj_loss, navigator.TrajAdamW).

Yardstick (tests/navigator_step_ref.py): every figure is compared with a float64 evaluation and may differ from it by 8 x what
the reference's own float32 CPU evaluation differs from it, with a floor of 8 * 2^-24 relative; every figure is printed with its
bound.  Metrics: the four loss scalars |got - f64| / |f64|; gradients and optimizer state max|got - f64| / max|f64|; parameters
max|p - p64| / max|p64 - p_start| per group, the error of the UPDATE.

Observed on one MI355X (kernel / fp32 CPU; profiles/navigator_train.txt): loss scalars 1.9e-9 .. 8.8e-8 / 1.9e-9 .. 1.5e-7, d pre_traj
6.5e-8 .. 8.4e-8 / 6.5e-8 .. 9.4e-8; synthetic gradients: update 2.9e-6 .. 1.3e-4 / the same, exp_avg 5.1e-8 .. 8.1e-7 / the same,
exp_avg_sq 1.1e-7 .. 3.9e-7 / 8.3e-8 .. 3.8e-7; whole steps: loss 9.4e-9 .. 1.2e-7 / 1.7e-10 .. 1.6e-7, parameters after the fifth
1.7e-4 .. 1.3e-2 / 1.0e-4 .. 1.5e-2 (Adam's first steps are sign-like: an element whose gradient is rounding noise moves by +-lr in
either run, which is why the fp32 CPU run itself is that far from float64)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navigator_ref as R  # noqa: E402
import navigator_step_ref as SR  # noqa: E402
import navigator_train_ref as TR  # noqa: E402
from tcdiff_amd import TrajAdamW, TrajDecoder, TrajTrainer, traj_loss  # noqa: E402
from tcdiff_amd._lib import TcdiffError  # noqa: E402

DEV = "cuda"
SEED = (1234567, 7654321)
torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))

_loss_ref = {}


def loss_reference(shape):
    """(inputs, float64 scalars and gradient, float32-CPU scalars and gradient), once per shape"""
    if shape not in _loss_ref:
        pre, tgt = SR.loss_inputs(*shape)
        _loss_ref[shape] = (pre, tgt, SR.loss_and_grad(pre, tgt, torch.float64), SR.loss_and_grad(pre, tgt, torch.float32))
    return _loss_ref[shape]


def gpu_loss(pre, tgt, scale=None):
    """traj_loss on device copies: (the four scalars, the gradient of (scale *) total)"""
    p = pre.to(DEV).requires_grad_(True)
    total, parts = traj_loss(p, tgt.to(DEV))
    assert total.dim() == 0 and total.grad_fn is not None and type(total.grad_fn).__name__ == "_TrajLossFnBackward"
    assert all(t.dim() == 0 and not t.requires_grad for t in parts)
    (total if scale is None else scale * total).backward()
    return torch.stack([total.detach(), *parts]), p.grad


def check_loss(label, vals, grad, shape, fails, scale=1.0):
    _, _, (v64, g64), (v32, g32) = loss_reference(shape)
    for name, e, y in zip(("total", "recon", "dis", "v"), SR.scalar_errs(vals, v64), SR.scalar_errs(v32, v64)):
        print(f"{label} {name:6s}: {e:.3e}   bound {SR.bound(y):.3e}   (fp32 CPU: {y:.3e})")
        if not e <= SR.bound(y):
            fails.append((label, name, e, SR.bound(y)))
    e, y = R.rel_err(grad, scale * g64), R.rel_err(g32, g64)
    print(f"{label} d_pre : {e:.3e}   bound {SR.bound(y):.3e}   (fp32 CPU: {y:.3e})")
    if not e <= SR.bound(y):
        fails.append((label, "d_pre", e, SR.bound(y)))


@pytest.mark.parametrize("shape", SR.LOSS_CASES, ids=[f"b{b}_dn{dn}_seq{s}" for b, dn, s in SR.LOSS_CASES])
def test_loss_values_and_gradient_against_float64(shape):
    pre, tgt, _, _ = loss_reference(shape)
    vals, grad = gpu_loss(pre, tgt)
    fails = []
    check_loss(str(shape), vals, grad, shape, fails)
    assert not fails, fails


def test_loss_reads_non_contiguous_views_in_place():
    shape = SR.LOSS_CASES[1]
    b, dn, seq = shape
    pre, tgt, _, _ = loss_reference(shape)
    want_vals, want_grad = gpu_loss(pre, tgt)
    big_t = torch.full((b, dn + 1, seq + 7, 3), 9.0)
    big_t[:, 1:, 4:4 + seq, 1:] = tgt
    big_p = torch.full((b, dn, seq + 5, 2), -7.0)
    big_p[:, :, 2:2 + seq] = pre
    leaf = big_p.to(DEV).requires_grad_(True)
    p_view, t_view = leaf[:, :, 2:2 + seq], big_t.to(DEV)[:, 1:, 4:4 + seq, 1:]
    assert not p_view.is_contiguous() and not t_view.is_contiguous()
    total, parts = traj_loss(p_view, t_view)
    total.backward()
    vals = torch.stack([total.detach(), *parts])
    fails = []
    check_loss("views", vals, leaf.grad[:, :, 2:2 + seq], shape, fails)
    assert not fails, fails
    assert torch.equal(vals, want_vals) and torch.equal(leaf.grad[:, :, 2:2 + seq], want_grad)
    assert float(leaf.grad[:, :, :2].abs().max()) == 0.0 and float(leaf.grad[:, :, 2 + seq:].abs().max()) == 0.0


def test_loss_gradient_scales_with_the_incoming_gradient_and_repeats_bit_for_bit():
    shape = SR.LOSS_CASES[2]
    pre, tgt, _, _ = loss_reference(shape)
    v1, g1 = gpu_loss(pre, tgt)
    v2, g2 = gpu_loss(pre, tgt)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    v3, g3 = gpu_loss(pre, tgt, scale=3.0)
    assert torch.equal(v1, v3)
    fails = []
    check_loss("3 x total", v3, g3, shape, fails, scale=3.0)
    assert not fails, fails
    assert not torch.equal(g3, g1)


# ---- the optimizer ---------------------------------------------------------------------------------------------------------------
LAYERS, WINDOW = 1, 20


def small_net():
    net = TrajDecoder(nfeats=2, trans_layer=LAYERS, window_size=WINDOW)
    sd = R.synth_state_dict(net)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).eval(), sd


def feed(net, names, step):
    ps = dict(net.named_parameters())
    for k, g in SR.synth_grads(names, step).items():
        ps[k].grad = g.to(DEV)


def state_of(opt, net, key):
    return {k: opt.state[p][key] for k, p in net.named_parameters() if p in opt.state}


_opt_ref = {}


def opt_reference(sd, names, n_steps, wd, decoupled):
    key = (n_steps, wd, decoupled)
    if key not in _opt_ref:
        _opt_ref[key] = (SR.torch_run(sd, names, torch.float64, n_steps, wd, decoupled),
                         SR.torch_run(sd, names, torch.float32, n_steps, wd, decoupled))
    return _opt_ref[key]


def check_against_runs(label, net, sd, names, ref, fails, opt=None):
    (p64, o64), (p32, o32) = ref
    got = {k: p for k, p in net.named_parameters() if k in p64}
    SR.check(label + " update    ", SR.update_errs(got, p64, sd), SR.update_errs(p32, p64, sd), fails)
    if opt is not None:
        for key in ("exp_avg", "exp_avg_sq"):
            s64 = {k: o64.state[p][key] for k, p in p64.items()}
            s32 = {k: o32.state[p][key] for k, p in p32.items()}
            SR.check(f"{label} {key:10s}", SR.state_errs(state_of(opt, net, key), s64), SR.state_errs(s32, s64), fails)


@pytest.mark.parametrize("decoupled,wd", [(True, 0.1), (True, 1e-6), (False, 0.1), (False, 1e-6)],
                         ids=["adamw_wd0.1", "adamw_wd1e-6", "adam_wd0.1", "adam_wd1e-6"])
def test_five_steps_on_synthetic_gradients_against_torch_in_float64(decoupled, wd):
    net, sd = small_net()
    names = SR.trained_names(net)
    opt = TrajAdamW(TrajTrainer(net, dropout=0.0), weight_decay=wd, decoupled=decoupled)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=SR.MILESTONES, gamma=SR.GAMMA)
    for s in range(5):
        feed(net, names, s)
        opt.step()
        sch.step()
    assert abs(opt.param_groups[0]["lr"] - 2e-3 * SR.GAMMA) < 1e-12
    assert all(float(st["step"]) == 5.0 and st["step"].device.type == "cpu" for st in opt.state.values())
    fails = []
    check_against_runs("adamw" if decoupled else "adam", net, sd, names, opt_reference(sd, names, 5, wd, decoupled), fails, opt)
    assert not fails, fails


def real_step(net, trainer, opt, x, cond, target, clone_grads=False):
    total, _ = traj_loss(trainer(x, cond, seed=SEED), target)
    opt.zero_grad()
    total.backward()
    if clone_grads:
        for p in net.parameters():
            if p.grad is not None:
                p.grad = p.grad.clone()
    opt.step()
    return total.detach()


def case_inputs(case):
    name, layers, window, dn, b, frames, p = case
    x, cond = R.synth_inputs("train." + name, window, dn, b, frames)
    return x, cond, TR.synth_target(name, b, dn, window)


def test_gradient_views_and_cloned_gradients_give_the_same_bits():
    case = TR.CASES[0]
    x, cond, target = (t.to(DEV) for t in case_inputs(case))
    runs = []
    for clone in (False, True):
        net = TrajDecoder(nfeats=2, trans_layer=case[1], window_size=case[2])
        net.load_state_dict(R.synth_state_dict(net))
        net.to(DEV).eval()
        trainer = TrajTrainer(net, dropout=case[6])
        opt = TrajAdamW(trainer)
        tables = set()
        for _ in range(3):
            real_step(net, trainer, opt, x, cond, target, clone_grads=clone)
            tables.add(opt._table.data_ptr())
        base = trainer._flat.untyped_storage().data_ptr()
        views = [p.grad.untyped_storage().data_ptr() == base for p in net.parameters() if p.grad is not None]
        assert all(views) if not clone else not any(views)
        if not clone:
            assert len(tables) == 1                              # same pointers every step: the table is built once
        runs.append(({k: v.clone() for k, v in net.state_dict().items()}, opt))
    (sd_a, opt_a), (sd_b, opt_b) = runs
    assert all(torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    for sa, sb in zip(opt_a.state.values(), opt_b.state.values()):
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


def test_packed_images_follow_the_fused_step_and_other_edits_still_repack():
    case = TR.CASES[0]
    x, cond, target = (t.to(DEV) for t in case_inputs(case))
    net = TrajDecoder(nfeats=2, trans_layer=case[1], window_size=case[2])
    net.load_state_dict(R.synth_state_dict(net))
    net.to(DEV).eval()
    trainer = TrajTrainer(net, dropout=case[6])
    opt = TrajAdamW(trainer)
    before = net(x, cond)
    images = net._weights()
    versions = [p._version for p in net.parameters()]
    for _ in range(3):
        real_step(net, trainer, opt, x, cond, target)
    assert net._weights() is images                              # the cache was kept, not rebuilt
    assert all(p._version > v for p, v in zip(net.parameters(), versions) if p.grad is not None)

    def fresh_output():
        fresh = TrajDecoder(nfeats=2, trans_layer=case[1], window_size=case[2])
        fresh.load_state_dict(net.state_dict())
        return fresh.to(DEV).eval()(x, cond)
    out = net(x, cond)
    assert not torch.equal(out, before)
    assert torch.equal(out, fresh_output())
    assert torch.equal(out, TrajTrainer(net, dropout=0)(x, cond, seed=SEED).detach())
    with torch.no_grad():
        net.Decoder[6].bias.add_(0.25)                           # anyone else's in-place edit: the torch path rebuilds
    edited = net(x, cond)
    assert net._weights() is not images
    assert torch.equal(edited, fresh_output()) and not torch.equal(edited, out)
    real_step(net, trainer, opt, x, cond, target)                # and the fused step carries on in the rebuilt images
    assert torch.equal(net(x, cond), fresh_output())


def test_parameters_without_a_gradient_stay_untouched_and_stateless():
    net, sd = small_net()
    names = [(k, s) for k, s in SR.trained_names(net) if k != "Decoder.0.bias"]
    frozen = net.Decoder[0].bias.requires_grad_(False)
    opt = TrajAdamW(TrajTrainer(net, dropout=0.0))
    for s in range(2):
        feed(net, names, s)
        frozen.grad = torch.ones_like(frozen)                    # a stale .grad on a frozen parameter is not an update either
        opt.step()
    ps = dict(net.named_parameters())
    for k in ("trans_extractor.traj_emb.weight", "trans_extractor.traj_emb.bias", "Decoder.0.bias"):
        assert torch.equal(ps[k].detach().cpu(), sd[k]) and ps[k] not in opt.state, k
    assert len(opt.state) == len(names)
    assert not torch.equal(ps["Decoder.0.weight"].detach().cpu(), sd["Decoder.0.weight"])
    saved = opt.state_dict()
    assert len(saved["state"]) == len(names) and set(next(iter(saved["state"].values()))) == {"step", "exp_avg", "exp_avg_sq"}


@pytest.mark.parametrize("direction", ["ours_to_torch", "torch_to_ours"])
def test_state_moves_between_the_fused_optimizer_and_torch_adamw(direction):
    wd = 1e-6
    net, sd = small_net()
    names = SR.trained_names(net)
    ours = TrajAdamW(TrajTrainer(net, dropout=0.0), weight_decay=wd)
    theirs = torch.optim.AdamW(net.parameters(), weight_decay=wd, **SR.HYPER)
    first, second = (ours, theirs) if direction == "ours_to_torch" else (theirs, ours)
    sch = torch.optim.lr_scheduler.MultiStepLR(first, milestones=SR.MILESTONES, gamma=SR.GAMMA)
    for s in range(2):
        feed(net, names, s)
        first.step()
        sch.step()
    second.load_state_dict(first.state_dict())
    assert abs(second.param_groups[0]["lr"] - 2e-3 * SR.GAMMA) < 1e-12
    feed(net, names, 2)
    second.step()
    assert all(float(st["step"]) == 3.0 for st in second.state.values())
    fails = []
    check_against_runs(direction, net, sd, names, opt_reference(sd, names, 3, wd, True), fails, second)
    assert not fails, fails
    x, cond, _ = case_inputs(("step", LAYERS, WINDOW, 2, 2, 50, 0.0))
    fresh = TrajDecoder(nfeats=2, trans_layer=LAYERS, window_size=WINDOW)
    fresh.load_state_dict(net.state_dict())
    assert torch.equal(net(x.to(DEV), cond.to(DEV)), fresh.to(DEV).eval()(x.to(DEV), cond.to(DEV)))


@pytest.mark.parametrize("case", TR.CASES[:2], ids=[c[0] for c in TR.CASES[:2]])
def test_five_whole_steps_follow_the_float64_run(case):
    name, layers, window, dn, b, frames, p = case
    x, cond, target = case_inputs(case)
    net = TrajDecoder(nfeats=2, trans_layer=layers, window_size=window)
    sd = R.synth_state_dict(net)
    net.load_state_dict(sd)
    net.to(DEV).eval()
    keep = TR.masks(SEED, p, layers, b, dn * window)

    def cpu_run(dtype):
        leaf = {k: (v.to(dtype).clone().requires_grad_(True) if TR.is_param(k) else v.to(dtype)) for k, v in sd.items()}
        o = torch.optim.AdamW([v for k, v in leaf.items() if TR.is_param(k)], weight_decay=1e-6, **SR.HYPER)
        sch = torch.optim.lr_scheduler.MultiStepLR(o, milestones=SR.MILESTONES, gamma=SR.GAMMA)
        losses = []
        for _ in range(5):
            loss = TR.loss_fn(TR.forward(leaf, x.to(dtype), cond.to(dtype), layers, keep, p), target.to(dtype))
            o.zero_grad()
            loss.backward()
            o.step()
            sch.step()
            losses.append(float(loss.detach()))
        return losses, {k: v for k, v in leaf.items() if TR.is_param(k) and ".traj_emb." not in k}
    l64, p64 = cpu_run(torch.float64)
    l32, p32 = cpu_run(torch.float32)
    trainer = TrajTrainer(net, dropout=p)
    opt = TrajAdamW(trainer)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=SR.MILESTONES, gamma=SR.GAMMA)
    xd, cd, td = x.to(DEV), cond.to(DEV), target.to(DEV)
    got = []
    for _ in range(5):
        got.append(real_step(net, trainer, opt, xd, cd, td))
        sch.step()
    got = [float(v) for v in got]
    fails = []
    for i, (g, w, y) in enumerate(zip(got, l64, l32)):
        e, y = abs(g - w) / abs(w), abs(y - w) / abs(w)
        print(f"{name} loss at iteration {i}: {g:.9e} (f64 {w:.9e})   {e:.3e}   bound {SR.bound(y):.3e}   (fp32 CPU: {y:.3e})")
        if not e <= SR.bound(y):
            fails.append(("loss", i, e, SR.bound(y)))
    params = {k: v for k, v in net.named_parameters() if k in p64}
    SR.check(f"{name} update after 5", SR.update_errs(params, p64, sd), SR.update_errs(p32, p64, sd), fails)
    assert not fails, fails


def test_refusals():
    pre, tgt = (t.to(DEV) for t in SR.loss_inputs(2, 3, 5))
    with pytest.raises(TcdiffError, match=r"dancer axis \(1\)"):
        traj_loss(pre[:, :1], tgt[:, :1])
    with pytest.raises(TcdiffError, match=r"frame axis \(2\)"):
        traj_loss(pre[:, :, :1], tgt[:, :, :1])
    with pytest.raises(TcdiffError, match="differ in shape"):
        traj_loss(pre, tgt[:, :, :4])
    with pytest.raises(TcdiffError, match="float32"):
        traj_loss(pre.double(), tgt.double())
    with pytest.raises(TcdiffError, match="float32"):
        traj_loss(pre, tgt.half())
    with pytest.raises(TcdiffError, match="MI355X"):
        traj_loss(pre, tgt.cpu())
    net, _ = small_net()
    opt = TrajAdamW(TrajTrainer(net, dropout=0.0))
    with pytest.raises(TcdiffError, match="one parameter group"):
        opt.add_param_group({"params": [torch.zeros(3, device=DEV, requires_grad=True)]})
