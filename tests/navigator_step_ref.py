"""Reference for the Navigator's loss head and optimizer (tcdiff_amd.navigator.traj_loss, TrajAdamW): the loss of
TrajDecoder/train_traj.py:183-196 as that script spells it (F.mse_loss, reduction="none", then the means), a float64 restatement of
its gradient, the yardstick of the GPU tests and the synthetic gradients the optimizer tests feed to every run.

Yardstick (the convention of tests/test_navigator_train_gpu.py): a kernel result may differ from the float64 evaluation by FACTOR = 8
times what the reference's own float32 CPU evaluation differs from it, and never less than FLOOR = 8 * 2^-24 relative -- on the
tiniest shapes the float32 run can be exact, and a loss element passes eight half-ulp roundings: subtract, square, two sum stages,
scale and the three-term combination."""
import os
import sys
import zlib

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navigator_ref as R  # noqa: E402
import navigator_train_ref as TR  # noqa: E402

FACTOR = 8.0
FLOOR = 8.0 * 2.0 ** -24
LOSS_CASES = [(1, 2, 2), (2, 3, 17), (3, 4, 100), (5, 2, 250)]      # (b, dn, seq): ends only, odd length, training shape, T = 500
HYPER = dict(lr=2e-3, betas=(0.5, 0.9), eps=1e-8)                   # option_traj.py's defaults
MILESTONES, GAMMA = [2], 0.05


def bound(err32: float) -> float:
    return max(FACTOR * err32, FLOOR)


def literal_loss(pre_traj, x_target):
    """train_traj.py:183-196: (total, (recon, dis, v)) in the inputs' dtype"""
    def steps(t, axis):                                   # neighbour differences along the dancers (1) or the frames (2)
        n = t.shape[axis]
        return t.narrow(axis, 1, n - 1) - t.narrow(axis, 0, n - 1)
    # elementwise squared errors first, their means afterwards; the two difference terms take the target as first argument
    recon = F.mse_loss(pre_traj, x_target, reduction="none").mean()
    dis = F.mse_loss(steps(x_target, 1), steps(pre_traj, 1), reduction="none").mean()
    v = F.mse_loss(steps(x_target, 2), steps(pre_traj, 2), reduction="none").mean()
    return recon + 2 * dis + 2 * v, (recon, dis, v)


def loss_grad(pre_traj, x_target):
    """d total / d pre_traj, restated: the position term plus the two second-difference terms with their one-sided ends"""
    e = pre_traj - x_target
    g = 2.0 * e / e.numel()
    ed = e[:, 1:] - e[:, :-1]
    g[:, 1:] += 4.0 / ed.numel() * ed
    g[:, :-1] -= 4.0 / ed.numel() * ed
    ev = e[:, :, 1:] - e[:, :, :-1]
    g[:, :, 1:] += 4.0 / ev.numel() * ev
    g[:, :, :-1] -= 4.0 / ev.numel() * ev
    return g


def loss_inputs(b, dn, seq):
    g = torch.Generator().manual_seed(zlib.crc32(f"loss.{b}.{dn}.{seq}".encode()))
    return 0.5 * torch.randn(b, dn, seq, 2, generator=g), 0.5 * torch.randn(b, dn, seq, 2, generator=g)


def loss_and_grad(pre, tgt, dtype, scale=1.0):
    """autograd through the literal expression in `dtype`: (the four scalars [4], d (scale * total) / d pre)"""
    p = pre.to(dtype).clone().requires_grad_(True)
    total, parts = literal_loss(p, tgt.to(dtype))
    (scale * total).backward()
    return torch.stack([total.detach(), *[t.detach() for t in parts]]), p.grad


def scalar_errs(got, want):
    """per scalar |got - want| / |want|, in float64"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return [float(abs(g - w) / abs(w)) for g, w in zip(got, want)]


# ---- the optimizer ---------------------------------------------------------------------------------------------------------------
def synth_grads(names_shapes, step):
    """{name: gradient} of one step: normal entries of size 1e-2, about a tenth exact zeros and a twentieth 1e-12"""
    out = {}
    for name, shape in names_shapes:
        g = torch.Generator().manual_seed(zlib.crc32(f"grad.{step}.{name}".encode()))
        v = 1e-2 * torch.randn(shape, generator=g)
        u = torch.rand(shape, generator=g)
        v[u < 0.10] = 0.0
        v[(u >= 0.10) & (u < 0.15)] = 1e-12
        out[name] = v
    return out


def trained_names(net):
    """the parameters a step updates: all but trans_extractor.traj_emb.*, which forward never uses"""
    return [(k, tuple(p.shape)) for k, p in net.named_parameters() if ".traj_emb." not in k]


def torch_run(sd, names_shapes, dtype, n_steps, weight_decay, decoupled, first_step=0):
    """`n_steps` of torch.optim.AdamW / Adam with MultiStepLR on CPU copies of `sd` in `dtype`, fed synth_grads.
    Returns ({name: parameter}, optimizer)."""
    ps = {k: sd[k].to(dtype).clone().requires_grad_(True) for k, _ in names_shapes}
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(list(ps.values()), weight_decay=weight_decay, **HYPER)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=MILESTONES, gamma=GAMMA)
    for s in range(first_step, first_step + n_steps):
        for k, g in synth_grads(names_shapes, s).items():
            ps[k].grad = g.to(dtype)
        opt.step()
        sch.step()
    return ps, opt


def update_errs(got, want, start, group_of=TR.group_of):
    """{group: max|got - want| / max|want - start|}: the error of the UPDATE (a parameter's leading digits never move)"""
    num, den = {}, {}
    for k, w in want.items():
        g, w, s = got[k].detach().cpu().double(), w.detach().cpu().double(), start[k].detach().cpu().double()
        grp = group_of(k)
        num[grp] = max(num.get(grp, 0.0), float((g - w).abs().max()))
        den[grp] = max(den.get(grp, 0.0), float((w - s).abs().max()))
    return {k: num[k] / den[k] for k in num}


def state_errs(got, want, group_of=TR.group_of):
    """{group: max|got - want| / max|want|} of one state entry ({name: tensor})"""
    num, den = {}, {}
    for k, w in want.items():
        g, w = got[k].detach().cpu().double(), w.detach().cpu().double()
        grp = group_of(k)
        num[grp] = max(num.get(grp, 0.0), float((g - w).abs().max()))
        den[grp] = max(den.get(grp, 0.0), float(w.abs().max()))
    return {k: num[k] / den[k] for k in num}


def check(label, errs, yard, fails):
    """print every figure with its bound; collect the misses"""
    for grp in sorted(errs):
        b = bound(yard[grp])
        print(f"{label} {grp:18s}: {errs[grp]:.3e}   bound {b:.3e}   (fp32 CPU: {yard[grp]:.3e})")
        if not errs[grp] <= b:
            fails.append((label, grp, errs[grp], b))
