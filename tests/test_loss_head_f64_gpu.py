"""The training loss head on MI355X -- tcdiff_amd.diffusion._LossFn and the kernels under it -- against the float64 reference of
tests/loss_ref.py (pinned to the oracle by tests/test_loss_reference_cpu.py), kernel by kernel and region by region:

  a. loss_terms_bwd alone: d_out (recon + velocity) per channel group x first / last / interior frame, d_joints (FK + foot) per
     joint set (root, feet, the rest) -- a foot-term defect is invisible in a whole-tensor norm;
  b. fk_bwd alone on random, identity and near-pi rotations (every quaternion candidate), n at and around the 64-thread block,
     accumulation into a prefilled d_out; the forward joint positions of ax_from_6v + smpl_fk on the same rows;
  c. loss_terms + loss_total with non-trivial p2 weights and active contacts;
  d. the composite: _LossFn through autograd, (k * total).backward();
  e. the wiring through GaussianDiffusion.p_losses (target, p2 weights, l1) with a synthetic denoiser output;
  f. the conditioning-path kernels select_rows, select_rows_bwd, pool_bwd, loss_total.
The bounds and their derivations are loss_ref.BOUNDS."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import loss_ref as R  # noqa: E402
from oracle import tcdiff_oracle as O  # noqa: E402  (checker only)
from tcdiff_amd import diffusion as DF  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd.model import DanceDecoder  # noqa: E402

DEV = "cuda"
D = torch.float64
PAR, OFF = list(O.SMPL_PARENTS), [list(r) for r in O.SMPL_OFFSETS]
B = R.BOUNDS


def gpu_joints(rows):
    """the forward kernels of _LossFn on (n, C) float32 device rows: ax_from_6v of channels 7.., smpl_fk with root 4..6"""
    n, c = rows.shape
    aa = torch.empty(n, 24, 3, device=DEV)
    K.ax_from_6v(rows[:, 7:], n, 24, c, aa)
    j = torch.empty(n, 24, 3, device=DEV)
    K.smpl_fk(aa, rows[:, 4:7].contiguous(), n, PAR, OFF, j)
    return j


def _case(case):
    b, dn, S, l1, p2, cont, gs = case
    mo, tg, t, w = R.make_case(b, dn, S, l1, p2, cont, R.case_seed(case))
    return mo, tg, t, w


def _show(tag, st):
    print(f"{tag}: " + ", ".join(f"{k} {v[0]:.1e}" for k, v in st.items()))


# ---- a. loss_terms_bwd alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[R.case_id(c) for c in R.GPU_CASES])
def test_loss_terms_bwd_alone_vs_float64_by_region(case):
    """fed the float32 images of the reference's joints, so that only loss_terms_bwd's arithmetic is measured"""
    b, dn, S, l1, p2, cont, gs = case
    mo, tg, t, w = _case(case)
    ref = R.loss_head(mo, tg, t, w, l1, gs, with_vjp=False)
    n = b * S * dn
    d_out = torch.full((b, S * dn, 151), float("nan"), device=DEV)
    d_j = torch.full((n, 24, 3), float("nan"), device=DEV)
    K.loss_terms_bwd(mo.to(DEV), tg.to(DEV), ref["jm"].float().to(DEV), ref["jt"].float().to(DEV), w.to(DEV), t.to(DEV),
                     torch.tensor([gs], device=DEV), d_out, d_j, b, dn, S, 151, l1)
    assert bool(torch.isfinite(d_out).all()) and bool(torch.isfinite(d_j).all())       # every element written
    eo = R.region_errors(d_out, ref["d_out_direct"], R.out_regions(S, dn), "out")
    ej = R.region_errors(d_j, ref["d_joints"], R.JOINT_SETS, "joints")
    _show(f"loss_terms_bwd {R.case_id(case)} d_out", eo)
    _show("    d_joints", ej)
    for k, (e, _) in eo.items():
        assert e <= B["out"], (k, e)
    for k, (e, _) in ej.items():
        assert e <= B["joints"][k], (k, e)


# ---- b. fk_bwd alone -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 14400])
def test_fk_bwd_alone_vs_float64_vjp_and_accumulates(n):
    extra = 64                                           # rows past n: must stay untouched
    rows = R.fk_rows(n + extra, R.FK_SEED + n)
    cot = R.fk_cotangent(n + extra, R.FK_SEED + n)
    if n >= 64:
        assert set(R.quat_candidate(rows[:n]).reshape(-1).tolist()) == {0, 1, 2, 3}
    rd, cd = rows.to(DEV), cot.to(DEV)
    g0 = torch.zeros(n + extra, 151, device=DEV)
    K.fk_bwd(rd, cd, n, 151, PAR, OFF, g0)
    G0 = g0.cpu()
    assert not G0[:, :4].any() and not G0[n:].any()
    assert bool(torch.isfinite(G0).all())
    want = R.fk_vjp(rows[:n], cot[:n])
    st = R.fk_errors(G0[:n], want)
    per_kind = {k: R.fk_errors(G0[:n][[i for i in range(n) if R.FK_KINDS[i % 4] == k]],
                               want[[i for i in range(n) if R.FK_KINDS[i % 4] == k]])["rot"]
                for k in set(R.FK_KINDS[:min(n, 4)])}
    # the forward of the same rows: joint positions (not axis-angle, which is ill-conditioned near pi)
    pos = gpu_joints(rd[:n]).cpu().to(D)
    pw = R.joints(rows[:n].to(D))
    pe = float((pos - pw).abs().max() / pw.abs().max())
    print(f"fk_bwd n={n}: rot {st['rot']:.1e}, root {st['root']:.1e}, per kind " +
          ", ".join(f"{k} {v:.1e}" for k, v in per_kind.items()) + f"; positions {pe:.1e}")
    assert st["rot"] <= B["fk_rot"] and st["root"] <= B["fk_root"] and pe <= B["fk_pos"]
    # accumulation: into a prefilled P the result is P + G0 bit for bit, channels 0..3 and the rows past n untouched
    g = torch.Generator().manual_seed(n)
    P = torch.randn(n + extra, 151, generator=g)
    p = P.to(DEV)
    K.fk_bwd(rd, cd, n, 151, PAR, OFF, p)
    want_p = P.clone()
    want_p[:n, 4:] = P[:n, 4:] + G0[:n, 4:]
    assert torch.equal(p.cpu(), want_p)


def test_fk_bwd_on_nearly_degenerate_rotations_is_finite():
    """a2 parallel to a1 (exactly, or to 1e-7): no meaningful gradient, but a finite one"""
    rows = R.degenerate_rows(130, 3)
    cot = R.fk_cotangent(130, 4)
    out = torch.zeros(130, 151, device=DEV)
    K.fk_bwd(rows.to(DEV), cot.to(DEV), 130, 151, PAR, OFF, out)
    assert bool(torch.isfinite(out).all())
    assert bool(torch.isfinite(gpu_joints(rows.to(DEV))).all())


# ---- c. forward: loss_terms + loss_total ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[R.case_id(c) for c in R.GPU_CASES])
def test_loss_terms_and_total_forward_vs_float64(case):
    b, dn, S, l1, p2, cont, gs = case
    mo, tg, t, w = _case(case)
    ref = R.loss_head(mo, tg, t, w, l1, gs, with_vjp=False)
    terms = torch.full((b, 4), float("nan"), device=DEV)
    K.loss_terms(mo.to(DEV), tg.to(DEV), ref["jm"].float().to(DEV), ref["jt"].float().to(DEV), w.to(DEV), t.to(DEV), terms, b, dn,
                 S, 151, l1)
    tot = torch.full((5,), float("nan"), device=DEV)
    K.loss_total(terms, b, tot)
    got = tot.cpu().to(D)
    want = torch.cat([ref["terms"], ref["total"].reshape(1)])
    rel = ((got - want).abs() / want.abs().clamp_min(1e-30)).tolist()
    print(f"loss_terms {R.case_id(case)}: relative error recon {rel[0]:.1e} velocity {rel[1]:.1e} fk {rel[2]:.1e} foot {rel[3]:.1e} "
          f"total {rel[4]:.1e} (foot {float(want[3]):.3e})")
    if cont == "none":
        assert float(got[3]) == 0.0 and float(want[3]) == 0.0
    else:
        assert float(want[3]) > 0
    for k in range(5):
        assert abs(float(got[k] - want[k])) <= B["terms"] * abs(float(want[k])), (k, float(got[k]), float(want[k]))


# ---- d. the composite: _LossFn through autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[R.case_id(c) for c in R.GPU_CASES])
def test_loss_fn_backward_vs_float64_by_region(case):
    b, dn, S, l1, p2, cont, gs = case
    mo, tg, t, w = _case(case)
    out = mo.to(DEV).requires_grad_(True)
    total, m = DF._LossFn.apply(out, tg.to(DEV), t.to(DEV), w.to(DEV), PAR, OFF, l1)
    (gs * total).backward()
    n = b * S * dn
    with torch.no_grad():                                # the kernel's own joints: the l1 signs of its joint differences
        jm = gpu_joints(mo.to(DEV).reshape(n, 151))
        jt = gpu_joints(tg.permute(0, 2, 1, 3).reshape(n, 151).contiguous().to(DEV))
    ref = R.loss_head(mo, tg, t, w, l1, gs, sign_joints=(jm, jt))
    st = R.region_errors(out.grad, ref["d_out"], R.out_regions(S, dn), "out")
    _show(f"_LossFn {R.case_id(case)} d_out", st)
    got_t = torch.cat([m.detach().cpu().to(D), total.detach().cpu().to(D).reshape(1)])
    want_t = torch.cat([ref["terms"], ref["total"].reshape(1)])
    for k in range(5):
        assert abs(float(got_t[k] - want_t[k])) <= B["composite_terms"] * abs(float(want_t[k])), (k, float(got_t[k]), float(want_t[k]))
    for k, (e, _) in st.items():
        assert e <= B["composite"], (k, e)


# ---- e. the wiring through GaussianDiffusion.p_losses -----------------------------------------------------------------------------
U = 2.0 ** -24


def p2_f64(T, use_p2):
    """the p2 weights from the float64 cosine schedule (oracle), and the relative float32 rounding of the module's table allowed at
    each t: betas rounded, 1 - beta, t + 1 cumprod products, 1 - ac (which loses ac / (1 - ac) of it), the quotient and the power"""
    ac = np.cumprod(1 - O.cosine_betas(T))
    gamma = 0.5 if use_p2 else 0.0
    tol = gamma * ((np.arange(T) + 4) * U * ac / (1 - ac) + 4 * U)
    return torch.from_numpy((1 + ac / (1 - ac)) ** -gamma), tol


@pytest.mark.parametrize("loss_type,eps,p2", [("l2", False, False), ("l1", True, False), ("l1", False, True), ("l2", True, True)])
def test_p_losses_wires_the_loss_head(monkeypatch, loss_type, eps, p2):
    """the denoiser output is replaced by out + (synthetic - out).detach() (synthetic: active contacts, l1 ties), so the loss head
    sees values the float64 reference knows while the gradient still reaches the denoiser; a hook captures d_out.  The reference gets
    the correct target (the noise in dataset layout when predict_epsilon) and p2 weights from the float64 schedule."""
    dn, S, T, b = 2, 20, 100, 3
    l1 = loss_type == "l1"
    model = DanceDecoder(nfeats=151, seq_len=S, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                         cond_feature_dim=438, activation=F.gelu, required_dancer_num=dn, compute_dtype="f32")
    model.load_state_dict(O.synth_state_dict(dn=dn, seq_len=S))
    diff = DF.GaussianDiffusion(model, S, 151, None, schedule="cosine", n_timestep=T, predict_epsilon=eps, loss_type=loss_type,
                                use_p2=p2, cond_drop_prob=0.25, guidance_weight=2, seq_len=S).to(DEV).eval()
    g = torch.Generator().manual_seed(31)
    x_start = torch.rand(b, dn, S, 151, generator=g) * 2 - 1
    cond = torch.stack([O.synth_cond(c, S) for c in range(b)])
    noise = torch.randn(b, S, dn, 151, generator=g)
    t = R.timesteps(b, 41)
    keep = torch.tensor([True, False, True])
    syn = R.make_case(b, dn, S, l1, p2, "some", 43)[0]
    real, cap = DF._LossFn, {}

    class Wrapped:
        @staticmethod
        def apply(out, target, tt, p2w, parents, offsets, l1_):
            cap["shape"], cap["l1"] = tuple(out.shape), l1_
            o2 = out + (syn.to(out.device) - out).detach()
            o2.register_hook(lambda gr: cap.__setitem__("d_out", gr.detach().clone()))
            return real.apply(o2, target, tt, p2w, parents, offsets, l1_)

    monkeypatch.setattr(DF, "_LossFn", Wrapped)
    k = 1.7
    total, losses = diff.p_losses(x_start.to(DEV), cond.to(DEV), t.to(DEV), noise=noise.to(DEV), keep_mask=keep.to(DEV))
    (k * total).backward()
    assert cap["shape"] == (b, S * dn, 151) and cap["l1"] == l1
    target = noise.permute(0, 2, 1, 3).contiguous() if eps else x_start
    w64, tol = p2_f64(T, p2)
    slack = float(tol[t].max())
    ref = R.loss_head(syn, target, t, w64, l1, k)
    got_t = torch.stack([lv.detach().cpu().to(D) for lv in losses])
    rel = ((got_t - ref["terms"]).abs() / ref["terms"].abs()).tolist()
    st = R.region_errors(cap["d_out"], ref["d_out"], R.out_regions(S, dn), "out")
    _show(f"p_losses ({loss_type}, eps={eps}, p2={p2}) d_out [p2 slack {slack:.1e}]; terms " + " ".join(f"{v:.1e}" for v in rel), st)
    assert float(ref["terms"][3]) > 0
    for v in rel:
        assert v <= B["composite_terms"] + slack
    for name, (e, _) in st.items():
        assert e <= B["composite"] + slack, (name, e)
    grads = [p.grad for p in diff.model.parameters() if p.grad is not None]
    assert len(grads) > 0 and all(bool(torch.isfinite(q).all()) for q in grads)


# ---- f. the conditioning-path kernels ----------------------------------------------------------------------------------------------
MASKS = [(1, [1]), (1, [0]), (4, [1, 1, 1, 1]), (4, [0, 0, 0, 0]), (4, [1, 0, 0, 1]), (5, [0, 1, 0, 1, 1])]


@pytest.mark.parametrize("Bn,keep", MASKS, ids=[f"B{b}-{''.join(map(str, k))}" for b, k in MASKS])
def test_select_rows_and_its_backward_exact(Bn, keep):
    n = 1000                                             # not a multiple of the 256-thread block
    g = torch.Generator().manual_seed(Bn * 10 + sum(keep))
    x, nul, gr = torch.randn(Bn, n, generator=g), torch.randn(n, generator=g), torch.randn(Bn, n, generator=g)
    kt = torch.tensor(keep, dtype=torch.bool)
    ku = kt.to(torch.uint8).to(DEV)
    out = torch.full((Bn, n), float("nan"), device=DEV)
    K.select_rows(x.to(DEV), nul.to(DEV), ku, out, Bn, n)
    assert torch.equal(out.cpu(), torch.where(kt[:, None], x, nul[None].expand(Bn, n)))
    s = torch.zeros(n)                                   # the fixed-order float32 sum over the dropped clips
    for i in range(Bn):
        if not keep[i]:
            s = s + gr[i]
    want_dx = torch.where(kt[:, None], gr, torch.zeros_like(gr))
    d0 = torch.randn(n, generator=g)
    dx, dnul = torch.full((Bn, n), float("nan"), device=DEV), d0.to(DEV)
    K.select_rows_bwd(gr.to(DEV), ku, dx, dnul, Bn, n)
    assert torch.equal(dx.cpu(), want_dx) and torch.equal(dnul.cpu(), d0 + s)       # dnul accumulates
    dnul2 = d0.to(DEV)
    K.select_rows_bwd(gr.to(DEV), ku, None, dnul2, Bn, n)                          # dx = none
    assert torch.equal(dnul2.cpu(), d0 + s)
    dx2 = torch.full((Bn, n), float("nan"), device=DEV)
    K.select_rows_bwd(gr.to(DEV), ku, dx2, None, Bn, n)                            # dnul = none
    assert torch.equal(dx2.cpu(), want_dx)


@pytest.mark.parametrize("Bn,S", [(1, 1), (3, 61), (2, 150)])
def test_pool_bwd_vs_float64(Bn, S):
    """dx = g_tok + g_pool / S (two float32 roundings), g_tok = none included"""
    C = 512
    g = torch.Generator().manual_seed(S)
    gt, gp = torch.randn(Bn, S, C, generator=g), torch.randn(Bn, C, generator=g)
    for tok in (gt, None):
        dx = torch.full((Bn, S, C), float("nan"), device=DEV)
        K.pool_bwd(None if tok is None else tok.to(DEV), gp.to(DEV), dx, Bn, S, C)
        want = (0 if tok is None else tok.to(D)) + gp.to(D)[:, None, :] / S
        mag = (0 if tok is None else tok.to(D).abs()) + gp.to(D).abs()[:, None, :] / S
        assert bool(((dx.cpu().to(D) - want).abs() <= 2 * U * mag).all())


@pytest.mark.parametrize("b", [1, 3, 32, 100])
def test_loss_total_fixed_order_sum_vs_float64(b):
    """out[k] = coef[k] * mean_b terms[b][k] (b float32 additions, a quotient, a product), out[4] their sum (3 additions)"""
    g = torch.Generator().manual_seed(b)
    terms = torch.rand(b, 4, generator=g) * torch.tensor([1.0, 3.0, 0.1, 1e-3])
    out = torch.full((5,), float("nan"), device=DEV)
    K.loss_total(terms.to(DEV), b, out)
    want = torch.tensor(R.COEF, dtype=D) * terms.to(D).mean(0)
    want = torch.cat([want, want.sum().reshape(1)])
    got = out.cpu().to(D)
    assert bool(((got[:4] - want[:4]).abs() <= (b + 3) * U * want[:4]).all())
    assert abs(float(got[4] - want[4])) <= (b + 6) * U * float(want[4])
    # the same call twice: the fixed-order sum is reproducible
    out2 = torch.full((5,), float("nan"), device=DEV)
    K.loss_total(terms.to(DEV), b, out2)
    assert torch.equal(out, out2)
