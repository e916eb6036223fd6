"""MI355X-native ``GaussianDiffusion`` -- drop-in for the reference's ``model.diffusion.GaussianDiffusion``.

Same constructor arguments, registered buffers and sampler methods (reference model/diffusion.py:79-806).
Every sampler step is: one stacked (unconditional | conditional) evaluation of the denoiser in HIP kernels,
then ONE fused kernel doing CFG combine + clamp + the DDPM / DDIM update (+ trajectory in-painting), with the
step scalars read from device memory so that a single captured hipGraph is replayed for every step.

Out of scope here: the stick-figure renderer behind ``render_sample`` (this class returns
the samples instead) and the backward pass of the training loss (``p_losses`` is forward-only).
"""
from __future__ import annotations

import copy
import os
from functools import partial
from typing import Callable, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import kernels as K
from .step_graphs import StepSpec, plan_runs, steps_per_graph


def cosine_beta_schedule(n_timestep: int, cosine_s: float = 8e-3) -> np.ndarray:
    """fp64 cosine schedule (reference model/utils.py:78-86)."""
    steps = torch.arange(n_timestep + 1, dtype=torch.float64) / n_timestep + cosine_s
    ac = torch.cos(steps / (1 + cosine_s) * np.pi / 2).pow(2)
    ac = ac / ac[0]
    return np.clip((1 - ac[1:] / ac[:-1]).numpy(), a_min=0, a_max=0.999)


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3) -> np.ndarray:
    if schedule == "cosine":
        return cosine_beta_schedule(n_timestep, cosine_s)
    if schedule == "linear":
        return (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=torch.float64) ** 2).numpy()
    if schedule == "sqrt_linear":
        return torch.linspace(linear_start, linear_end, n_timestep, dtype=torch.float64).numpy()
    if schedule == "sqrt":
        return (torch.linspace(linear_start, linear_end, n_timestep, dtype=torch.float64) ** 0.5).numpy()
    raise ValueError(f"schedule '{schedule}' unknown.")


def extract(a, t, x_shape):
    b, *_ = t.shape
    return a.gather(-1, t).reshape(b, *((1,) * (len(x_shape) - 1)))


class EMA:
    """Exponential moving average of parameters (reference model/diffusion.py:61-76).

    On the GPU the whole parameter list is updated by ONE launch of tcdiff_ema_update (the reference issues three
    elementwise kernels per tensor, 435 tensors); the rounding is the reference's (`old * beta + (1 - beta) * new`,
    products rounded separately).  No CPU fallback: parameters that are not contiguous fp32 CUDA tensors raise."""

    def __init__(self, beta):
        self.beta = beta
        self._table = None
        self._table_key = None

    def update_model_average(self, ma_model, current_model):
        cur_p, ma_p = list(current_model.parameters()), list(ma_model.parameters())
        key = tuple(p.data_ptr() for p in cur_p) + tuple(p.data_ptr() for p in ma_p)
        if key != self._table_key:                       # (re)allocation: decide the path and rebuild the chunk table
            ts = [p.data for p in cur_p + ma_p]
            fused = len(cur_p) > 0 and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts)
            self._table = K.ema_chunk_table([p.data for p in ma_p], [p.data for p in cur_p],
                                            cur_p[0].device) if fused else None
            self._table_key = key
        if self._table is None:
            raise L.TcdiffError("EMA.update_model_average runs as one fused HIP launch over contiguous fp32 CUDA parameters "
                                "(no CPU fallback): move both models to the GPU")
        K.ema_update(self._table, self.beta)
        # the kernel wrote through raw pointers: bump ._version so DanceDecoder._weights_version sees new weights
        # (packed bf16 copies, conditioning caches and captured graphs are keyed by it)
        torch.autograd.graph.increment_version(ma_p)

    def update_average(self, old, new):
        return new if old is None else old * self.beta + (1 - self.beta) * new


class _LossFn(torch.autograd.Function):
    """total = 0.636 recon + 2.964 velocity + 0.646 fk + 10.942 foot (reference model/diffusion.py:668-741) of the denoiser
    output, forward and backward in HIP kernels (csrc/train.hip, csrc/train_ops.hip): 6-D rotations -> axis-angle ->
    SMPL chain -> the four per-clip means; the reverse pass differentiates the same chain by hand (csrc/fk_math.h)."""

    @staticmethod
    def forward(ctx, out, x_start, t, p2w, parents, offsets, l1):
        dev = out.device
        bs, dn, sq, c = x_start.shape
        out = out.detach().float().contiguous()
        n = bs * sq * dn
        xs_rows = x_start.permute(0, 2, 1, 3).reshape(n, c).contiguous()      # target rows in token order (a copy)
        joints = []
        for rows in (out.reshape(n, c), xs_rows):
            aa = torch.empty(n, 24, 3, device=dev)
            K.ax_from_6v(rows[:, 7:], n, 24, c, aa)               # channels: 4 contact, 3 root, 24 x 6 rotations
            jt = torch.empty(n, 24, 3, device=dev)
            K.smpl_fk(aa, rows[:, 4:7].contiguous(), n, parents, offsets, jt)
            joints.append(jt)
        terms = torch.empty(bs, 4, device=dev)
        K.loss_terms(out, x_start, joints[0], joints[1], p2w, t, terms, bs, dn, sq, c, l1=l1)
        tot = torch.empty(5, device=dev)
        K.loss_total(terms, bs, tot)
        m = tot[:4].clone()
        ctx.save_for_backward(out, x_start, t, p2w, joints[0], joints[1])
        ctx.meta = (parents, offsets, l1)
        ctx.mark_non_differentiable(m)
        return tot[4].clone(), m

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        out, x_start, t, p2w, jm, jt = ctx.saved_tensors
        parents, offsets, l1 = ctx.meta
        bs, dn, sq, c = x_start.shape
        n = bs * sq * dn
        d_out = torch.empty_like(out)
        d_j = torch.empty(n, 24, 3, device=out.device)
        gs = g_total.detach().reshape(1).float().contiguous()
        K.loss_terms_bwd(out, x_start, jm, jt, p2w, t, gs, d_out, d_j, bs, dn, sq, c, l1)
        K.fk_bwd(out.reshape(n, c), d_j, n, c, parents, offsets, d_out.reshape(n, c))
        return d_out, None, None, None, None, None, None


FOOT_JOINTS = [1, 2, 3, 4, 5, 7, 8, 10, 11]  # lower-body joints of ddim_sample_Footwork (model/diffusion.py:307)


def sampler_steps(eng, st: dict, spec: StepSpec, u: int = 1):
    """u sampler steps on the engine's sampler state `st`: the body of a captured step graph.  Which launches it issues, with which
    arguments, comes from `spec` alone -- the graph's key -- so a graph cannot be replayed for a body it was not captured from."""
    mode, branches, noise, traj, clip_offset, B, kind, q_noise, mask_rows, cparams, couple, form = spec
    rows, nf = st["x"].shape
    Lq = rows // B
    for _ in range(u):
        eng.step_prologue(st, 2 * B, st["x"], rows, form)
        if branches == 2:
            out = eng.network(st["x"], B, 2, 0, B, 0, x_ready=True, form=form)
            unc, con = out, out[rows:]
        else:
            out = eng.network(st["x"], B, 1, 1, 0, B, x_ready=True, form=form)
            unc, con = None, out
        K.sampler_update(mode | L.SAMPLER_ADVANCE, unc, con, 152, st["x"], st["eps"] if noise else None,
                         st["traj"] if traj else None, None, rows, nf, Lq, st["counter"], st["params"], st["tseq"], seed=0,
                         clip0=clip_offset)
        if kind is not None:
            K.sampler_constrain(kind, st["x"], st["cmask"], mask_rows, st["cval"], st["qeps"] if q_noise else None, rows, nf, Lq,
                                st["counter"], st["cparams"] if cparams else st["params"], st["tseq"], seed=0, clip0=clip_offset)
        if couple is not None:
            K.window_couple_step(st["x"], B, couple[0], couple[1], st["counter"], st["params"])


def _capture(body: Callable[[], None]):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    return graph


class GaussianDiffusion(nn.Module):
    def __init__(self, model, horizon, repr_dim, smpl, n_timestep=1000, schedule="linear", loss_type="l1",
                 clip_denoised=True, predict_epsilon=True, guidance_weight=3, use_p2=False, cond_drop_prob=0.2,
                 seq_len=150):
        super().__init__()
        self.horizon = horizon
        self.transition_dim = repr_dim
        self.model = model
        self.ema = EMA(0.9999)
        self.master_model = copy.deepcopy(self.model)
        self.seq_len = seq_len
        self.cond_drop_prob = cond_drop_prob
        self.smpl = smpl
        self.n_timestep = int(n_timestep)
        self.clip_denoised = clip_denoised
        self.predict_epsilon = predict_epsilon
        self.guidance_weight = guidance_weight
        self.loss_type = loss_type

        # the 13 fp32 [T] tables (reference model/diffusion.py:109-169): betas are rounded to fp32 first and
        # everything downstream is fp32; coef1/coef2 use numpy's sqrt like the reference does
        betas = torch.Tensor(make_beta_schedule(schedule=schedule, n_timestep=n_timestep))
        alphas = 1.0 - betas
        ac = torch.cumprod(alphas, axis=0)
        ac_prev = torch.cat([torch.ones(1), ac[:-1]])
        reg = self.register_buffer
        reg("betas", betas)
        reg("alphas_cumprod", ac)
        reg("alphas_cumprod_prev", ac_prev)
        reg("sqrt_alphas_cumprod", torch.sqrt(ac))
        reg("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - ac))
        reg("log_one_minus_alphas_cumprod", torch.log(1.0 - ac))
        reg("sqrt_recip_alphas_cumprod", torch.sqrt(1.0 / ac))
        reg("sqrt_recipm1_alphas_cumprod", torch.sqrt(1.0 / ac - 1))
        post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
        reg("posterior_variance", post_var)
        reg("posterior_log_variance_clipped", torch.log(torch.clamp(post_var, min=1e-20)))
        reg("posterior_mean_coef1", betas * torch.from_numpy(np.sqrt(ac_prev.numpy())) / (1.0 - ac))
        reg("posterior_mean_coef2", (1.0 - ac_prev) * torch.from_numpy(np.sqrt(alphas.numpy())) / (1.0 - ac))
        self.p2_loss_weight_k = 1
        self.p2_loss_weight_gamma = 0.5 if use_p2 else 0
        reg("p2_loss_weight", (self.p2_loss_weight_k + ac / (1 - ac)) ** -self.p2_loss_weight_gamma)

    # ------------------------------------------------------------------------------------------
    # fused sampler core
    # ------------------------------------------------------------------------------------------
    def _device(self):
        return self.betas.device

    def _guidance_weight_at(self, i: int, w=None) -> float:
        """Guidance clipping of p_mean_variance (reference model/diffusion.py:219-224)."""
        w = self.guidance_weight if w is None else w
        if i > 1.0 * self.n_timestep:
            return min(w, 0)
        if i < 0.1 * self.n_timestep:
            return min(w, 1)
        return w

    def _prepare(self, B: int, cond: torch.Tensor, tseq, slot: int = 0, eng=None):
        """Step-invariant work, once per sampler call: music encoder, cross-attention caches, time tables.  `eng`: the engine the
        caller already fetched for this job (model.engine() walks all 435 parameters for in-place changes: 0.3 ms, once per job)."""
        eng = self.model.engine(B, slot) if eng is None else eng
        b = eng.b
        dev = eng.dev
        tok, hid = eng.encode_music(cond.to(dev))
        eng.fill_kv_slots(eng.w["null_embed"], 1, 0)
        eng.fill_kv_slots(tok, B, 1)
        b["hidden_all"][:B] = eng.w["null_hidden"]
        b["hidden_all"][B:2 * B] = hid
        uniq, rows = self._time_rows(tseq)
        key = (eng.weights_version, tuple(uniq))
        if eng.tables_key != key:
            eng.build_time_tables(torch.tensor(uniq, dtype=torch.int32, device=dev))
            eng.tables_key = key
            eng.reset_graphs()
        # the FiLM rows of every (timestep, conditioning row) of this job as one GEMM; graphs hold the table's address
        old = eng.film_tab.data_ptr() if eng.film_tab is not None else None
        if os.environ.get("TCDIFF_FILM_TABLE", "1") != "0" and len(uniq) > 2:
            tab = eng.build_film_table(B)
        else:
            eng.film_tab = tab = None
        if (tab.data_ptr() if tab is not None else None) != old:
            eng.reset_graphs()
        return eng, rows

    _steps_per_graph = staticmethod(steps_per_graph)

    @staticmethod
    def _time_rows(tseq):
        """(sorted distinct timesteps of a job, the row of every step in the per-job time tables)"""
        uniq = sorted(set(int(t) for t in tseq))
        row_of = {t: i for i, t in enumerate(uniq)}
        return uniq, [row_of[int(t)] for t in tseq]

    def _upload_job(self, eng, shape, x, tseq, params, traj, constrain, seed: int):
        """The job's start and step tables into the engine's sampler state.  Returns (the state, the time-table row of every step, the
        rows of the constraint's mask).
        Host-to-device copies only, issued BEFORE the job's device work (_prepare: music branch, caches, tables): a copy from pageable
        host memory blocks the host until everything queued before it has run, and behind _prepare's ~40 launches that was 0.6 ms of
        host wait per job plus the launches that could not be queued meanwhile (a one-clip ddim_sample is 27 ms)."""
        B, Lq, nf = shape
        n = len(tseq)
        rows = self._time_rows(tseq)[1]
        st = eng.sampler_state(n, B * Lq, nf)
        st["x"].copy_(x.reshape(B * Lq, nf))
        st["counter"].zero_()
        st["rows"][:n] = torch.tensor(rows, dtype=torch.int32)
        st["tseq"][:n] = torch.tensor([int(t) for t in tseq], dtype=torch.int32)
        st["params"][:n] = params.to(torch.float32)
        # the constraint kernel's own step table (q_sample coefficients in columns 4, 5, enable bit in column 7): separate from the
        # update kernel's, whose columns 4, 5 carry the predict_epsilon coefficients
        if constrain is not None and constrain.get("params") is not None:
            st["cparams"][:n] = constrain["params"].to(torch.float32)
        if traj is not None:
            st["traj"].copy_(traj.reshape(B * Lq, 3))
        mask_rows = 0
        if constrain is not None:
            st["cval"].copy_(constrain["value"].reshape(B * Lq, nf))
            m = constrain["mask"].to(st["x"].device, torch.float32).reshape(-1, nf)
            mask_rows = Lq if m.shape[0] == Lq else B * Lq      # one [L, nfeat] mask for every clip, or a full one
            st["cmask"][:mask_rows].copy_(m)
        # the seed lives in device memory (counter[1..2]) so that a captured graph can be re-seeded
        st["counter"][1:3] = torch.tensor([seed & 0x7FFFFFFF, (seed >> 31) & 0x7FFFFFFF], dtype=torch.int32)
        return st, rows, mask_rows

    def _run(self, mode: int, shape, cond, x: torch.Tensor, tseq, params: torch.Tensor, *, traj=None,
             step_noise: Optional[Callable] = None, seed: Optional[int] = None, clip_offset: int = 0,
             after_step: Optional[Callable] = None, use_graph: bool = True, collect=None, constrain=None, couple=None):
        """Run len(tseq) sampler steps on x (fp32 [B, L, nfeat]); returns the updated tensor.

        constrain = dict(kind, mask [L or B*L, nfeat] float, value [B, L, nfeat], q_noise=None | callable(t, shape)) and
        couple = (seq_len, row_elems) put the in-painting constraint / window coupling INSIDE the captured step
        (tcdiff_sampler_constrain / tcdiff_window_couple_step, enabled per step by params[:, 7] bits 1 / 0), so those
        samplers replay one graph per step like the plain ones; `after_step` remains for callers' own hooks."""
        B, Lq, nf = shape
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        branches = [1 if w == 1.0 else 2 for w in params[:, 0].tolist()]
        # one stream, one launch chain: with one resident-block kernel per layer the chip is full, and two half-batch chains on
        # two streams measured 3 % slower (rounds 1-3 kept that as a default-off option; removed in round 4)
        eng = self.model.engine(B, 0)
        st, rows, mask_rows = self._upload_job(eng, shape, x, tseq, params, traj, constrain, seed)
        assert self._prepare(B, cond, tseq, slot=0, eng=eng)[1] == rows
        graphs = eng.step_graphs                # (fetched after _prepare, which drops them when a table moved)
        q_noise = constrain.get("q_noise") if constrain is not None else None
        # Every per-step quantity lives in device memory (counter, step tables, seed), so one captured graph serves every step -- and
        # SEVERAL consecutive steps of the same kind can be one graph: a replay boundary costs ~8 us of GPU idle time
        # (profiles/r04_gap_analysis.txt), 0.8 % of a 1.05-ms step.  Runs of `unroll` steps with the same branch count and no host work
        # between them (injected noise, callbacks, collected states) replay a graph of that many steps; the rest go one by one.
        hostless = step_noise is None and q_noise is None and after_step is None and collect is None
        unroll = max(1, int(os.environ.get("TCDIFF_GRAPH_STEPS", "20"))) if (use_graph and hostless) else 1
        for i, u in plan_runs(branches, unroll):
            t = int(tseq[i])
            if step_noise is not None:
                st["eps"].copy_(step_noise(t, (B, Lq, nf)).reshape(B * Lq, nf))
            if q_noise is not None:
                st["qeps"].copy_(q_noise(t, (B, Lq, nf)).reshape(B * Lq, nf))
            # (the form is resolved from the engine's switches as they are now: a switch changed after a capture is another key)
            spec = StepSpec(mode=mode, branches=branches[i], noise=step_noise is not None, traj=traj is not None,
                            clip_offset=clip_offset, B=B, kind=None if constrain is None else constrain["kind"],
                            q_noise=q_noise is not None, mask_rows=mask_rows,
                            cparams=constrain is not None and constrain.get("params") is not None, couple=couple,
                            form=eng.form(branches[i] * B))
            body = partial(sampler_steps, eng, st, spec, u)
            if use_graph:
                graphs.visit((spec, u), body, _capture)
            else:
                body()
            if after_step is not None:
                after_step(i + u - 1, t, st["x"].view(B, Lq, nf))
            if collect is not None:
                collect.append(st["x"].view(B, Lq, nf).clone())
        return st["x"].view(B, Lq, nf).clone()

    # ------------------------------------------------------------------------------------------
    # reference sampling API
    # ------------------------------------------------------------------------------------------
    def predict_start_from_noise(self, x_t, t, noise):
        """reference model/diffusion.py:176-187 (inside the samplers the update kernel does this itself, _ddpm_params)"""
        if self.predict_epsilon:
            return extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - \
                extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise
        return noise

    def predict_noise_from_start(self, x_t, t, x0):
        return (extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - x0) / \
            extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape)

    @torch.no_grad()
    def model_predictions(self, x, cond, t, weight=None, clip_x_start=False):
        weight = weight if weight is not None else self.guidance_weight
        x_start = self.model.guided_forward(x, cond, t, weight)
        if clip_x_start:
            x_start = torch.clamp(x_start, min=-1.0, max=1.0)
        return self.predict_noise_from_start(x, t, x_start), x_start

    def q_posterior(self, x_start, x_t, t):
        mean = extract(self.posterior_mean_coef1, t, x_t.shape) * x_start + \
            extract(self.posterior_mean_coef2, t, x_t.shape) * x_t
        return mean, extract(self.posterior_variance, t, x_t.shape), \
            extract(self.posterior_log_variance_clipped, t, x_t.shape)

    @torch.no_grad()
    def p_mean_variance(self, x, cond, t):
        """reference model/diffusion.py:215-239 (predict_start_from_noise is the identity unless predict_epsilon)"""
        weight = self._guidance_weight_at(int(t[0]))
        x_recon = self.predict_start_from_noise(x, t, self.model.guided_forward(x, cond, t, weight))
        if self.clip_denoised:
            x_recon = x_recon.clamp_(-1.0, 1.0)
        mean, var, logvar = self.q_posterior(x_start=x_recon, x_t=x, t=t)
        return mean, var, logvar, x_recon

    def _cached_params(self, key, make) -> torch.Tensor:
        """Step tables are functions of the (constant) schedule buffers and the options in `key`: computed once per process and key on the
        host (three device-to-host copies and, for DDIM, ~20 tensor ops per step -- a millisecond of host time in front of a 27-ms
        one-clip job), handed out as copies (callers edit theirs)."""
        cache = self.__dict__.setdefault("_param_cache", {})
        key = key + (self.n_timestep, bool(self.predict_epsilon), bool(self.clip_denoised))      # (the schedule of an instance never changes)
        if key not in cache:
            if len(cache) >= 32:
                cache.clear()
            cache[key] = make()
        return cache[key].clone()

    def _ddpm_params(self, tseq, weight=None) -> torch.Tensor:
        tk = tuple(int(i) for i in tseq)
        return self._cached_params(("ddpm", tk, None if weight is None else float(weight), float(self.guidance_weight)),
                                   lambda: self._make_ddpm_params(tk, weight))

    def _make_ddpm_params(self, tseq, weight=None) -> torch.Tensor:
        t = torch.tensor([int(i) for i in tseq], dtype=torch.long)
        c1 = self.posterior_mean_coef1.cpu()[t]
        c2 = self.posterior_mean_coef2.cpu()[t]
        sig = (1 - (t == 0).float()) * (0.5 * self.posterior_log_variance_clipped.cpu()[t]).exp()
        p = torch.zeros(len(tseq), 8)
        p[:, 0] = torch.tensor([float(self._guidance_weight_at(int(i), weight)) for i in tseq])
        p[:, 1], p[:, 2], p[:, 3] = c1, c2, sig
        # constructor options outside the production configuration (model/diffusion.py:80-95,176-187,230-233): the update
        # kernel forms x_0 = sqrt(1/ac) x_t - sqrt(1/ac - 1) eps_hat itself (flag bit 2) and skips the clamp (bit 3)
        p[:, 4], p[:, 5] = self.sqrt_recip_alphas_cumprod.cpu()[t], self.sqrt_recipm1_alphas_cumprod.cpu()[t]
        p[:, 7] = (4 if self.predict_epsilon else 0) + (0 if self.clip_denoised else 8)
        return p

    @torch.no_grad()
    def p_sample(self, x, cond, t, *, noise=None, seed=None):
        """One reverse step (reference model/diffusion.py:241-252); returns (x_{t-1}, x_start)."""
        i = int(t[0])
        shape = tuple(x.shape)
        x0_holder = []
        eng = self.model.engine(shape[0])
        out = self._run(L.SAMPLER_DDPM, shape, cond, x.float(), [i], self._ddpm_params([i]),
                        step_noise=(lambda _t, s: noise) if noise is not None else None, seed=seed, use_graph=False)
        # x_start = clamp(guided) is recomputed from the network outputs of that step
        b, B, Lq = eng.b, shape[0], shape[1]
        w = self._guidance_weight_at(i)
        y = torch.empty(B, Lq, shape[2], device=out.device, dtype=torch.float32)
        K.cfg_combine(b["out"], b["out"][B * Lq:] if w != 1.0 else b["out"], 152, float(w), y, B * Lq, shape[2])
        y = self.predict_start_from_noise(x.to(y).reshape(y.shape), t.to(y.device).long(), y)     # identity unless predict_epsilon
        return out, (y.clamp_(-1.0, 1.0) if self.clip_denoised else y)

    @torch.no_grad()
    def p_sample_loop(self, shape, cond, noise=None, constraint=None, return_diffusion=False, start_point=None, *,
                      step_noise=None, seed=None, clip_offset=0, use_graph=True):
        """T sequential DDPM steps (reference model/diffusion.py:255-286).

        Extra keyword-only arguments: ``step_noise(t, shape)`` injects the per-step N(0,1) draw (parity tests);
        otherwise eps comes from an in-kernel Philox stream keyed by (seed, clip_offset + clip, t, element), so
        the NOISE of a clip does not depend on the batch it is in or on how clips are sharded over GPUs.  Its sample does in
        bf16 only: the per-rank job size picks the kernel family of the decoder layers (small jobs: tcdiff_chain_split), another
        fp32 summation order, so a clip sampled alone and inside a larger job differ by bf16 rounding (f32 / bf16x3: identical)."""
        device = self._device()
        start_point = self.n_timestep if start_point is None else start_point
        x = torch.randn(shape, device=device) if noise is None else noise.to(device)
        tseq = list(reversed(range(0, start_point)))
        chain = [x] if return_diffusion else None
        out = self._run(L.SAMPLER_DDPM, tuple(shape), cond, x.float(), tseq, self._ddpm_params(tseq),
                        step_noise=step_noise, seed=seed, clip_offset=clip_offset, use_graph=use_graph, collect=chain)
        return (out, chain) if return_diffusion else out

    # ---- DDIM ------------------------------------------------------------------------------------
    def _ddim_pairs(self, sampling_timesteps=50):
        times = torch.linspace(-1, self.n_timestep - 1, steps=sampling_timesteps + 1)
        times = list(reversed(times.int().tolist()))
        return list(zip(times[:-1], times[1:]))

    def _ddim_params(self, pairs, weights) -> torch.Tensor:
        pk, wk = tuple((int(a), int(b)) for a, b in pairs), tuple(float(w) for w in weights)
        return self._cached_params(("ddim", pk, wk), lambda: self._make_ddim_params(pk, wk))

    def _make_ddim_params(self, pairs, weights) -> torch.Tensor:
        ac = self.alphas_cumprod.cpu()
        sr, srm1 = self.sqrt_recip_alphas_cumprod.cpu(), self.sqrt_recipm1_alphas_cumprod.cpu()
        p = torch.zeros(len(pairs), 8)
        for i, ((time, time_next), w) in enumerate(zip(pairs, weights)):
            p[i, 0], p[i, 1], p[i, 2] = float(w), sr[time], srm1[time]
            p[i, 7] = 0 if self.clip_denoised else 8      # clip_x_start=self.clip_denoised (model/diffusion.py:316,409,476)
            if time_next < 0:
                p[i, 6] = 1.0
                continue
            alpha, alpha_next = ac[time], ac[time_next]
            sigma = 1 * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()   # eta = 1
            c = (1 - alpha_next - sigma ** 2).sqrt()
            p[i, 3], p[i, 4], p[i, 5] = alpha_next.sqrt(), c, sigma
        return p

    @torch.no_grad()
    def ddim_sample(self, shape, cond, x_0=None, **kwargs):
        """50-step DDIM, eta=1, optional trajectory in-painting of channels 4,5 (reference model/diffusion.py:386-442).
        ``noise=``/``start_point=``/``constraint=`` are accepted and ignored like the reference's **kwargs does;
        recognised extras: init_noise, step_noise, seed, clip_offset."""
        device = self._device()
        B, Lq, nf = shape
        init = kwargs.get("init_noise")
        x = torch.randn(shape, device=device) if init is None else init.to(device).float().clone()
        traj = None
        if x_0 is not None:
            traj = x_0.to(device).float().reshape(B, Lq, 3)
            x.view(B, Lq, nf)[:, :, 4:6] = traj[:, :, 0:2]
        pairs = self._ddim_pairs()
        params = self._ddim_params(pairs, [self.guidance_weight] * len(pairs))
        out = self._run(L.SAMPLER_DDIM, (B, Lq, nf), cond, x, [a for a, _ in pairs], params, traj=traj,
                        step_noise=kwargs.get("step_noise"), seed=kwargs.get("seed"),
                        clip_offset=kwargs.get("clip_offset", 0))
        return out

    @torch.no_grad()
    def long_ddim_sample(self, shape, cond, x_0, **kwargs):
        """Half-overlapping windows generated as one batch, coupled every step (reference model/diffusion.py:446-515)."""
        B, Lq, nf = shape
        halo = kwargs.get("halo_exchange")      # callable(x_view): cross-rank boundary copy (tcdiff_amd/stitch.py); the
        if B == 1 and halo is None:              # windows of one song sharded over ranks stay "long" with one per rank
            return self.ddim_sample(shape, cond, **{k: v for k, v in kwargs.items()
                                                    if k in ("init_noise", "step_noise", "seed", "clip_offset")})
        device = self._device()
        init = kwargs.get("init_noise")
        x = torch.randn(shape, device=device) if init is None else init.to(device).float().clone()
        traj = None
        if x_0 is not None:
            traj = x_0.to(device).float().reshape(B, Lq, 3)
            x.view(B, Lq, nf)[:, :, 4:6] = traj[:, :, 0:2]
        assert B > 1 or halo is not None
        assert self.seq_len % 2 == 0
        pairs = self._ddim_pairs()
        weights = np.clip(np.linspace(0, self.guidance_weight * 2, 50), None, self.guidance_weight)
        params = self._ddim_params(pairs, weights)
        row = (Lq // self.seq_len) * nf
        for i, (time, time_next) in enumerate(pairs):       # x[1:, :half] = x[:-1, half:] after every step but the last
            params[i, 7] += 1.0 if (time_next >= 0 and time > 0) else 0.0      # (bit 3, no clamp, stays: _ddim_params)
        after = None
        if halo is not None:
            def after(i, t, xv):
                if pairs[i][1] >= 0 and t > 0:
                    halo(xv)
        return self._run(L.SAMPLER_DDIM, (B, Lq, nf), cond, x, [a for a, _ in pairs], params, traj=traj,
                         step_noise=kwargs.get("step_noise"), seed=kwargs.get("seed"),
                         clip_offset=kwargs.get("clip_offset", 0), couple=(self.seq_len, row), after_step=after)

    def _footwork_mask(self, Lq, nf, dn, device):
        m = torch.zeros(self.seq_len, dn, nf, dtype=torch.bool, device=device)
        for j in FOOT_JOINTS:
            m[75:120, :, 4 + 3 + (j - 1) * 6: 4 + 3 + j * 6] = True
        return m.reshape(Lq, nf)

    @torch.no_grad()
    def ddim_sample_Footwork(self, shape, cond, x_0=None, **kwargs):
        """DDIM with trajectory + lower-body rotation in-painting on frames 75:120 and a 10-frame linear blend at
        the end (reference model/diffusion.py:289-383).  The in-painting copies are tensor plumbing; the network
        and the DDIM update are the same kernels as ddim_sample."""
        device = self._device()
        B, Lq, nf = shape
        dn = Lq // self.seq_len
        init = kwargs.get("init_noise")
        x = torch.randn(shape, device=device) if init is None else init.to(device).float().clone()
        pairs = self._ddim_pairs()
        params = self._ddim_params(pairs, [self.guidance_weight] * len(pairs))
        traj, constrain = None, None
        if x_0 is not None:
            x_0 = x_0.to(device).float().reshape(B, Lq, nf)
            mask = self._footwork_mask(Lq, nf, dn, device)
            traj = torch.zeros(B, Lq, 3, device=device)
            traj[:, :, 0:2] = x_0[:, :, 0:2]        # the reference copies x_0[...,[0,1]] of the 151-d x_0 into x[...,[4,5]] (:303)
            x[:, :, 4:6] = x_0[:, :, 0:2]
            x = torch.where(mask[None], x_0, x)
            constrain = dict(kind=1, mask=mask.float(), value=x_0)     # re-imposed inside every captured step but the last
            for i, (_, time_next) in enumerate(pairs):
                params[i, 7] += 2.0 if time_next >= 0 else 0.0
        x = self._run(L.SAMPLER_DDIM, (B, Lq, nf), cond, x, [a for a, _ in pairs], params, traj=traj,
                      step_noise=kwargs.get("step_noise"), seed=kwargs.get("seed"),
                      clip_offset=kwargs.get("clip_offset", 0), constrain=constrain)
        if x_0 is not None:
            xv = x.view(B, self.seq_len, dn, nf)
            x0v = x_0.view(B, self.seq_len, dn, nf)
            xv[:, :, :, 4:6] = x0v[:, :, :, 0:2]
            width = 10
            wgt = torch.from_numpy(np.linspace(0, 1, width)).to(xv)[None, :, None, None]
            for j in FOOT_JOINTS:
                sl = slice(4 + 3 + (j - 1) * 6, 4 + 3 + j * 6)
                xv[:, 75:75 + width, :, sl] = wgt * x0v[:, 75:75 + width, :, sl] + (1 - wgt) * xv[:, 75:75 + width, :, sl]
                xv[:, 75 + width:-width, :, sl] = x0v[:, 75 + width:-width, :, sl]
                xv[:, 120 - width:120, :, sl] = (1 - wgt) * x0v[:, 120 - width:120, :, sl] + wgt * xv[:, 120 - width:120, :, sl]
            x = xv.reshape(B, Lq, nf)
        return x

    # ---- in-painting loops ---------------------------------------------------------------------------
    @torch.no_grad()
    def inpaint_loop(self, shape, cond, noise=None, constraint=None, return_diffusion=False, start_point=None, **kw):
        """DDPM loop with a hard constraint re-imposed after every step (reference model/diffusion.py:519-557)."""
        device = self._device()
        x = torch.randn(shape, device=device) if noise is None else noise.to(device)
        mask = constraint["mask"].to(device)
        value = constraint["value"].to(device)
        start_point = self.n_timestep if start_point is None else start_point
        tseq = list(reversed(range(0, start_point)))
        chain = [x] if return_diffusion else None

        q_noise = kw.get("q_noise")      # optional callable(t, shape): the randn_like q_sample draws in step t
        params = self._ddpm_params(tseq)
        cpar = torch.zeros(len(tseq), 8)
        sa, s1 = self.sqrt_alphas_cumprod.cpu(), self.sqrt_one_minus_alphas_cumprod.cpu()
        for i, tt in enumerate(tseq):    # x = q_sample(value, t - 1) * mask + (1 - mask) * x after every step with t > 0
            if tt > 0:
                cpar[i, 4], cpar[i, 5] = sa[tt - 1], s1[tt - 1]
                cpar[i, 7] = 2.0
        constrain = dict(kind=2, mask=mask.float().expand(shape).reshape(-1, shape[-1]), value=value.float().expand(shape),
                         q_noise=(lambda tt, sh: q_noise(tt, sh).to(device)) if q_noise is not None else None, params=cpar)
        out = self._run(L.SAMPLER_DDPM, tuple(shape), cond, x.float(), tseq, params, step_noise=kw.get("step_noise"),
                        seed=kw.get("seed"), collect=chain, constrain=constrain)
        return (out, chain) if return_diffusion else out

    @torch.no_grad()
    def long_inpaint_loop(self, shape, cond, noise=None, constraint=None, return_diffusion=False, start_point=None,
                          **kw):
        """DDPM loop over half-overlapping windows (reference model/diffusion.py:560-608)."""
        device = self._device()
        B, Lq, nf = shape
        x = torch.randn(shape, device=device) if noise is None else noise.to(device)
        assert x.shape[1] % 2 == 0
        if B == 1:
            return self.p_sample_loop(shape, cond, noise=noise, constraint=constraint,
                                      return_diffusion=return_diffusion, start_point=start_point, **kw)
        start_point = self.n_timestep if start_point is None else start_point
        tseq = list(reversed(range(0, start_point)))
        chain = [x] if return_diffusion else None

        params = self._ddpm_params(tseq)
        for i, tt in enumerate(tseq):
            params[i, 7] += 1.0 if tt > 0 else 0.0
        out = self._run(L.SAMPLER_DDPM, (B, Lq, nf), cond, x.float(), tseq, params, step_noise=kw.get("step_noise"),
                        seed=kw.get("seed"), collect=chain, couple=(Lq, nf))
        return (out, chain) if return_diffusion else out

    @torch.no_grad()
    def conditional_sample(self, shape, cond, constraint=None, *args, horizon=None, **kwargs):
        return self.p_sample_loop(shape, cond, *args, **kwargs)

    # ---- forward process -----------------------------------------------------------------------------
    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        return extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start + \
            extract(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise

    def noise_to_t(self, x, timestep):
        t = torch.full((len(x),), timestep, device=x.device).long()
        return self.q_sample(x, t) if timestep > 0 else x

    def partial_denoise(self, x, cond, t):
        return self.p_sample_loop(x.shape, cond, noise=self.noise_to_t(x, t), start_point=t)

    # ---- training loss (reference model/diffusion.py:636-753) ---------------------------------------------------------------
    def _skeleton(self, dev):
        from .fk import SMPLSkeleton
        smpl = self.smpl
        if smpl is None or not hasattr(smpl, "_parents"):
            smpl = self.__dict__.setdefault("_smpl_hip", SMPLSkeleton(dev))
        # the kernels take the skeleton as host lists: fetched ONCE per skeleton object, not with a device-to-host copy (a host wait for
        # the whole denoiser forward) in every training step.  Measured neutral at batch 32 -- the step is device-bound and the host
        # catches up during the backward (profiles/r06_train_skeleton_sync_ab.txt) -- kept because it is one sync less
        key = (id(smpl), smpl._offsets.data_ptr(), smpl._offsets._version)
        hit = self.__dict__.get("_skeleton_lists")
        if hit is None or hit[0] != key:
            hit = (key, [int(p) for p in smpl._parents], smpl._offsets.detach().cpu().tolist())
            self.__dict__["_skeleton_lists"] = hit
        return hit[1], hit[2]

    def p_losses(self, x_start, cond, t, trj_dist=None, *, noise=None, keep_mask=None):
        """The four-term training loss (reference model/diffusion.py:636-741): q_sample with the trajectory channels
        restored, one evaluation of the denoiser (keep mask ~ 1 - cond_drop_prob; dropout live in ``.train()`` mode), then
        reconstruction, velocity, SMPL-FK and foot-skate terms -- every stage a HIP kernel.  Returns
        ``(total, (recon, velocity, fk, foot))`` like the reference; with gradients enabled ``total`` carries an autograd
        graph of two nodes (loss terms, denoiser) whose backward passes are HIP kernels too (csrc/train_ops.hip,
        tcdiff_amd/train_engine.py), so ``TCDiff.train_loop`` (TCDiff.py:227-234) runs unchanged.
        Keyword-only extras inject the random draws (parity tests): ``noise`` in the permuted (b, S, dn, C) layout the
        reference draws it in, ``keep_mask`` (b,) bool; the dropout seed through ``self.model.train_seed``."""
        if trj_dist is not None:
            raise L.TcdiffError("trj_dist: the reference raises for any trj_dist (model/model.py:97,394: an [L, L] score bias added "
                                "to [L, S + 2] cross-attention scores); so does this build")
        dev = self._device()
        if dev.type != "cuda":
            raise L.TcdiffError("p_losses runs on MI355X only (no CPU fallback)")
        x_start = x_start.to(dev).float().contiguous()
        bs, dn, sq, c = x_start.shape
        t = t.to(dev).long().contiguous()
        if noise is None:
            noise = torch.randn(bs, sq, dn, c, device=dev)
        noise = noise.to(dev).float().contiguous()
        x_noisy = torch.empty(bs, sq * dn, c, device=dev)
        K.q_sample_traj(x_start, noise, t, self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, x_noisy, bs, dn,
                        sq, c)
        out = self.model(x_noisy, cond, t, cond_drop_prob=self.cond_drop_prob, keep_mask=keep_mask)
        parents, offsets = self._skeleton(dev)
        # the regression target (model/diffusion.py:657-660): x_start, or -- predict_epsilon -- the noise, which the reference
        # then also feeds to the velocity / FK / foot terms as if it were motion (:664-733); same here (dataset layout)
        target = noise.permute(0, 2, 1, 3).contiguous() if self.predict_epsilon else x_start
        total, terms = _LossFn.apply(out, target, t, self.p2_loss_weight, parents, offsets, self.loss_type == "l1")
        m = terms
        return total, (m[0], m[1], m[2], m[3])

    def loss(self, x, cond, t_override=None, trj_dist=None):
        batch_size = len(x)
        dev = self._device()
        if t_override is None:
            t = torch.randint(0, self.n_timestep, (batch_size,), device=dev).long()
        else:
            t = torch.full((batch_size,), t_override, device=dev).long()
        return self.p_losses(x, cond, t, trj_dist=trj_dist)

    def forward(self, x, cond, t_override=None, trj_dist=None):
        return self.loss(x, cond, t_override, trj_dist=trj_dist)

    # ---- render_sample: sampling and the fk_out pose export ----------------------------------------------------------
    body = None          # a BodyModel (tcdiff_amd/body.py load_body_model): render_sample's draw_out then shows the skinned bodies
    draw_format = "png"          # "avi": render_sample's draw_out writes Motion-JPEG AVI files (tcdiff_amd/video.py), with the clips' music if `sound`
    draw_audio_folder = None     # where the clips' .wav files are looked up by basename; None: beside the names
    foot_lock = False            # True: render_sample pins the planted feet (tcdiff_amd/footlock.py) before anything is written
    keep_apart = False           # True: render_sample shifts the roots so that the bodies do not touch (tcdiff_amd/apart.py); the order: see render_sample
    ground = False               # True / a number: render_sample then shifts the roots vertically onto the estimated / that floor (tcdiff_amd/ground.py)
    smooth = False               # True / an odd window: render_sample filters the jitter out of the exported poses (tcdiff_amd/smooth.py)
    beat_sync = False            # True: render_sample retimes the exported poses onto the music's beats, before the four above (tcdiff_amd/beat_sync.py)

    @torch.no_grad()
    def render_sample(self, shape, cond, normalizer=None, epoch=None, render_out=None, fk_out=None, name=None,
                      sound=True, mode="normal", noise=None, constraint=None, sound_folder="ood_sliced",
                      start_point=None, render=True, required_dancer_num=4, x_0=None, render_len=512, *, glb_out=None,
                      draw_out=None):
        """Mode dispatch of the reference (model/diffusion.py:784-806); a tensor ``shape`` is taken as the samples.

        With a ``normalizer`` and an ``fk_out`` directory, the post-processing of model/diffusion.py:811-988 follows:
        un-normalise, 6-D -> axis-angle, the window stitch in "long" mode, SMPL FK -- one HIP launch
        (tcdiff_amd/export.py) -- and the reference's pickles: one ``{epoch}_{num}_{clip}.pkl`` per clip in "normal",
        "inpaint" and "ctrl" mode, one ``{epoch}_{song}.pkl`` per song in "long" mode, each holding ``smpl_poses``,
        ``smpl_trans`` and ``full_pose``.

        With a ``normalizer`` and a ``draw_out`` directory (keyword only), what was exported is also drawn, on the device
        (tcdiff_amd/draw.py: the bones, floor trail and foot markers of ``skeleton_render``, vis.py:223-327, by a HIP
        rasteriser instead of matplotlib) and written as animated PNGs, clip by clip: ``e{epoch}_b{num}_{clip}.png`` per clip,
        or ``{epoch}_{song}.png`` of the song's first ``render_len`` frames in "long" mode -- the reference's names with the new
        extension.  An animated PNG has no sound: ``render_out``, ``sound``, ``sound_folder`` and ``render`` are unused with it, and
        without ``draw_out`` nothing is drawn.  With ``self.draw_format = "avi"`` (an attribute, "png" by default, for the reason
        given for ``body`` below) the files are Motion-JPEG AVI instead (tcdiff_amd/video.py), encoded on the device, and if
        ``sound`` is true each carries its clip's music as the reference finds it (``clip_audio``: the .wav beside each name, or in
        ``self.draw_audio_folder``; "long" mode stitches the windows' files); a .wav that does not exist raises before the
        sampler runs.  With ``self.body`` set to what ``load_body_model`` returns (an attribute, None by default: this
        method's parameter list is pinned by the tests, so the body is no keyword here), each clip's frames are the dancers'
        skinned, shaded bodies over that picture (tcdiff_amd/shade.py), skinned and drawn one clip at a time under the same file
        names; ``write_draw_out(..., body=, q=, pos=)`` is the keyword form.  Without ``draw_out`` the body changes nothing.

        With a ``normalizer`` and a ``glb_out`` directory (keyword only), the exported poses are also written as animated glTF
        files (tcdiff_amd/gltf.py: the open counterpart of the reference's Blender_Visulization/ FBX conversion), one per clip with
        all its dancers, under ``fk_out``'s names with the extension .glb.  The export runs once whichever of the three asks.
        Five correctors, each an attribute of this object (False by default; attributes for the same reason as ``body``), stand
        between the export and the writers.  Those that are on run once, in this one order, each on what the one before it returned,
        and every writer gets the last one's ``q``, ``pos``, joints and contacts; with all of them False nothing changes:
        1. ``self.beat_sync = True``: ``beat_sync`` (tcdiff_amd/beat_sync.py: a monotone time warp that brings the kinematic beats --
           the minima of the smoothed joint speed -- onto the music's beats, read from ``cond`` by ``beats_from_cond``; it needs
           ``cond``) retimes ``q``, ``pos``, the joints and the contacts, so that the filter takes out the kinks of the resampling;
        2. ``self.smooth = True``, or an odd integer, the window: ``smooth`` (tcdiff_amd/smooth.py: a Savitzky-Golay filter of the
           root positions and, through unit quaternions, of the rotations, against the frame-to-frame jitter of the sampler's
           independent rows) returns the filtered ``q``, ``pos`` and joints, so that the three below act on filtered joints;
        3. ``self.keep_apart = True``: ``keep_apart`` (tcdiff_amd/apart.py: the roots shifted horizontally so that the dancers'
           bodies do not touch) returns the shifted ``pos`` and joints; a shifted root slides a planted foot, and the lock re-pins it;
        4. ``self.ground = True``, or a number, the floor's height: ``ground`` (tcdiff_amd/ground.py: the roots shifted vertically
           so that the planted feet stand on the floor estimated from them and no part of a body sinks below it) returns the shifted
           ``pos`` and joints, so that the lock pins feet that already stand on the floor;
        5. ``self.foot_lock = True``: ``foot_lock`` (tcdiff_amd/footlock.py: the planted feet pinned, hip and knee re-solved)
           returns the locked ``q`` and joints.
        What each promises is measured on the end of the whole chain in tests/test_post_chain_gpu.py, on two seeded dances: every
        planted foot stays on its anchor, and against the raw export the frames with body contact, with a body below the floor and
        with a planted foot above it do not grow, the jitter and the mean acceleration fall and ``beat_align`` rises.  That is what
        is measured, not a guarantee: ``keep_apart``'s shift is found frame by frame, and a deep overlap of swinging arms raised the
        mean acceleration of the pushed dancers above the raw value (tests/test_post_chain_cpu.py).
        The samples are returned either way (the reference returns None)."""
        if self.draw_format not in ("png", "avi"):
            raise L.TcdiffError(f'render_sample: draw_format must be "png" or "avi", got {self.draw_format!r}')
        with_sound = normalizer is not None and draw_out is not None and self.draw_format == "avi" and bool(sound)
        if with_sound:
            from .video import clip_audio, clip_audio_paths
            clip_audio_paths(name, mode, self.draw_audio_folder)          # a missing .wav is an error before any sampling
        samples = self._render_samples(shape, cond, mode, noise, constraint, start_point, x_0)
        if normalizer is not None and (fk_out is not None or draw_out is not None or glb_out is not None):
            from .export import export_poses, write_fk_out
            x = samples if samples.is_cuda else samples.to(self._device())
            parents, offsets = self._skeleton(x.device)
            q, pos, poses, contacts = export_poses(x, normalizer, mode, required_dancer_num, parents=parents, offsets=offsets)
            if getattr(self, "beat_sync", False):          # before anything else: the filter and the correctors below act on the retimed motion
                from .beat_sync import beat_sync
                from .export import _is_long
                from .metrics import beats_from_cond
                if cond is None:
                    raise L.TcdiffError("render_sample: beat_sync reads the music's beats from cond, got None")
                beats = beats_from_cond(cond.to(x.device), poses.shape[2], long=_is_long(mode))
                synced = beat_sync(q, pos, beats, dn=int(required_dancer_num), contacts=contacts, parents=parents, offsets=offsets, measure=False)
                q, pos, poses, contacts = synced.q, synced.pos, synced.joints, synced.contacts
            smooth_by = getattr(self, "smooth", False)
            if smooth_by is not False and smooth_by is not None:          # before the three correctors below: they act on the filtered joints
                from .smooth import smooth
                kw = {} if smooth_by is True else dict(window=smooth_by)
                q, pos, poses = smooth(q, pos, dn=int(required_dancer_num), parents=parents, offsets=offsets, measure=False, **kw)[:3]
            if self.keep_apart:          # before the foot lock: a shifted root slides a planted foot, and the lock re-pins it
                from .apart import keep_apart
                pos, poses = keep_apart(pos, poses, dn=int(required_dancer_num), parents=parents)[:2]
            if self.ground is not False and self.ground is not None:          # after keep_apart, before the foot lock: the lock then pins feet on the floor
                from .ground import ground
                level = None if self.ground is True else self.ground
                pos, poses = ground(pos, poses, contacts, dn=int(required_dancer_num), floor=level, parents=parents)[:2]
            if self.foot_lock:
                from .footlock import foot_lock
                locked = foot_lock(q, pos, contacts, dn=int(required_dancer_num), parents=parents, offsets=offsets)
                q, poses = locked.q, locked.joints
            if fk_out is not None:
                write_fk_out(fk_out, mode, epoch, name, q, pos, poses)
            if glb_out is not None:
                from .gltf import write_glb_out
                write_glb_out(glb_out, mode, epoch, name, q, pos, required_dancer_num, parents=parents, offsets=offsets)
            if draw_out is not None:
                from .draw import write_draw_out
                kw = {} if self.body is None else dict(body=self.body, q=q, pos=pos)
                if self.draw_format == "avi":
                    kw.update(format="avi", audio=clip_audio(name, mode, self.draw_audio_folder, x.device) if with_sound else None)
                write_draw_out(draw_out, mode, epoch, name, poses, contacts, render_len=render_len, parents=parents, **kw)
        return samples

    def _render_samples(self, shape, cond, mode, noise, constraint, start_point, x_0):
        if isinstance(shape, tuple):
            if mode == "inpaint":
                fn = self.inpaint_loop
            elif mode == "normal":
                fn = self.ddim_sample
            elif mode == "long":
                fn = self.long_ddim_sample
            elif mode == "ctrl":
                fn = self.ddim_sample_Footwork
            else:
                assert False, "Unrecognized inference mode"
            if mode == "inpaint":
                return fn(shape, cond, noise=noise, constraint=constraint, start_point=start_point).detach().cpu()
            return fn(shape, cond, noise=noise, constraint=constraint, start_point=start_point, x_0=x_0).detach().cpu()
        return shape
