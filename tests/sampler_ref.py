"""A plain numpy reference of the sampler's per-step kernels (tcdiff_amd/csrc/ops.hip: tcdiff_sampler_update, tcdiff_sampler_constrain,
tcdiff_window_couple_step) -- what tests/test_sampler_kernels_f64_gpu.py holds them to.  No torch, no GPU.

  * philox4x32_10: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011) in exact integer
    arithmetic; tests/test_sampler_reference_cpu.py pins it to the Random123 known answers.
  * philox_normals: the keying include/tcdiff_hip.h documents -- counter = (tok * quads + quad, tseq[step], clip0 + row // L, stream
    word), key = (seed_lo ^ counter[1], seed_hi ^ counter[2]), stream word 0 for the step and 1 for the constraint -- and Box-Muller on
    the four words: (w0, w1) -> r(u0) cos / sin(2 pi u1) = elements 0, 1 of the quad, (w2, w3) -> elements 2, 3.  u and the angle are the
    kernel's float32 values bit for bit (they are IEEE operations); sqrt(-2 ln u), cos and sin are float64 of those float32 values
    (or float32 numpy, to measure what a float32 evaluation of the same expression loses: normals_floor).
  * Ref.update / Ref.constrain / Ref.couple: float64 evaluations of the fp32 inputs, written from the reference's lines (model/diffusion.py,
    cited at each expression).  Each returns the result and, per element, S = the sum of the absolute values of the terms it added (for
    DDIM after the division by params[2]) and r = the number of fp32 roundings on the longest path of the expression, so that
    |fp32 evaluation - float64| <= (r + 1) 2^-24 S to first order, whatever the association and with or without fma contraction.

The small methods of Ref (coef, clamp, predicts_eps, stream_word, token_clip) are the places a kernel can be wrong in; MUTANTS
overrides one each, and the CPU test shows that the GPU test's bounds tell every mutant from the reference on the GPU test's own inputs
(cases, update_cases, philox_cases: shared by both tests)."""
import itertools

import numpy as np

F64, F32 = np.float64, np.float32
U = 2.0 ** -24                       # unit roundoff of fp32, round to nearest
MASK = 0xFFFFFFFF
DDPM, DDIM = 0, 1                    # TC_SAMPLER_DDPM, TC_SAMPLER_DDIM

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
TWO_PI_F32 = F32(6.283185307179586)  # 6.2831855f


def philox4x32_10(counter, key, rounds=10):
    """counter: four, key: two uint32 values or arrays (broadcast against each other) -> the four output words (uint32 arrays)"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in key]
    m32, s32 = np.uint64(MASK), np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(PHILOX_M0) * c[0]                          # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(PHILOX_W0)) & m32, (k[1] + np.uint64(PHILOX_W1)) & m32]
    shape = np.broadcast(*c).shape
    return tuple(np.broadcast_to(v, shape).astype(np.uint32) for v in c)


def u01(w):
    """the kernel's float32 uniform of a 32-bit word: ((float)(w >> 8) + 0.5f) * 2^-24.  The sum rounds (ties to even) once
    w >> 8 >= 2^23, so u is exactly 1.0 for w >> 8 = 2^24 - 1 and never 0."""
    w = np.asarray(w, dtype=np.uint32)
    return ((w >> np.uint32(8)).astype(F32) + F32(0.5)) * F32(2.0 ** -24)


def normals_of_words(w, dtype=F64):
    """Box-Muller of four word arrays -> four arrays of normals: r(u0) cos a1, r(u0) sin a1, r(u2) cos a3, r(u2) sin a3 with
    u_i = u01(w_i) and a_i = 6.2831855f * u_i in float32; sqrt(-2 ln u), cos, sin and the products in `dtype`"""
    u = [u01(v) for v in w]
    a1, a3 = TWO_PI_F32 * u[1], TWO_PI_F32 * u[3]                  # float32 products
    assert a1.dtype == F32 and u[0].dtype == F32
    r0 = np.sqrt(dtype(-2.0) * np.log(u[0].astype(dtype)))
    r1 = np.sqrt(dtype(-2.0) * np.log(u[2].astype(dtype)))
    a1, a3 = a1.astype(dtype), a3.astype(dtype)
    return r0 * np.cos(a1), r0 * np.sin(a1), r1 * np.cos(a3), r1 * np.sin(a3)


def _token_clip(row, L, clip0):
    return row % L, clip0 + row // L


def philox_normals(n_rows, nfeat, L, t, seed=0, dev=(0, 0), clip0=0, stream=0, dtype=F64, token_clip=_token_clip):
    """the [n_rows][nfeat] normals of a launch at timestep t = tseq[step]: seed is the by-value 64-bit seed, dev the device seed
    words counter[1], counter[2] (int32, may be negative), stream 0 for the step's noise and 1 for the constraint's"""
    quads = (nfeat + 3) // 4
    row = np.arange(n_rows, dtype=np.int64)
    tok, clip = token_clip(row, L, clip0)
    c0 = (tok[:, None] * quads + np.arange(quads, dtype=np.int64)[None, :]) & MASK
    c2 = np.broadcast_to((clip & MASK)[:, None], c0.shape)
    k0 = (int(seed) & MASK) ^ (int(dev[0]) & MASK)
    k1 = ((int(seed) >> 32) & MASK) ^ (int(dev[1]) & MASK)
    w = philox4x32_10((c0, int(t) & MASK, c2, int(stream)), (k0, k1))
    z = np.stack(normals_of_words(w, dtype), axis=-1)             # [n_rows][quads][4]
    return z.reshape(n_rows, quads * 4)[:, :nfeat]


class Ref:
    """float64 evaluations of the three kernels on fp32 inputs; see the module docstring for S and r"""

    # ---- the places a kernel can go wrong in (MUTANTS override one each) ---------------------------------------------------------
    def coef(self, pr):
        return pr

    def clamp(self, g):
        return np.clip(g, -1.0, 1.0)

    def predicts_eps(self, flags):
        return bool(flags & 4)

    def stream_word(self, constraint):
        return 1 if constraint else 0

    token_clip = staticmethod(_token_clip)

    def normals(self, shape, noise, constraint, dtype=F64):
        """noise = dict(L, t, seed, dev, clip0): the launch's Philox normals"""
        return philox_normals(shape[0], shape[1], noise["L"], noise["t"], noise.get("seed", 0), noise.get("dev", (0, 0)),
                              noise.get("clip0", 0), self.stream_word(constraint), dtype, self.token_clip)

    # ---- tcdiff_sampler_update ----------------------------------------------------------------------------------------------------
    def update(self, mode, unc, cond, x, pr, eps=None, traj=None, noise=None):
        """unc (or None), cond: [rows][>= nfeat] network outputs; x, eps: [rows][nfeat]; pr: the step's 8 scalars; traj [rows][3] or None;
        eps None -> Philox normals of `noise`.  Returns x, x0, their S and r (S_x0, r_x0 for x0), bound / bound_x0 = (r + 1) 2^-24 S, and
        noise_coef = |the scalar that multiplies eps|."""
        x = np.asarray(x, F64)
        nf = x.shape[1]
        pr = self.coef(np.asarray(pr, F64))
        w, flags = pr[0], int(pr[7])
        cond = np.asarray(cond, F64)[:, :nf]
        e = self.normals(x.shape, noise, False) if eps is None else np.asarray(eps, F64)
        if unc is not None:
            unc = np.asarray(unc, F64)[:, :nf]
            out = unc + (cond - unc) * w                              # model/model.py:546 (guided_forward)
            S0 = np.abs(unc) + (np.abs(cond) + np.abs(unc)) * abs(w)
            r0 = 3                                                    # difference, product, sum
        else:
            out, S0, r0 = cond, np.abs(cond), 0                       # weight 1: the conditional output itself
        if mode == DDPM and self.predicts_eps(flags):
            # model/diffusion.py:181-185 (predict_start_from_noise); DDPM only: model_predictions (:195-204) takes the output as x_0
            out = pr[4] * x - pr[5] * out
            S0 = np.abs(pr[4] * x) + abs(pr[5]) * S0
            r0 += 2                                                   # the product with the network output, the difference
        x0 = out if flags & 8 else self.clamp(out)                    # :230-231 / :198-201; 1-Lipschitz, no rounding of its own
        if mode == DDPM:
            xn = pr[1] * x0 + pr[2] * x + pr[3] * e                   # :207-210 (q_posterior mean), :251 (sigma = 0 at t = 0)
            S = abs(pr[1]) * S0 + np.abs(pr[2] * x) + np.abs(pr[3] * e)
            r = r0 + 3                                                # coef1 * x0, two sums
            ncoef = abs(pr[3])
        elif pr[6] != 0.0:
            xn, S, r, ncoef = x0, S0, r0, 0.0                         # :411-413 (time_next < 0: x = x_start)
        else:
            pn = (pr[1] * x - x0) / pr[2]                             # :189-193 (predict_noise_from_start)
            Sp = (np.abs(pr[1] * x) + S0) / abs(pr[2])
            xn = x0 * pr[3] + pr[4] * pn + pr[5] * e                  # :423-425
            S = abs(pr[3]) * S0 + abs(pr[4]) * Sp + np.abs(pr[5] * e)
            r = r0 + 5                                                # x0 -> difference, quotient, product with c, two sums
            ncoef = abs(pr[5])
        xn, S = np.array(xn), np.array(S)
        if traj is not None:
            c = min(nf, 6)
            if c > 4:
                xn[:, 4:c] = np.asarray(traj, F64)[:, :c - 4]         # :427-431: a copy, exact
                S[:, 4:c] = 0.0
        return dict(x=xn, x0=x0, S=S, r=r, S_x0=S0, r_x0=r0, bound=(r + 1) * U * S, bound_x0=(r0 + 1) * U * S0, noise_coef=ncoef)

    # ---- tcdiff_sampler_constrain -------------------------------------------------------------------------------------------------
    def constrain(self, kind, x, mask, value, pr, q_eps=None, noise=None):
        """mask [mask_rows][nfeat] serves row % mask_rows; the step is enabled by bit 1 of pr[7]"""
        x, value = np.asarray(x, F64), np.asarray(value, F64)
        pr = self.coef(np.asarray(pr, F64))
        mask = np.asarray(mask, F64)
        m = mask[np.arange(x.shape[0]) % mask.shape[0]]
        if not int(pr[7]) & 2:
            return dict(x=x.copy(), S=np.abs(x), r=0, bound=np.zeros_like(x), noise_coef=0.0)
        if kind == 1:                                                 # :341-356: x[mask] = value[mask], a copy
            return dict(x=np.where(m != 0.0, value, x), S=np.zeros_like(x), r=0, bound=np.zeros_like(x), noise_coef=0.0)
        e = self.normals(x.shape, noise, True) if q_eps is None else np.asarray(q_eps, F64)
        qs = pr[4] * value + pr[5] * e                                # :625-634 (q_sample at t - 1: the host puts its scalars here)
        xn = qs * m + (1.0 - m) * x                                   # :545-551
        S = np.abs(m) * (np.abs(pr[4] * value) + np.abs(pr[5] * e)) + (1.0 + np.abs(m)) * np.abs(x)
        r = 4                                                         # product, sum (q_sample); product with the mask, sum
        return dict(x=xn, S=S, r=r, bound=(r + 1) * U * S, noise_coef=abs(pr[5]) * np.abs(m))

    # ---- tcdiff_window_couple_step ------------------------------------------------------------------------------------------------
    def couple(self, x, b, seq_len, pr):
        """:502-506 on the (b, seq_len, row_elems) view, after the steps whose pr[7] has bit 0 set"""
        x = np.array(x)
        if not int(pr[7]) & 1 or b == 1:
            return x
        v = x.reshape(b, seq_len, -1)
        out = v.copy()
        out[1:, :seq_len // 2] = v[:-1, seq_len // 2:]
        return out.reshape(x.shape)


# ---- emulated defects: each a copy of the reference with one place changed ------------------------------------------------------
class SwapCoefs(Ref):
    def coef(self, pr):
        pr = pr.copy()
        pr[1], pr[2] = pr[2], pr[1]
        return pr


class NoClamp(Ref):
    def clamp(self, g):
        return g


class IgnoreBit2(Ref):
    def predicts_eps(self, flags):
        return False


class StepStreamForConstraint(Ref):
    def stream_word(self, constraint):
        return 0


class KeyedByRow(Ref):
    @staticmethod
    def token_clip(row, L, clip0):
        return row, np.full_like(row, clip0)


MUTANTS = {"swap_params_1_2": SwapCoefs, "no_clamp": NoClamp, "ignore_bit2": IgnoreBit2, "constraint_stream0": StepStreamForConstraint,
           "keyed_by_row": KeyedByRow}


# ---- the GPU test's inputs (the CPU test shows on the same that the bounds separate the mutants) ---------------------------------
L_SEQ, CLIPS = 6, 3
ROWS = L_SEQ * CLIPS                       # 18 rows: at nfeat = 151, 684 threads = two full blocks and a ragged third
NFEATS = (151, 5, 4, 1)                    # 38 quads with a last quad 3 wide; one quad + one element; exactly one quad; one element
TSEQ = (999, 0, 417)
SEED = 0x9E3779B97F4A7C15                  # both 32-bit halves nonzero
DEV_WORDS = (0x01234567, -5)               # device seed words; the second is negative as an int32


def ldos(nfeat):
    return (nfeat, 152, 160)


def cases(nfeat, ldo=None):
    """fp32 inputs of one shape.  The network outputs hold exactly +-1, their neighbours and values beyond (unc == cond there, so that
    the guided output is that value exactly); columns nfeat.. of the [rows][ldo] outputs hold 1e6 (never to be read)."""
    ldo = nfeat if ldo is None else ldo
    g = np.random.default_rng(1000 + nfeat)
    rn = lambda *s, scale=1.0: (g.standard_normal(s) * scale).astype(F32)      # noqa: E731
    cond, unc = np.full((ROWS, ldo), 1e6, F32), np.full((ROWS, ldo), 1e6, F32)
    cond[:, :nfeat], unc[:, :nfeat] = rn(ROWS, nfeat, scale=0.8), rn(ROWS, nfeat, scale=0.8)
    edge = np.array([1.0, -1.0, np.nextafter(F32(1), F32(2)), np.nextafter(F32(1), F32(0)), np.nextafter(F32(-1), F32(-2)),
                     np.nextafter(F32(-1), F32(0)), 1.5, -2.25, 3.0, 0.0], F32)
    flat = np.arange(ROWS * nfeat)
    pick = flat[::max(1, (ROWS * nfeat) // 40)][:40]
    for j, i in enumerate(pick):
        cond[i // nfeat, i % nfeat] = unc[i // nfeat, i % nfeat] = edge[j % len(edge)]
    # masks 0, 0.25 and 1, all three in every L rows at every width (a 1-wide row included)
    mask = np.array([0.0, 0.25, 1.0], F32)[((flat + flat // 3) % 3).reshape(ROWS, nfeat)]
    return dict(nfeat=nfeat, ldo=ldo, cond=cond, unc=unc, x=rn(ROWS, nfeat), eps=rn(ROWS, nfeat), traj=rn(ROWS, 3),
                value=rn(ROWS, nfeat, scale=0.7), q_eps=rn(ROWS, nfeat), mask=mask, mask_L=mask[L_SEQ:2 * L_SEQ].copy())


def params(flags, step, last=False):
    """three rows of step scalars, all different; row `step` carries `flags` in column 7 (with bits 0 and 1, which the update must
    ignore, set at step 2), the other rows the opposite of bits 2 and 3"""
    p = np.array([[2.0, 0.31, 0.62, 0.21, 1.05, 0.33, 0.0, 0.0],
                  [0.5, 0.11, 0.87, 0.45, 1.40, 0.90, 0.0, 0.0],
                  [1.7, 0.93, 0.27, 0.58, 0.71, 0.14, 0.0, 0.0]], F32)
    p[:, 7] = (flags ^ 12)
    p[step, 7] = flags + (3 if step == 2 else 0)
    if last:
        p[step, 6] = 1.0
    return p


def noise_params():
    """step scalars under which a launch on x = 0 returns its noise: the DDPM update's (., 0, 0, 1) and, for the kind-2 constraint on
    value 0 under mask 1, params[5] = 1 with bit 1 of column 7"""
    return np.array([[2.0, 0.0, 0.0, 1.0, 0.9, 1.0, 0.0, 2.0],
                     [0.5, 0.0, 0.0, 1.0, 0.4, 1.0, 0.0, 2.0],
                     [1.7, 0.0, 0.0, 1.0, 0.6, 1.0, 0.0, 2.0]], F32)


def update_cases():
    """every form the engine can launch: mode x unconditional branch x flags x step, then DDIM's last step"""
    for mode, with_unc, flags, step in itertools.product((DDPM, DDIM), (True, False), (0, 4, 8, 12), (0, 2)):
        yield dict(mode=mode, with_unc=with_unc, flags=flags, step=step, last=False)
    for with_unc, flags in itertools.product((True, False), (0, 8)):
        yield dict(mode=DDIM, with_unc=with_unc, flags=flags, step=2, last=True)


def philox_cases():
    """(nfeat, step, clip0, seed, device words) of the launches whose output is the kernel's noise"""
    out = []
    for nfeat in NFEATS:
        for step, clip0 in itertools.product((0, 1), (0, 2 ** 20 + 3)):                 # timesteps 999 and 0
            out.append(dict(nfeat=nfeat, step=step, clip0=clip0, seed=SEED, dev=DEV_WORDS))
        out.append(dict(nfeat=nfeat, step=2, clip0=5, seed=0, dev=(0, 0)))
    return out


def noise_of(case):
    return dict(L=L_SEQ, t=TSEQ[case["step"]], seed=case["seed"], dev=case["dev"], clip0=case["clip0"])


def normals_floor():
    """(what a float32 numpy evaluation of the normals loses against float64 on the GPU test's own counters, both stream words: the
    maximum absolute difference; the largest |z|; the number of draws)"""
    worst, top, n = 0.0, 0.0, 0
    ref = Ref()
    for c in philox_cases():
        for constraint in (False, True):
            z64 = ref.normals((ROWS, c["nfeat"]), noise_of(c), constraint, F64)
            z32 = ref.normals((ROWS, c["nfeat"]), noise_of(c), constraint, F32)
            assert z32.dtype == F32
            worst = max(worst, float(np.abs(z32.astype(F64) - z64).max()))
            top = max(top, float(np.abs(z64).max()))
            n += z64.size
    return worst, top, n


def normals_bound():
    """8 x the measured floor, absolute: the device's logf / sincosf may each be a few ulp off where numpy's are (nearly) correctly
    rounded; a wrong bit anywhere in the generator moves a normal by order 1"""
    return 8.0 * normals_floor()[0]
