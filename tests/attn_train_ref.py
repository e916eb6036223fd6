"""Train-mode attention, forward and backward, in float64: the reference that tcdiff_attention_train and tcdiff_attention_bwd
(csrc/attention_train.hip, the TRAIN half of csrc/attn_res.h) are held to, region by region, by tests/test_attn_train_f64_gpu.py;
pinned to torch autograd in float64 and to bf16_ref's attention model by tests/test_attn_train_reference_cpu.py.

Inputs are the operand VALUES as stored: the Q' image (already times 1/8), K, V, dO as [n_seq, H, L, 64], the keep mask
oracle.dropout_keep(seed, site, (n_seq * H, Lq, Lk), p) (class Keep) and the fp32 scale of kernels.drop_params.

``Ref(rounding=False)`` is plain float64:
    S = Q' K^T, P = softmax(S), Pd = keep P scale, O = Pd V, lse = log2 sum 2^(S log2e), delta = sum_d dO O, dV = Pd^T dO,
    dS = P o (keep scale (dO V^T) - delta), dQ = scale_q dS K, dK = dS^T Q'.
``Ref(rounding=True)`` rounds to bf16 (x3_ref.bf16_rne) exactly where the bf16 kernels hand a value on, and nowhere else:

  * forward (attention_train_kernel, attention_res_kernel<NG, true>): keys in tiles of 64 (the resident kernel: chunks of 512 keys
    in 64-key tiles -- the same walk), the running maximum in the exp2 domain, p = exp2(fma(s, log2e, -m_new)), the denominator
    summed from the UNROUNDED, UNDROPPED p, the dropped, scaled, still unnormalised p rounded in front of P V, the accumulator
    rescaled by exp2(m_run - m_new), 1 / l last, then the bf16 store; O_lo = bf16(o - float(bf16(o))); lse = m + log2(l);
  * backward: delta from the STORED dO and O (+ O_lo); P = exp2(fma(s, log2e, -lse)) from the stored fp32 lse; the dq kernels round
    dS in front of dS K and store dQ = bf16(scale_q acc); the dkv kernels round Pd and dS in front of their products and store bf16.

The f32 kernels round nothing: their model is float64.  ``standin()`` is the same arithmetic in float32 torch on the CPU with
torch's bf16 casts at those points.  ``defect`` emulates a kernel defect (DEFECTS).  The launcher's selection predicates are
restated below from the CU count, and the GPU module's cases, inputs and BOUNDS are defined here so that the CPU module runs the
reference and the stand-in on exactly them.  Not a test module: no test_* name, nothing collected here."""
import math

import numpy as np
import torch

from bf16_ref import bf, bf16_rne, bf16_trunc, region_stats, rnd, round_up  # noqa: F401  (re-exported to the test modules)
from layer_ref import LOG2E

D = torch.float64
TILE, CHUNK = 64, 512
LN2 = math.log(2.0)
SEED = (1234, 5678)

DEFECTS = (
    "mask_off_by_one",      # key Lk takes part in the softmax
    "p_trunc",              # the dropped P truncated to bf16 instead of rounded in front of P V
    "denom_after_dropout",  # the softmax denominator summed from the dropped, scaled p
    "keep_stride_lpk",      # the keep bit's flat index with Lp_k as its row stride in place of Lk (forward and backward)
    "bwd_keep_group_shift", # the backward's keep bit taken one 32-row group further down
    "no_rescale_chunk",     # no rescale of the accumulator in the first tile of a second 512-key chunk
    "lse_natural",          # lse stored as a natural logarithm
    "no_scale_q",           # scale_q missing from dQ
    "delta_no_lo",          # delta from O alone although O_lo was given
)

# Bounds (tests/test_attn_train_f64_gpu.py): (max, mean) of |kernel - reference| / max |reference| per region, for (output, kind,
# against).  "model": Ref(rounding=True); "f64": Ref(rounding=False) on the same operand values.  A "_big" output is that of a
# gain-4 case (logits in the hundreds, nearly one-hot rows).  Set from the MI355X run recorded in profiles/attn_train_f64.txt at 4x
# the worst value observed over the output's cases and regions (in brackets: max / mean), with the two figures of bf16_ref.BOUNDS
# that are not measurements: the MAX of a bf16 store against the model is ONE_ULP = 2^-7 wherever a flip was seen (the mean is the
# sharp statistic), and an f32 output against float64 stays under 1e-5.  O + O_lo is a 16-bit value, not a bf16 store: its max is
# measured.  The worst means come from the smallest (sequence, head) blocks (33 keys x 64: a handful of flips); one entry is 4x the
# float32 stand-in's mean where 4x the kernels' own is less than the stand-in's flips cost, marked [stand-in] as in bf16_ref.
# lse and delta are fp32 statistics: their model is float64 of the same operands and both entries are equal.
ONE_ULP = 2.0 ** -7
BOUNDS = {
    ("O", "f32", "model"):             (3.2e-06, 2.0e-07),    # [7.8e-07 / 4.8e-08]
    ("O", "f32", "f64"):               (3.2e-06, 2.0e-07),    # [7.8e-07 / 4.8e-08]
    ("O", "bf16", "model"):            (ONE_ULP, 2.9e-06),    # [2.4e-03 / 7.2e-07]
    ("O", "bf16", "f64"):              (1.8e-02, 2.4e-03),    # [4.4e-03 / 6.0e-04]
    ("O_big", "bf16", "model"):        (ONE_ULP, 4.1e-06),    # [1.8e-03 / 1.0e-06]
    ("O_big", "bf16", "f64"):          (2.0e-02, 1.3e-03),    # [4.8e-03 / 3.1e-04]
    ("O+O_lo", "bf16", "model"):       (4.4e-03, 2.8e-06),    # [1.1e-03 / 6.8e-07]
    ("O+O_lo", "bf16", "f64"):         (6.7e-03, 1.9e-03),    # [1.7e-03 / 4.7e-04]
    ("O+O_lo_big", "bf16", "model"):   (8.1e-04, 7.8e-07),    # [2.0e-04 / 2.0e-07]
    ("O+O_lo_big", "bf16", "f64"):     (6.3e-03, 1.1e-03),    # [1.6e-03 / 2.6e-04]
    ("lse", "f32", "model"):           (8.9e-07, 3.7e-07),    # [2.2e-07 / 9.3e-08]
    ("lse", "f32", "f64"):             (8.9e-07, 3.7e-07),    # [2.2e-07 / 9.3e-08]
    ("lse", "bf16", "model"):          (6.4e-07, 9.8e-08),    # [1.6e-07 / 2.4e-08]
    ("lse", "bf16", "f64"):            (6.4e-07, 9.8e-08),    # [1.6e-07 / 2.4e-08]
    ("lse_big", "bf16", "model"):      (2.0e-07, 2.4e-08),    # [4.9e-08 / 5.8e-09]
    ("lse_big", "bf16", "f64"):        (2.0e-07, 2.4e-08),    # [4.9e-08 / 5.8e-09]
    ("delta", "f32", "model"):         (4.4e-07, 9.0e-08),    # [1.1e-07 / 2.2e-08]
    ("delta", "f32", "f64"):           (4.4e-07, 9.0e-08),    # [1.1e-07 / 2.2e-08]
    ("delta", "bf16", "model"):        (4.6e-07, 1.6e-07),    # [1.1e-07 / 3.8e-08]
    ("delta", "bf16", "f64"):          (4.6e-07, 1.6e-07),    # [1.1e-07 / 3.8e-08]
    ("delta_big", "bf16", "model"):    (3.3e-07, 4.7e-08),    # [8.2e-08 / 1.2e-08]
    ("delta_big", "bf16", "f64"):      (3.3e-07, 4.7e-08),    # [8.2e-08 / 1.2e-08]
    ("dQ", "f32", "model"):            (6.2e-06, 2.9e-07),    # [1.5e-06 / 7.1e-08]
    ("dQ", "f32", "f64"):              (6.2e-06, 2.9e-07),    # [1.5e-06 / 7.1e-08]
    ("dQ", "bf16", "model"):           (ONE_ULP, 2.0e-05),    # [3.0e-03 / 4.9e-06]
    ("dQ", "bf16", "f64"):             (2.3e-02, 9.1e-04),    # [5.6e-03 / 2.3e-04]
    ("dQ_big", "bf16", "model"):       (ONE_ULP, 5.4e-07),    # [1.9e-04 / 2.0e-08]  [stand-in mean 1.33e-07]
    ("dQ_big", "bf16", "f64"):         (1.5e-02, 2.9e-04),    # [3.7e-03 / 7.1e-05]
    ("dK", "f32", "model"):            (4.6e-06, 2.7e-07),    # [1.2e-06 / 6.6e-08]
    ("dK", "f32", "f64"):              (4.6e-06, 2.7e-07),    # [1.2e-06 / 6.6e-08]
    ("dK", "bf16", "model"):           (ONE_ULP, 2.8e-05),    # [2.6e-03 / 7.0e-06]
    ("dK", "bf16", "f64"):             (1.8e-02, 1.7e-03),    # [4.3e-03 / 4.1e-04]
    ("dK_big", "bf16", "model"):       (ONE_ULP, 5.0e-07),    # [4.3e-04 / 1.2e-07]
    ("dK_big", "bf16", "f64"):         (1.5e-02, 7.0e-04),    # [3.7e-03 / 1.7e-04]
    ("dV", "f32", "model"):            (5.5e-06, 3.0e-07),    # [1.4e-06 / 7.4e-08]
    ("dV", "f32", "f64"):              (5.5e-06, 3.0e-07),    # [1.4e-06 / 7.4e-08]
    ("dV", "bf16", "model"):           (ONE_ULP, 2.8e-05),    # [3.1e-03 / 6.9e-06]
    ("dV", "bf16", "f64"):             (1.8e-02, 2.3e-03),    # [4.3e-03 / 5.7e-04]
    ("dV_big", "bf16", "model"):       (ONE_ULP, 3.5e-07),    # [7.5e-04 / 8.5e-08]
    ("dV_big", "bf16", "f64"):         (1.4e-02, 5.0e-04),    # [3.4e-03 / 1.2e-04]
}
OUTPUTS = ("O", "O+O_lo", "lse", "delta", "dQ", "dK", "dV")
# the existing whole-tensor Frobenius bounds of tests/test_train_kernels_gpu.py, which the new cases must also meet: (O, gradients)
FROBENIUS = {"bf16": (1.5e-2, 2.25e-2), "f32": (3e-6, 1e-5)}


# ---- the keep mask --------------------------------------------------------------------------------------------------------------------
class Keep:
    """the keep bits of one attention launch: element (bh, q, k) of the [n_seq * H, Lq, Lk] weights tensor has the flat index
    (bh Lq + q) Lk + k in the oracle's counter hash.  p = 0: no mask.  `fixed`: a given [n, H, Lq, Lk] bool tensor (probes)."""

    def __init__(self, site, n, H, Lq, Lk, p, *, Lp_k=None, seed=SEED, fixed=None):
        self.site, self.n, self.H, self.Lq, self.Lk, self.p, self.Lp_k, self.seed, self.fixed = site, n, H, Lq, Lk, p, Lp_k, seed, fixed
        self._memo = {}

    @property
    def scale(self):
        """the fp32 scale the kernels multiply by (kernels.drop_params passes 1 / (1 - p) as a C float)"""
        return float(np.float32(1.0 / (1.0 - self.p))) if self.p > 0 else 1.0

    def mask(self, defect=None):
        if self.fixed is not None:
            return self.fixed
        if self.p <= 0:
            return None
        if defect not in self._memo:
            from oracle import tcdiff_oracle as O
            n, H, Lq, Lk = self.n, self.H, self.Lq, self.Lk
            if defect == "keep_stride_lpk":
                m = O.dropout_keep(self.seed, self.site, (n * H * Lq, self.Lp_k), self.p)[:, :Lk]
            elif defect == "bwd_keep_group_shift":
                m = O.dropout_keep(self.seed, self.site, (n * H * Lq + 32, Lk), self.p)[32:]
            else:
                m = O.dropout_keep(self.seed, self.site, (n * H, Lq, Lk), self.p)
            self._memo[defect] = m.reshape(n, H, Lq, Lk)
        return self._memo[defect]


def tok(t):
    """head-major [n, H, L, 64] -> token-major [n L, H 64]"""
    n, H, Lx, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(n * Lx, H * 64)


def heads(t, n, H):
    """token-major [n L, H 64] -> head-major [n, H, L, 64]"""
    return t.reshape(n, -1, H, 64).permute(0, 2, 1, 3)


class Ref:
    def __init__(self, rounding=True, defect=None, dtype=D):
        if defect is not None and defect not in DEFECTS:
            raise ValueError(defect)
        self.rounding, self.defect, self.D = rounding, defect, dtype
        self.fused = dtype != D      # the stand-in: the kernels' x = fma(s, log2e, -m), one rounding; m = fp32(max s * log2e)

    def c(self, t):
        return torch.as_tensor(t).detach().cpu().to(self.D)

    def rb(self, v, trunc=False):
        """a bf16 hand-off of the kernel's fp32 value; identity without rounding"""
        if not self.rounding:
            return v
        if self.D != D:
            return v.to(torch.float32).to(torch.bfloat16).to(self.D)
        f = v.to(torch.float32)
        return torch.from_numpy((bf16_trunc if trunc else bf16_rne)(f).reshape(tuple(f.shape))).to(self.D)

    def _keepf(self, keep, defects, shape, nk=None):
        m = keep.mask(self.defect if self.defect in defects else None)
        if m is None:
            return torch.ones(shape, dtype=self.D), 1.0
        m = m.to(self.D)
        if nk is not None and nk > m.shape[-1]:
            m = torch.cat([m, torch.ones(*m.shape[:-1], nk - m.shape[-1], dtype=self.D)], -1)
        return m, keep.scale

    def _exp2(self, s, m):
        """exp2(fma(s, log2e, -m)): the stand-in evaluates the fused exponent in double and rounds once"""
        if self.fused:
            return torch.exp2((s.double() * LOG2E - m.double()).to(self.D))
        return torch.exp2(s * LOG2E - m)

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    def fwd(self, q, k, v, keep, Lk, *, tile=TILE, chunk=CHUNK):
        """q [n, H, Lq, 64], k / v [n, H, >= Lk, 64] (padding rows included) -> head-major o (the fp32 value in front of the store),
        O, O_lo, O+O_lo [n, H, Lq, 64] and lse [n, H, Lq]"""
        q = self.c(q)
        n, H, Lq = q.shape[:3]
        nk = Lk + 1 if self.defect == "mask_off_by_one" and k.shape[2] > Lk else Lk
        kk, vv = self.c(k)[:, :, :nk], self.c(v)[:, :, :nk]
        kf, sc = self._keepf(keep, ("keep_stride_lpk",), (n, H, Lq, nk), nk)
        s_all = q @ kk.transpose(-1, -2)
        m = torch.full((n, H, Lq, 1), -math.inf, dtype=self.D)
        l = torch.zeros(n, H, Lq, 1, dtype=self.D)
        o = torch.zeros(n, H, Lq, 64, dtype=self.D)
        for t0 in range(0, nk, tile):
            s = s_all[..., t0:t0 + tile]
            m_new = torch.maximum(m, s.amax(-1, keepdim=True) * torch.tensor(LOG2E, dtype=self.D))
            p = self._exp2(s, m_new)
            pd = p * kf[..., t0:t0 + tile] * sc
            alpha = torch.exp2(m - m_new)
            l = l * alpha + (pd if self.defect == "denom_after_dropout" else p).sum(-1, keepdim=True)
            if not (self.defect == "no_rescale_chunk" and t0 > 0 and t0 % chunk == 0):
                o = o * alpha
            o = o + self.rb(pd, trunc=self.defect == "p_trunc") @ vv[..., t0:t0 + tile, :]
            m = m_new
        o = o / l
        lse = (m + torch.log2(l)).squeeze(-1)
        if self.defect == "lse_natural":
            lse = lse * LN2
        O = self.rb(o)
        O_lo = self.rb(o - O)
        return {"o": o, "O": O, "O_lo": O_lo, "O+O_lo": O + O_lo, "lse": lse}

    # ---- backward --------------------------------------------------------------------------------------------------------------
    def bwd(self, q, k, v, dO, O, O_lo, lse, keep, Lk, scale_q=0.125):
        """q, dO, O, O_lo (or None) [n, H, Lq, 64], k / v [n, H, >= Lk, 64], lse [n, H, Lq] as stored -> delta [n, H, Lq] and
        head-major dQ [n, H, Lq, 64], dK, dV [n, H, Lk, 64]"""
        q, dO, O = self.c(q), self.c(dO), self.c(O)
        n, H, Lq = q.shape[:3]
        kk, vv = self.c(k)[:, :, :Lk], self.c(v)[:, :, :Lk]
        if O_lo is not None and self.defect != "delta_no_lo":
            O = O + self.c(O_lo)
        delta = (dO * O).sum(-1)
        kf, sc = self._keepf(keep, ("keep_stride_lpk", "bwd_keep_group_shift"), (n, H, Lq, Lk))
        P = self._exp2(q @ kk.transpose(-1, -2), self.c(lse).unsqueeze(-1))
        g = kf * sc * (dO @ vv.transpose(-1, -2))
        dS = self.rb(P * (g - delta.unsqueeze(-1)))
        Pd = self.rb(P * kf * sc)
        dQ = dS @ kk
        if self.defect != "no_scale_q":
            dQ = dQ * scale_q
        return {"delta": delta, "dQ": self.rb(dQ), "dK": self.rb(dS.transpose(-1, -2) @ q), "dV": self.rb(Pd.transpose(-1, -2) @ dO)}


def standin(defect=None):
    """the bf16 kernels' arithmetic in float32 torch on the CPU"""
    return Ref(True, defect, dtype=torch.float32)


# ---- kernel selection, restated from the launchers (csrc/attention_train.hip) -------------------------------------------------------
def resident_fwd(kind, Lp_q, ldo):
    return kind == "bf16" and Lp_q >= 512 and ldo % 8 == 0


def resident_fwd_ng(Lq, H, n_seq, n_cu):
    """row groups per wave of attention_res_kernel<NG, true>: 1 while a workgroup per 256 query rows fits one wave of the chip"""
    return 1 if -(-Lq // 256) * H * n_seq <= n_cu else 2


def resident_bwd(kind, Lq, Lk, ld_dq=1536, ld_dkv=1024):
    return kind == "bf16" and 256 <= Lq <= 512 and Lk <= 512 and ld_dq % 8 == 0 and ld_dkv % 8 == 0


def last_tile_ns(Lk):
    """32-key halves the resident forward runs in the last tile of the last chunk (NS = 1: at most 32 keys left)"""
    left = Lk - (Lk - 1) // 64 * 64
    return 1 if left <= 32 else 2


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def case(Lq, Lk, kind="bf16", *, n=2, H=8, p=0.0, gain=1, vshift=0.0, ldo=None, Lp_k=None, want=None, olo=True, name=None):
    """want: the kernel family the case is meant to reach ("res1" / "res2" / "stream" for a forward case, "res" / "stream" for a
    backward one); n = 0 stands for n_cu // 16 + 1 sequences"""
    return dict(Lq=Lq, Lk=Lk, kind=kind, n=n, H=H, p=p, gain=gain, vshift=vshift, ldo=ldo or 64 * H + 8, Lp_k=Lp_k, want=want, olo=olo,
                name=name)


def case_id(c):
    s = f"{c['Lq']}x{c['Lk']}-{c['kind']}-p{c['p']}"
    s += f"-n{c['n'] or 'cu'}" if c["n"] != 2 else ""
    s += "-gain4" if c["gain"] > 1 else ""
    s += "-vshift" if c["vshift"] else ""
    s += f"-ldo{c['ldo']}" if c["ldo"] % 8 else ""
    s += "" if c["olo"] else "-nolo"
    return s


def fwd_cases():
    out = []
    for kind in ("bf16", "f32"):
        for Lq, Lk in ((1, 1), (33, 31), (128, 64), (129, 65), (384, 97)):
            out += [case(Lq, Lk, kind, H=3, p=p, want="stream") for p in (0.0, 0.1)]
        out.append(case(129, 65, kind, H=3, p=0.5, want="stream"))
    out += [case(450, 152, "bf16", H=3, p=p, ldo=516, want="stream") for p in (0.0, 0.1)]
    out.append(case(129, 65, "bf16", H=3, p=0.1, gain=4, want="stream"))
    for Lq, Lk in ((385, 32), (385, 33), (450, 63), (512, 64), (450, 152), (450, 450), (512, 512), (450, 513), (450, 545)):
        out += [case(Lq, Lk, p=p, want="res1") for p in (0.0, 0.1)]
    out.append(case(450, 450, p=0.5, want="res1"))
    out.append(case(450, 545, p=0.1, gain=4, want="res1"))
    out += [case(385, 40, n=0, p=p, want="res2") for p in (0.0, 0.1)]
    return out


def bwd_cases():
    out = []
    for Lq, Lk in ((256, 1), (257, 33), (289, 31), (450, 152), (450, 450), (512, 512)):
        out += [case(Lq, Lk, p=p, olo=olo, want="res") for p in (0.0, 0.1) for olo in (True, False)]
    for Lq, Lk in ((255, 40), (513, 40), (300, 513)):
        out += [case(Lq, Lk, H=3, p=p, olo=olo, want="stream") for p in (0.0, 0.1) for olo in (True, False)]
    for Lq, Lk in ((1, 1), (33, 31), (129, 65), (128, 128)):
        out += [case(Lq, Lk, H=3, p=p, olo=olo, want="stream") for p in (0.0, 0.1) for olo in (True, False)]
        out += [case(Lq, Lk, "f32", H=3, p=p, olo=False, want="stream") for p in (0.0, 0.1)]
    out.append(case(450, 450, p=0.0, vshift=1.5, want="res"))
    out.append(case(450, 152, p=0.1, gain=4, want="res"))
    return out


def n_seq(c, n_cu=256):
    return c["n"] or n_cu // 16 + 1


def pads(c, backward=False):
    """(Lp_q, Lp_k): the Q image in 128 rows; the K / V images in 64 rows for a forward-only case, 128 where the backward reads them"""
    return round_up(c["Lq"], 128), c["Lp_k"] or round_up(c["Lk"], 128 if backward else 64)


SITE = 16 + 8 * 3


def keep_of(c, Lp_k, n_cu=256):
    return Keep(SITE, n_seq(c, n_cu), c["H"], c["Lq"], c["Lk"], c["p"], Lp_k=Lp_k)


def inputs(c, Lp_q, Lp_k, *, poison=False, n_cu=256, seed=70):
    """the padded images Q' [n, H, Lp_q, 64], K, V [n, H, Lp_k, 64], dO [n, H, Lp_q, 64] as float32 values, bf16-representable in a
    bf16 case.  Q' = 0.25 gain N(0, 1) (logits of deviation 2 gain); with gain > 1 one dominant key 2 q[row 5] sits three keys from
    the end and, for Lk > 512, at key 512.  V = N(0, 1) + vshift.  Padding rows are zero, or with `poison` finite values that would
    change every output if a kernel let them in: K rows 8 q[row 0] of the head (they would win every softmax), V rows 100, Q' rows
    50.  dO's padding rows are always zero (tcdiff_hip.h)."""
    n, H, Lq, Lk = n_seq(c, n_cu), c["H"], c["Lq"], c["Lk"]
    cast = bf if c["kind"] == "bf16" else (lambda t: t)
    q = cast(rnd(seed, n, H, Lq, 64, scale=0.25 * c["gain"]))
    k, v = cast(rnd(seed + 1, n, H, Lk, 64)), cast(rnd(seed + 2, n, H, Lk, 64) + c["vshift"])
    do = cast(rnd(seed + 3, n, H, Lq, 64))
    if c["gain"] > 1 and Lq > 5:
        k[:, :, max(Lk - 3, 0)] = 2.0 * q[0, :, 5].unsqueeze(0)
        if Lk > 512:
            k[:, :, 512] = 2.0 * q[0, :, 5].unsqueeze(0)
    Q, dO = torch.zeros(n, H, Lp_q, 64), torch.zeros(n, H, Lp_q, 64)
    Kp, Vp = torch.zeros(n, H, Lp_k, 64), torch.zeros(n, H, Lp_k, 64)
    Q[:, :, :Lq], dO[:, :, :Lq], Kp[:, :, :Lk], Vp[:, :, :Lk] = q, do, k, v
    if poison:
        Q[:, :, Lq:] = 50.0
        Kp[:, :, Lk:] = (8.0 * q[0, :, 0]).reshape(1, H, 1, 64)
        Vp[:, :, Lk:] = 100.0
    return Q, Kp, Vp, dO


def out_name(out, c):
    return out + ("_big" if c["gain"] > 1 else "")


# ---- regions --------------------------------------------------------------------------------------------------------------------------
def tok_regions(n, H, Lx):
    """regions of a token-major [n Lx, H 64] output: the whole tensor, each (sequence, head) block, the rows of each sequence's last
    partial 32-row group (for dK / dV: 32-key group) and of its last partial 128-row block"""
    pos, seq = torch.arange(n * Lx) % Lx, torch.arange(n * Lx) // Lx
    out = [("all", None, slice(0, 64 * H))]
    out += [(f"sh{s}.{h}", seq == s, slice(64 * h, 64 * h + 64)) for s in range(n) for h in range(H)]
    if Lx % 32:
        out.append(("tail32", pos >= Lx // 32 * 32, slice(0, 64 * H)))
    if Lx % 128:
        out.append(("tail128", pos >= Lx // 128 * 128, slice(0, 64 * H)))
    return out


def row_regions(Lq):
    """regions of a per-row statistic laid out [n H, Lq]"""
    out = [("all", None, slice(0, Lq))]
    if Lq % 32:
        out.append(("tail32", None, slice(Lq // 32 * 32, Lq)))
    return out


def region_class(name):
    return "sh" if name.startswith("sh") else name


# ---- mask probes ----------------------------------------------------------------------------------------------------------------------
PROBE_SHAPES = ((450, 450), (417, 97))
PROBE_P = {"fwd": 0.1, "dkv": 0.1, "dq": 0.75}


def probe_blocks(which, Lk):
    """the launches of a probe: one, or for "dq" one per 64-key block"""
    return list(range(-(-Lk // 64))) if which == "dq" else [None]


def probe_inputs(which, Lq, Lk, kind, Lp_q, Lp_k, n=2, H=8, seed=90, block=None):
    """inputs that make each regenerated keep bit observable on its own.  Q = 0.25 N(0, 1), Q' = Q / 8 (P nearly uniform) and one-hot rows
    e_{i mod 64} collapse an output element onto the handful of weights whose index is congruent to it:
      "fwd": V = e_{k mod 64}:  O[q][d]  = sum_{k = d mod 64} Pd[q, k];
      "dkv": dO = e_{q mod 64}: dV[k][d] = sum_{q = d mod 64} Pd[q, k];
      "dq":  K = e_{k mod 64}, V and dO positive (dPd = dO V^T about 1.27): dQ[q][d] = scale_q sum_{k = d mod 64} dS[q, k].
    The first two are sums of positive terms.  dS = P (keep scale dPd - delta) is not: its row sums are zero, and with every key
    live an element is the difference of n_d = Lk / 64 kept terms of (scale - 1) dPd and dropped ones of -dPd, which cancels
    to nothing in the rows where delta = sum_k Pd dPd comes out a few per cent high -- no tolerance relative to the element
    holds there.  So the dq probe runs once per 64-key block with V zero outside the block (dPd = 0 there, the block's bits are
    the observed ones), at p = 0.75: delta is dPd times the block's share of the keys, an element is P (4 dPd - n_d delta) when its
    one live bit is kept (n_d delta is 0.9 to 1.3 dPd: about +3 dPd P) and -n_d delta P when it is dropped, one term in one sign,
    and delta's own spread (a fifth of it) leaves the kept form many deviations from zero (tests/test_attn_train_reference_cpu.py
    asserts that no element is less than an eighth of the magnitudes summed into it)."""
    cast = bf if kind == "bf16" else (lambda t: t)
    eye = torch.eye(64)
    q = cast(rnd(seed, n, H, Lq, 64, scale=0.25 * 0.125))
    k, v, do = cast(rnd(seed + 1, n, H, Lk, 64)), cast(rnd(seed + 2, n, H, Lk, 64)), cast(rnd(seed + 3, n, H, Lq, 64))
    if which == "fwd":
        v = eye[torch.arange(Lk) % 64].expand(n, H, Lk, 64).clone()
    elif which == "dkv":
        do = eye[torch.arange(Lq) % 64].expand(n, H, Lq, 64).clone()
    else:
        k = eye[torch.arange(Lk) % 64].expand(n, H, Lk, 64).clone()
        v = cast(1.0 + 0.25 * torch.rand(n, H, Lk, 64, generator=torch.Generator().manual_seed(seed + 4)))
        do = cast((1.0 + 0.25 * torch.rand(n, H, Lq, 64, generator=torch.Generator().manual_seed(seed + 5))) / 64.0)
        if block is not None:
            v = v * (torch.arange(Lk) // 64 == block).to(v.dtype)[None, None, :, None]
    Q, dO = torch.zeros(n, H, Lp_q, 64), torch.zeros(n, H, Lp_q, 64)
    Kp, Vp = torch.zeros(n, H, Lp_k, 64), torch.zeros(n, H, Lp_k, 64)
    Q[:, :, :Lq], dO[:, :, :Lq], Kp[:, :, :Lk], Vp[:, :, :Lk] = q, do, k, v
    return Q, Kp, Vp, dO


def bf16_ulp(x):
    """the bf16 ulp of |x| (float64 tensor): 2^(floor(log2 |x|) - 7); the smallest normal's below it"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


# ---- a case through a Ref, and its comparison (shared by the CPU and the GPU module) -------------------------------------------------
def model_of(kind, defect=None):
    """the model of a kind's kernels: the f32 kernels round nothing"""
    return Ref(kind == "bf16", defect)


def fwd_outputs(o, kind):
    """Ref.fwd's dict -> the compared outputs: token-major O (and O + O_lo in bf16), lse as [n H, Lq]"""
    out = {"O": tok(o["O"]), "lse": o["lse"].reshape(-1, o["lse"].shape[-1])}
    if kind == "bf16":
        out["O+O_lo"] = tok(o["O+O_lo"])
    return out


def bwd_outputs(b):
    return {"delta": b["delta"].reshape(-1, b["delta"].shape[-1]), "dQ": tok(b["dQ"]), "dK": tok(b["dK"]), "dV": tok(b["dV"])}


def regions_of(out, c, n):
    if out in ("lse", "delta"):
        return row_regions(c["Lq"])
    return tok_regions(n, c["H"], c["Lk"] if out in ("dK", "dV") else c["Lq"])


def zero_gradient_tops(c, Q, Kp, Vp, dO):
    """With one key P = 1 and dS = dP - delta = 0 exactly: dQ and dK are zero, and what a kernel or a reference holds there is the
    rounding residue of delta.  Their differences are scaled by the magnitude of the terms that cancel, P dP K and P dP Q',
    instead of the reference's own top magnitude (which is that residue).  {} for Lk > 1."""
    if c["Lk"] > 1:
        return {}
    Lq = c["Lq"]
    dp = float((dO[:, :, :Lq].double() @ Vp[:, :, :1].double().transpose(-1, -2)).abs().max())
    return {"dQ": 0.125 * dp * float(Kp[:, :, :1].abs().max()), "dK": dp * float(Q[:, :, :Lq].abs().max())}


def stats(got, ref, regs, top=None):
    """x3_ref.region_stats with a given top magnitude"""
    if top is None:
        return region_stats(got, ref, regs)
    return {k: (a * t / top, b * t / top) for t in [float(torch.as_tensor(ref).abs().max()) or 1.0]
            for k, (a, b) in region_stats(got, ref, regs).items()}


def measure(got, refs, c, n, tops=None):
    """[(bounds key, region, max, mean)] of every output in `got` against refs["model"] and refs["f64"], region by region"""
    rows = []
    for out, g in got.items():
        regs = regions_of(out, c, n)
        for against in ("model", "f64"):
            st = stats(g, refs[against][out], regs, (tops or {}).get(out))
            rows += [((out_name(out, c), c["kind"], against), reg, mx, mn) for reg, (mx, mn) in st.items()]
    return rows


def frobenius(got, ref):
    got, ref = torch.as_tensor(got).detach().cpu().double().reshape(-1), torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def report(rows, worst=None):
    """one printed line per (bounds key): the worst figure of each region class; folded into `worst` when given"""
    lines = {}
    for key, reg, mx, mn in rows:
        cls = region_class(reg)
        d = lines.setdefault(key, {})
        d[cls] = (max(d.get(cls, (0, 0))[0], mx), max(d.get(cls, (0, 0))[1], mn))
        if worst is not None:
            w = worst.setdefault(key, {})
            w[cls] = (max(w.get(cls, (0, 0))[0], mx), max(w.get(cls, (0, 0))[1], mn))
    for (out, kind, against), d in lines.items():
        print(f"{out:10s} {kind:4s} vs {against:5s} " + " ".join(f"{r}={a:.2e}/{b:.2e}" for r, (a, b) in d.items()))


def outside(rows, bounds=None):
    bounds = BOUNDS if bounds is None else bounds
    return [(key, reg, mx, mn, bounds[key]) for key, reg, mx, mn in rows if not (mx <= bounds[key][0] and mn <= bounds[key][1])]
