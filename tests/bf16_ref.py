"""The bf16 launchers' arithmetic in float64: the reference that compute_dtype "bf16" is held to, launcher by launcher and region by
region, by tests/test_bf16_kernels_f64_gpu.py; pinned to plain float64 and to torch's own bf16 cast by
tests/test_bf16_reference_cpu.py.

``Ref(rounding=False)`` is the operation in float64 on the given operand values.  ``Ref(rounding=True)`` rounds to bf16 (nearest,
ties to even: x3_ref.bf16_rne, as v_cvt_pk_bf16_f32 rounds) exactly where a bf16 kernel hands a value on, and nowhere else:

  * GEMM: the operands are bf16 already and every product is exact in fp32, so the only rounding is the bf16 store (TC_EPI_STORE_T,
    the Q / K / V images, h / rot of gemm_rowln and ln_rot); fp32 outputs are not rounded;
  * attention (csrc/attention.hip:120-157, csrc/attn_res.h:127-176): keys in tiles of 64 (a last tile is what is left), the running
    maximum per tile in the exp2 domain, p = exp2(s log2e - m_new), the denominator summed from the UNROUNDED p, P rounded to bf16
    before P V, the accumulator rescaled by exp2(m_run - m_new), 1 / l last, then the bf16 store;
  * elementwise launchers: the fp32 value, then the bf16 store.

``standin()`` is the same arithmetic in float32 torch on the CPU (fp32 sums, fp32 exp2 of the kernels' fused exponent
fma(s, log2e, -m), torch's bf16 casts at the same points): what an honest kernel looks like.  tests/test_bf16_reference_cpu.py keeps it inside every bound below, and shows that each
emulated kernel defect (DEFECTS) moves the region it touches by at least ten times that region's bound.

LayerNorm and rotary in float64 come from tests/layer_ref.py; rounding, regions and test data from tests/x3_ref.py.  The GPU
module's cases and their inputs are defined here, so that the CPU module runs the reference and the stand-in on exactly them.
Not a test module: no test_* name, nothing collected here."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import x3_ref as XR
from layer_ref import LOG2E
from layer_ref import Ref as LayerRef
from x3_ref import act64, bf16_rne, region_stats, rnd, rope_f32, sin_freq, worst  # noqa: F401  (re-exported to the test modules)

D = torch.float64
TILE, CHUNK = 64, 512            # attention: keys per tile, keys per LDS-resident chunk of the K/V-resident kernel

DEFECTS = (
    "acc_bf16",          # GEMM partial sums rounded to bf16 once per 64-deep k-tile
    "gelu_tanh",         # the tanh-approximated GELU in a GEMM epilogue
    "bias_chunk",        # the bias missing in the last partial 8-column chunk
    "p_trunc",           # attention's P truncated to bf16 instead of rounded
    "mask_off_by_one",   # key Lk takes part in the softmax
    "no_rescale_chunk",  # the accumulator not rescaled when the maximum grows in the first tile of a second 512-key chunk
    "eps_swap",          # the two LayerNorm eps (1e-6 after the product, 1e-5 in front of the next one) swapped
    "rope_tail_shift",   # the rows of the last partial row block rotated by their neighbour's angle (as in layer_ref)
)

# Bounds of the bf16 launchers (tests/test_bf16_kernels_f64_gpu.py): (max, mean) of |kernel - reference| / max |reference| per
# region, for (launcher, output kind, against).  "model": Ref(rounding=True); "f64": Ref(rounding=False) on the same operand values.
# Set from the MI355X run recorded in profiles/bf16_kernels_f64.txt at 4x the worst value observed over the launcher's cases and
# regions (in brackets: max / mean), with two figures that are not measurements:
#   * an fp32 store of a bf16 product against float64 has the ceiling 1e-5 (the project's own figure for fp32 sums of identical
#     products); every measured bound lies far below it;
#   * the MAX of a bf16 store against the model is ONE_ULP = 2^-7 wherever a flip was seen.  Kernel and model round nearly the same
#     fp32 value, so they differ by one bf16 ulp of the element (at most 2^-7 of it) or not at all; WHICH element flips is chance
#     (the float32 stand-in flips others: up to 3.1e-3 where the kernels' worst is 5e-4), so the max is the format's figure and the
#     MEAN is the sharp statistic.  In two launchers 4x the kernels' worst mean is less than ONE flip costs in a 128-column
#     region of 150 or 210 rows (1e-7 to 2e-7 of mean), and the stand-in, which has such a flip, would fail a bound that the
#     kernels met by chance; there the bound is 4x the stand-in's mean, marked [stand-in].
# "attention_big" are the gain-4 cases (logits of hundreds, nearly one-hot rows).  Their mean against the model is 100x that of the
# other cases, for a reason in the data, not the kernels: with the dominant key placed twice, a one-hot row's exact output is
# (v_512 + v_last) / 2 of two bf16 values -- an exact rounding TIE of the bf16 store, which the float64 model resolves to even and
# any fp32 evaluation (2^-20 from the tie) resolves by its last bit.  A float32 evaluation with the kernels' fused exponent
# (standin) shows the same 1.3e-5.
ONE_ULP = 2.0 ** -7
BOUNDS = {
    ("gemm_tile", "f32", "model"): (1.7e-6, 2e-7),          # [4.0e-7 / 4.8e-8]  model == f64: an fp32 store is not rounded
    ("gemm_tile", "f32", "f64"): (1.7e-6, 2e-7),            # [4.0e-7 / 4.8e-8]
    ("gemm_tile", "bf16", "model"): (ONE_ULP, 2.7e-7),      # [2.1e-3 / 6.7e-8]
    ("gemm_tile", "bf16", "f64"): (1.3e-2, 1.6e-3),         # [3.0e-3 / 3.9e-4]
    ("gemm_small", "f32", "model"): (7e-7, 1.1e-7),         # [1.7e-7 / 2.5e-8]
    ("gemm_small", "f32", "f64"): (7e-7, 1.1e-7),           # [1.7e-7 / 2.5e-8]
    ("gemm_small", "bf16", "model"): (ONE_ULP, 8.3e-7),     # [6.2e-4 / 5.2e-8]  [stand-in 1.3e-3 / 2.07e-7: cols2 of 150 x 1024]
    ("gemm_small", "bf16", "f64"): (1.4e-2, 1.2e-3),        # [3.4e-3 / 2.9e-4]
    ("gemm_rows", "f32", "model"): (1.9e-6, 1.5e-7),        # [4.7e-7 / 3.6e-8]
    ("gemm_rows", "f32", "f64"): (1.9e-6, 1.5e-7),          # [4.7e-7 / 3.6e-8]
    ("gemm_rows", "bf16", "model"): (ONE_ULP, 1.1e-6),      # [2.3e-3 / 2.7e-7]
    ("gemm_rows", "bf16", "f64"): (1.4e-2, 2e-3),           # [3.3e-3 / 4.9e-4]
    ("qkv", "bf16", "model"): (ONE_ULP, 4.1e-7),            # [5.1e-4 / 2.4e-8]  [stand-in 2.4e-3 / 1.03e-7: cols3 of 210 x 1536]
    ("qkv", "bf16", "f64"): (9.6e-3, 1e-3),                 # [2.4e-3 / 2.5e-4]
    ("gemm_rowln", "f32", "model"): (1.1e-6, 8e-8),         # [2.7e-7 / 2.0e-8]
    ("gemm_rowln", "f32", "f64"): (1.1e-6, 8e-8),           # [2.7e-7 / 2.0e-8]
    ("gemm_rowln", "bf16", "model"): (ONE_ULP, 9.2e-7),     # [2.3e-3 / 2.3e-7]
    ("gemm_rowln", "bf16", "f64"): (1.3e-2, 1.1e-3),        # [3.2e-3 / 2.8e-4]
    ("ln_rot", "f32", "model"): (5.2e-7, 6.2e-8),           # [1.3e-7 / 1.5e-8]
    ("ln_rot", "f32", "f64"): (5.2e-7, 6.2e-8),             # [1.3e-7 / 1.5e-8]
    ("ln_rot", "bf16", "model"): (ONE_ULP, 3.7e-7),         # [3.1e-3 / 9.1e-8]
    ("ln_rot", "bf16", "f64"): (1.3e-2, 1.6e-3),            # [3.1e-3 / 4.0e-4]
    ("attention", "bf16", "model"): (ONE_ULP, 1.5e-6),      # [3.9e-3 / 3.6e-7]
    ("attention", "bf16", "f64"): (1.4e-2, 1.1e-3),         # [3.3e-3 / 2.7e-4]
    ("attention_big", "bf16", "model"): (ONE_ULP, 7.4e-5),  # [1.9e-3 / 1.8e-5]  ties: see above
    ("attention_big", "bf16", "f64"): (9.3e-3, 8.2e-4),     # [2.3e-3 / 2.0e-4]
    ("sinusoidal", "bf16", "model"): (0.0, 0.0),            # [0 / 0]
    ("sinusoidal", "bf16", "f64"): (7.8e-3, 2.6e-3),        # [2.0e-3 / 6.4e-4]
    ("add_act", "f32", "model"): (5.1e-7, 9.6e-8),          # [1.3e-7 / 2.4e-8]
    ("add_act", "f32", "f64"): (7e-7, 9.7e-8),              # [1.7e-7 / 2.4e-8]
    ("add_act", "bf16", "model"): (2.5e-5, 3.5e-8),         # [6.1e-6 / 8.6e-9]  one flip of a small element
    ("add_act", "bf16", "f64"): (1.2e-2, 1.3e-3),           # [3.0e-3 / 3.2e-4]
    ("step_prologue", "bf16", "model"): (0.0, 0.0),         # [0 / 0]
    ("step_prologue", "bf16", "f64"): (8.6e-3, 7.9e-4),     # [2.2e-3 / 2.0e-4]
}
LAUNCHERS = sorted({k[0] for k in BOUNDS})


def bf(t):
    """float32 values as the float32 of their bf16 rounding: what a bf16 operand holds"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def bf16_trunc(x):
    """float32 values -> bf16 by truncation (the low 16 bits dropped)"""
    u = XR._np32(x).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def regions(M, N, *, row_block=128, seq_len=None):
    """x3_ref.regions with the bf16 chunk: the last partial chunk is N % 8 columns (16 bytes of bf16)"""
    out = [r for r in XR.regions(M, N, row_block=row_block, seq_len=seq_len) if r[0] != "chunk"]
    if N % 8:
        out.append(("chunk", None, slice(N - N % 8, N)))
    return out


class Ref:
    def __init__(self, rounding=True, defect=None, dtype=D):
        if defect is not None and defect not in DEFECTS:
            raise ValueError(defect)
        self.rounding, self.defect, self.D = rounding, defect, dtype
        self.lr = LayerRef(rounding=False)

    def c(self, t):
        return torch.as_tensor(t).detach().cpu().to(self.D)

    def rb(self, v, trunc=False):
        """a bf16 hand-off of the kernel's fp32 value; identity without rounding"""
        if not self.rounding:
            return v
        if self.D != D:                                            # the stand-in: torch's own cast
            return v.to(torch.float32).to(torch.bfloat16).to(self.D)
        f = v.to(torch.float32)
        return torch.from_numpy((bf16_trunc if trunc else bf16_rne)(f).reshape(tuple(f.shape))).to(self.D)

    def mm(self, a, b):
        """a [.., M, K] (x) b [.., N, K]^T on the operand values (bf16-representable: every product exact)"""
        a, b = self.c(a), self.c(b)
        if self.defect != "acc_bf16":
            return a @ b.transpose(-1, -2)
        acc = torch.zeros(*a.shape[:-1], b.shape[-2], dtype=self.D)
        for k0 in range(0, a.shape[-1], 64):
            acc = self.rb(acc + a[..., k0:k0 + 64] @ b[..., k0:k0 + 64].transpose(-1, -2))
        return acc

    def ln(self, v, g, b, eps):
        if self.D == D:
            return self.lr.ln(v, g, b, eps)
        return F.layer_norm(v, (512,), self.c(g), self.c(b), eps)

    def rotate(self, u, rope, pos):
        if self.D == D:
            return self.lr.rotate(u, rope, pos)
        cs = self.c(rope)[pos].reshape(-1, 256, 2)
        up = u.reshape(-1, 256, 2)
        return torch.stack((up[..., 0] * cs[..., 0] - up[..., 1] * cs[..., 1], up[..., 1] * cs[..., 0] + up[..., 0] * cs[..., 1]),
                           -1).reshape(-1, 512)

    def act(self, v, act):
        from tcdiff_amd import _lib as L
        if self.defect == "gelu_tanh" and act == L.ACT_GELU:
            return F.gelu(v, approximate="tanh")
        return act64(v, act)

    # ---- gemm_tile / gemm_small / gemm_rows ------------------------------------------------------------------------------------
    def gemm(self, A, W, M, *, bias=None, act=0, a_mod=0, A2=None, split_n=0, store=False, scale_cols=None):
        """C[M, N] = act(A[m % a_mod] W^T + bias) (columns >= split_n from A2); store: the bf16 TC_EPI_STORE_T output"""
        rows = torch.arange(M) % a_mod if a_mod else torch.arange(M)
        v = self.mm(self.c(A)[rows], W)
        if A2 is not None:
            v[:, split_n:] = self.mm(self.c(A2)[rows], self.c(W)[split_n:])
        if bias is not None:
            b = self.c(bias).clone()
            N = b.numel()
            if self.defect == "bias_chunk" and N % 8:
                b[N - N % 8:] = 0.0
            v = v + b
        v = self.act(v, act)
        if scale_cols is not None:
            v = v * scale_cols.to(self.D)
        return self.rb(v) if store else v

    def qkv_heads(self, A, W, Lq, nseq, *, A2=None, split_n=0, bias=None, scale_q=0.125, n_q=512):
        """the head-major Q / K / V token values [nseq, H, Lq, 64] per image of the QKV scatter; images in column order"""
        N = W.shape[0]
        sc = torch.ones(N, dtype=self.D)
        sc[:n_q] = scale_q
        v = self.gemm(A, W, nseq * Lq, bias=bias, A2=A2, split_n=split_n, store=True, scale_cols=sc)
        return [v[:, c:c + 512].reshape(nseq, Lq, 8, 64).permute(0, 2, 1, 3) for c in range(0, N, 512)]

    # ---- gemm_rowln ------------------------------------------------------------------------------------------------------------
    def rowln(self, A, W, M, *, a_mod=0, bias=None, ln=None, film=None, xres=None, xres_mod=0, Lseq=1, nln=None, rope=None,
              out_mul=1, out_add=0, groups=1, store_h=False):
        """the epilogue chain of tcdiff_gemm_rowln (see x3_ref.Ref.rowln): v = A W^T + bias; LN_POST (ln = (g, b, eps)); FILM of
        row m / Lseq; + xres[m % xres_mod]; x = v (fp32); NEXT_LN (nln) -> h (bf16); rotary -> rot (bf16).  Returns {mo: output row
        indices, x, h, rot} per group concatenated (row block 64)"""
        if self.defect == "eps_swap" and ln is not None and nln is not None:
            ln, nln = (ln[0], ln[1], nln[2]), (nln[0], nln[1], ln[2])
        rows = torch.arange(M) % a_mod if a_mod else torch.arange(M)
        out = {"mo": [], "x": [], "h": [], "rot": []}
        tail = torch.arange(M) >= (M // 64) * 64
        for g in range(groups):
            v = self.mm(self.c(A)[rows], W[512 * g:512 * g + 512])
            if bias is not None:
                v = v + self.c(bias[512 * g:512 * g + 512])
            if ln is not None:
                v = self.ln(v, ln[0], ln[1], ln[2])
            m = torch.arange(M)
            if film is not None:
                fr = self.c(film)[m // Lseq]
                v = (fr[:, :512] + 1) * v + fr[:, 512:1024]
            if xres is not None:
                v = self.c(xres)[m % xres_mod if xres_mod else m] + v
            mo = m * out_mul + out_add + g
            out["mo"].append(mo)
            out["x"].append(v)
            u = v
            if nln is not None:
                u = self.ln(v, nln[0], nln[1], nln[2])
                if rope is not None:
                    pos = mo % Lseq
                    if self.defect == "rope_tail_shift":
                        pos = torch.where(tail, pos + 1, pos)
                    out["rot"].append(self.rb(self.rotate(u, rope, pos)))
            if store_h:
                out["h"].append(self.rb(u))
        return {k: torch.cat(v) if v else None for k, v in out.items()}

    # ---- attention -------------------------------------------------------------------------------------------------------------
    def attention(self, q, k, v, Lk, n_shared=0, *, store=True, tile=TILE, chunk=CHUNK):
        """q [nseq, H, Lq, 64], k / v [n_kv, H, >= Lk, 64] (the values of the images, padding rows included) -> O token rows
        [nseq Lq, 512]: the online softmax of the kernels over key tiles; store=False: the fp32 value before the bf16 store"""
        nseq, H, Lq = q.shape[:3]
        kv = torch.tensor([0 if s < n_shared else s - n_shared + (1 if n_shared > 0 else 0) for s in range(nseq)])
        nk = Lk + 1 if self.defect == "mask_off_by_one" and k.shape[2] > Lk else Lk
        kk, vv = self.c(k)[kv][:, :, :nk], self.c(v)[kv][:, :, :nk]
        s_all = self.c(q) @ kk.transpose(-1, -2)
        fused = self.D != D          # the stand-in: the kernels' x = fma(s, log2e, -m), one rounding; m = fp32(max s * log2e)
        if not fused:
            s_all = s_all * LOG2E
        m = torch.full((nseq, H, Lq, 1), -math.inf, dtype=self.D)
        l = torch.zeros(nseq, H, Lq, 1, dtype=self.D)
        o = torch.zeros(nseq, H, Lq, 64, dtype=self.D)
        for t0 in range(0, nk, tile):
            s = s_all[..., t0:t0 + tile]
            if fused:
                m_new = torch.maximum(m, s.amax(-1, keepdim=True) * torch.tensor(LOG2E, dtype=self.D))
                p = torch.exp2((s.double() * LOG2E - m_new.double()).to(self.D))
            else:
                m_new = torch.maximum(m, s.amax(-1, keepdim=True))
                p = torch.exp2(s - m_new)
            alpha = torch.exp2(m - m_new)
            l = l * alpha + p.sum(-1, keepdim=True)
            if not (self.defect == "no_rescale_chunk" and t0 > 0 and t0 % chunk == 0):
                o = o * alpha
            o = o + self.rb(p, trunc=self.defect == "p_trunc") @ vv[..., t0:t0 + tile, :]
            m = m_new
        o = (o / l).permute(0, 2, 1, 3).reshape(nseq * Lq, H * 64)
        return self.rb(o) if store else o

    # ---- elementwise launchers -------------------------------------------------------------------------------------------------
    def ln_rot(self, x, g, b, eps, rope=None, pos=None):
        if self.defect == "eps_swap":
            eps = 1e-6 if eps == 1e-5 else 1e-5
        u = self.ln(self.c(x), g, b, eps)
        out = {"y32": u, "h": self.rb(u)}
        if rope is not None:
            out["rot"] = self.rb(self.rotate(u, rope, pos))
        return out

    def convert_pad(self, src, ld):
        v = torch.zeros(src.shape[0], ld, dtype=self.D)
        v[:, :src.shape[1]] = self.c(src)
        return self.rb(v)

    def sinusoidal(self, times, freq):
        ang = self.c(times.cpu().to(torch.float32)[:, None] * freq.cpu()[None, :])     # the kernel's fp32 angle
        return self.rb(torch.cat((ang.sin(), ang.cos()), -1))

    def add_act(self, a, ia, b, act):
        a = a.cpu()[ia.long().cpu()]
        v = self.c(a + b.cpu()) if self.rounding else self.c(a) + self.c(b)            # the kernel's fp32 sum, then the activation
        v = self.act(v, act)
        return {"out32": v, "out": self.rb(v)}


def standin(defect=None):
    """the bf16 kernels' arithmetic in float32 torch on the CPU"""
    return Ref(True, defect, dtype=torch.float32)


# ---- kernel selection, restated from the launchers ---------------------------------------------------------------------------------
def small_product(M, N, K, n_cu, *, ldc, A2=False):
    """csrc/gemm.hip small_product for a bf16 TC_EPI_STORE_T / _F32 product with small_m set and an aligned bias"""
    if A2 or N % 32 or K % 32 or K > 2048 or ldc % 4:
        return False
    big, small = -(-N // 128) * -(-M // 128), (N // 32) * -(-M // 32)
    return big * 4 <= n_cu and small <= 2 * n_cu


def deep_pipeline(M, N, K, n_cu):
    """csrc/gemm.hip launch_tile: the four-stage gemm_tile_kernel (about one tile per CU, at least three 64-deep k-tiles)"""
    return -(-N // 128) * -(-M // 128) * 4 <= n_cu * 5 and K // 64 >= 3


def long_loop_rows(N, n_cu):
    """the smallest M whose 128 x 128 tiles exceed 1.25 per CU (the two-stage kernel whatever K): 2561 at N = 2048 on 256 CUs"""
    nt = -(-N // 128)
    return 128 * ((n_cu * 5) // (4 * nt)) + 1


def rows_mt(M, n_cu):
    """csrc/gemm_rows.hip: mt of tcdiff_gemm_rows when the caller passes 0"""
    return 1 if -(-M // 16) <= n_cu else 2 if -(-M // 32) <= n_cu else 4


def resident(Lp_q):
    """csrc/attention.hip: bf16 takes the K/V-resident kernel when the Q image is padded to at least 512 rows"""
    return Lp_q >= 512


def round_up(x, m):
    return -(-x // m) * m


# ---- the GPU module's cases and their inputs ---------------------------------------------------------------------------------------
def _acts():
    from tcdiff_amd import _lib as L
    return L


def gemm_tile_cases(n_cu=256):
    """dicts of M, N, K, act and: stores ("f32" / "bf16"), ldc, a_mod, split_n (A2), lda (> K: A a column slice), deep (the pipeline
    the case is meant to reach)"""
    L = _acts()
    c = lambda M, N, K, act, **kw: dict(dict(M=M, N=N, K=K, act=act, stores=("f32", "bf16"), ldc=N + 8, a_mod=0, split_n=0, lda=K,  # noqa: E731
                                             deep=deep_pipeline(M, N, K, 256)), **kw)
    return [
        c(1, 512, 512, L.ACT_GELU), c(2, 2048, 512, L.ACT_MISH), c(2, 512, 2048, L.ACT_NONE),      # the time MLP's rows
        c(127, 1024, 64, L.ACT_RELU, deep=False), c(129, 640, 128, L.ACT_SILU, deep=False),        # 1 and 2 k-tiles
        c(130, 150, 192, L.ACT_NONE, deep=True),                                                   # 3 k-tiles; partial tile and chunk
        c(300, 151, 512, L.ACT_NONE, stores=("f32",), ldc=152), c(300, 438, 896, L.ACT_RELU),      # final projection; cond_projection
        c(long_loop_rows(2048, n_cu), 2048, 512, L.ACT_GELU, deep=False),                          # two stages, long k-loop
        c(260, 512, 128, L.ACT_NONE, a_mod=100, split_n=256, lda=128 + 64, deep=False),
    ]


def gemm_small_cases():
    """(M, N, K, act, bias, a_mod, selected)"""
    L = _acts()
    return [(150, 1024, 576, L.ACT_RELU, True, 0, True), (7, 64, 64, L.ACT_GELU, True, 0, True), (33, 96, 2048, L.ACT_SILU, True, 0, True),
            (31, 1024, 1024, L.ACT_NONE, False, 0, True), (150, 512, 320, L.ACT_NONE, True, 50, True),
            (150, 512, 2112, L.ACT_NONE, True, 0, False)]


GEMM_ROWS_M = (1, 17, 47, 917)
GEMM_ROWS_NK = ((512, 512, 0), (1024, 512, 0), (512, 1024, 0), (1536, 512, 1024))       # N, K, split_n (A2)


def gemm_inputs(M, N, K, *, a_mod=0, split_n=0, lda=None, seed=1, a_scale=1.0):
    """bf16-representable operands: A [rows, lda] (the operand is A[:, lda - K:]), W [N, K], A2 likewise when split_n; fp32 bias"""
    lda = lda or K
    rows = a_mod or M
    d = dict(A=bf(rnd(seed, rows, lda, scale=a_scale)), W=bf(rnd(seed + 1, N, K, scale=1 / math.sqrt(K))), bias=rnd(seed + 2, N),
             A2=bf(rnd(seed + 3, rows, lda, scale=a_scale)) if split_n else None, off=lda - K)
    return d


def gemm_ref(r, d, M, *, act=0, bias=True, a_mod=0, split_n=0, store=False):
    o = d["off"]
    return r.gemm(d["A"][:, o:], d["W"], M, bias=d["bias"] if bias else None, act=act, a_mod=a_mod,
                  A2=d["A2"][:, o:] if split_n else None, split_n=split_n, store=store)


# attention: (Lq, Lk, sequences, n_shared, gain)
ATTN_STREAM = [(1, 1, 1, 0, 1), (33, 64, 2, 0, 1), (120, 62, 2, 1, 1), (97, 65, 1, 0, 1), (128, 96, 1, 0, 1), (129, 97, 4, 2, 1),
               (70, 127, 2, 0, 4)]
ATTN_RES = [(1, 1, 1, 0, 1), (32, 64, 1, 0, 1), (33, 33, 2, 0, 1), (257, 152, 4, 2, 1), (450, 450, 1, 0, 1), (33, 512, 1, 0, 1),
            (33, 513, 1, 0, 1), (64, 545, 1, 0, 4), (257, 1024, 1, 0, 1), (33, 1025, 2, 1, 1), (513, 97, 1, 0, 1)]
ATTN_POISON = [(120, 62, 2, 1, 1), (257, 152, 4, 2, 1), (33, 513, 1, 0, 1)]


def attn_inputs(Lq, Lk, nseq, n_shared, gain, *, Lp_q, poison=False, seed=40, rounded=True):
    """the padded images Q [nseq, 8, Lp_q, 64], K / V [n_kv, 8, Lp_k, 64] (Lp_k: Lk rounded up to 64) as float32 values, bf16-
    representable when `rounded`.  q is scaled by 0.5 gain; with gain > 1 one dominant key k = 2 q[row 5] sits in the last partial
    tile and, for Lk > 512, at key 512 (the first tile of the second chunk).  Padding rows are zero, or with `poison` finite values
    that would change every output row if a kernel let them in: K rows 8 q[row 0] of the head (a key that would win every
    softmax), V rows 100, Q rows 50."""
    H, Lp_k = 8, round_up(Lk, 64)
    n_kv = nseq if n_shared == 0 else nseq - n_shared + 1
    cast = bf if rounded else (lambda t: t)
    q = cast(rnd(seed, nseq, H, Lq, 64, scale=0.5 * gain))
    k, v = cast(rnd(seed + 1, n_kv, H, Lk, 64)), cast(rnd(seed + 2, n_kv, H, Lk, 64))
    if gain > 1 and Lq > 5:
        k[:, :, max(Lk - 3, 0)] = 2.0 * q[0, :, 5].unsqueeze(0)
        if Lk > 512:
            k[:, :, 512] = 2.0 * q[0, :, 5].unsqueeze(0)
    Q = torch.zeros(nseq, H, Lp_q, 64)
    Kp, Vp = torch.zeros(n_kv, H, Lp_k, 64), torch.zeros(n_kv, H, Lp_k, 64)
    Q[:, :, :Lq], Kp[:, :, :Lk], Vp[:, :, :Lk] = q, k, v
    if poison:
        Q[:, :, Lq:] = 50.0
        Kp[:, :, Lk:] = (8.0 * q[0, :, 0]).reshape(1, H, 1, 64)
        Vp[:, :, Lk:] = 100.0
    return Q, Kp, Vp


def attn_ref(r, Q, Kp, Vp, Lq, Lk, n_shared, **kw):
    return r.attention(Q[:, :, :Lq], Kp, Vp, Lk, n_shared, **kw)


def attn_name(gain):
    """the bounds' launcher name of an attention case: the gain-4 cases (logits of hundreds) have their own"""
    return "attention_big" if gain > 1 else "attention"


def attn_regions(Lq, nseq):
    return regions(nseq * Lq, 512, row_block=128, seq_len=Lq)


# gemm_rowln: (name, K, M, Lseq) of the full chain; the variants and the low-variance case are built by rowln_case below
ROWLN_FULL = [(512, 270, 90), (1024, 270, 90), (512, 65, 65), (1024, 1, 1), (512, 1, 1), (1024, 65, 65)]
ROWLN_NAMES = ["full-%d-%d" % (k, m) for k, m, _ in ROWLN_FULL] + ["shared_rows", "groups", "low_variance"]


def rowln_case(name):
    """(inputs dict, keyword arguments of Ref.rowln, M, K) of a gemm_rowln case.  low_variance: A, the residual and the FiLM scale
    are sized so that the rows in front of BOTH LayerNorms have variance about 1e-4, where 1e-6 and 1e-5 differ by percent"""
    g = lambda s: 1 + 0.1 * rnd(s, 512)                                               # noqa: E731
    if name.startswith("full") or name == "low_variance":
        low = name == "low_variance"
        Kd, M, Lq = (512, 270, 90) if low else [c for c in ROWLN_FULL if name == "full-%d-%d" % c[:2]][0]
        nseq = -(-M // Lq)
        A, W = bf(rnd(20, M, Kd, scale=0.01 if low else 1.0)), bf(rnd(21, 512, Kd, scale=1 / math.sqrt(Kd)))
        bias = rnd(22, 512, scale=1e-3 if low else 1.0)
        film = rnd(27, nseq, 1024, scale=0.5)
        xres = rnd(28, M, 512)
        if low:
            film = torch.cat([-1 + 0.01 * (1 + 0.1 * rnd(27, nseq, 512)), 0.01 * rnd(29, nseq, 512)], 1)
            xres = xres * 0.01
        kw = dict(bias=bias, ln=(g(23), 0.1 * rnd(24, 512), 1e-6), film=film, xres=xres, Lseq=Lq, nln=(g(25), 0.1 * rnd(26, 512), 1e-5),
                  rope=rope_f32(Lq + 1), store_h=True)
        return dict(A=A, W=W), kw, M, Kd
    M, Kd, G = 200, 512, 3
    A, W, bias = bf(rnd(30, M, Kd)), bf(rnd(31, G * 512, Kd, scale=1 / math.sqrt(Kd))), rnd(32, G * 512)
    if name == "shared_rows":                                                      # a_mod / xres_mod, plain bf16 copy of x
        return dict(A=A, W=W[:512]), dict(a_mod=150, bias=bias[:512], xres=rnd(33, 100, 512), xres_mod=100, Lseq=50, store_h=True), M, Kd
    # grouped, interleaved output rows (out_mul = groups, out_add = 0), next LN + rotary
    return dict(A=A, W=W), dict(bias=bias, Lseq=60, nln=(g(36), 0.1 * rnd(37, 512), 1e-5), rope=rope_f32(61), out_mul=G, groups=G,
                                store_h=True), M, Kd


# ln_rot: (name, rows, rope, low variance)
LN_ROT = [("1", 1, True, False), ("333", 333, True, False), ("333-plain", 333, False, False), ("333-low", 333, True, True)]


def ln_rot_case(name):
    _, rows, with_rope, low = [c for c in LN_ROT if c[0] == name][0]
    Lq = 50
    x = 0.01 * rnd(11, rows, 512) if low else rnd(11, rows, 512, scale=3.0) + 0.7
    return dict(x=x, g=1 + 0.1 * rnd(12, 512), b=0.1 * rnd(13, 512), eps=1e-5, rope=rope_f32(64) if with_rope else None,
                pos=torch.arange(rows) % Lq + 3, Lq=Lq, rows=rows)
