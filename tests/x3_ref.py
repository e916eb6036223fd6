"""The split-bf16 arithmetic of the parity modes in float64: the reference that the f32 and bf16x3 launchers are held to by
tests/test_parity_kernels_f64_gpu.py, pinned to plain float64 and to kernels.to_x3 by tests/test_x3_reference_cpu.py.

Written from the storage definition of csrc/common.h (MmaBF16x3), not from kernels.to_x3:

  * split(x) = (hi, lo), hi = bf16_rne(x), lo = bf16_rne(x - hi), on the float32 bit patterns (ties to even, as
    v_cvt_pk_bf16_f32 rounds; x - hi is exact in float32);
  * a 16-byte chunk of four elements e0..e3 is [hi e0..e3 | lo e0..e3] (eight bf16);
  * a product a b is a_hi b_hi + a_hi b_lo + a_lo b_hi; lo lo is dropped, as the kernels drop it.

``Ref(rounding=True)`` routes every MFMA operand through the split at exactly the points where a kernel splits (GEMM and attention
operands, the unnormalised softmax P before P V, every split-format store) and keeps everything else in float64; with
``rounding=False`` it is the operation in float64 on the float32 inputs.  LayerNorm and rotary come from tests/layer_ref.py.

``defect`` emulates a plausible kernel defect (DEFECTS below; tests/test_x3_reference_cpu.py shows that each one moves the region
it touches by at least ten times that region's GPU bound).  Not a test module: no test_* name, nothing collected here."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from layer_ref import Ref as LayerRef

D = torch.float64

DEFECTS = (
    "act_lo",        # an epilogue stores its split output without lo (the STORE_T chunk keeps hi only)
    "w_lo",          # the weight operand's lo is dropped in the k-loop
    "cross",         # the a_hi b_lo cross term is missing
    "p_hi",          # attention's P is split as hi only before P V
    "quad_swap",     # hi and lo quads swapped in chunk position 3 of every 128-byte row of the A operand
    "tail_no_lo",    # the rows of the last partial row block are stored without lo
    "f32_as_x3",     # f32 mode: the exact fp32 products replaced by split-bf16 ones (Ref(rounding=True) against the f32 bounds)
)

# Bounds of the launchers against this reference (tests/test_parity_kernels_f64_gpu.py), per launcher and region: (max, mean) of
# |kernel - reference| / max |reference|.  "mm3": bf16x3 against Ref(rounding=True); "x3": bf16x3 against float64; "f32": f32
# against float64.  Set from the first MI355X run at no more than 4x the worst value observed (in brackets: max / mean), under the
# ceilings mm3 2e-5, x3 1e-4, f32 1e-5.  A split-format store is at most one lo ulp (2^-17 of the element) from the model's split of
# the same value, hence mm3 ~1e-5 there.  Each f32 bound lies below the smallest bf16x3 error against float64 of its cases.
BOUNDS = {
    ("gemm_f32", "f32"): (2e-6, 2.6e-7),     # [1.2e-6 / 6.6e-8]    bf16x3 against float64 >= 2.5e-6 in every case
    ("gemm_f32", "mm3"): (3.6e-6, 1.6e-7),   # [9.2e-7 / 3.9e-8]
    ("gemm_f32", "x3"): (1.4e-5, 3.4e-6),    # [3.5e-6 / 8.6e-7]
    ("gemm_t", "f32"): (2e-6, 2.6e-7),       # [1.2e-6 / 6.5e-8]
    ("gemm_t", "mm3"): (2e-5, 2.6e-7),       # [1.1e-5 / 6.6e-8]
    ("gemm_t", "x3"): (3e-5, 4.2e-6),        # [7.6e-6 / 1.0e-6]
    ("gemm_split", "f32"): (2e-6, 1.7e-7),   # [6.5e-7 / 4.2e-8]
    ("gemm_split", "mm3"): (1.2e-6, 9.6e-8), # [3.0e-7 / 2.4e-8]
    ("gemm_split", "x3"): (2.4e-5, 3.4e-6),  # [6.1e-6 / 8.5e-7]
    ("qkv", "f32"): (2e-6, 1.6e-7),          # [6.2e-7 / 4.1e-8]
    ("qkv", "mm3"): (2e-5, 1e-7),            # [8.7e-6 / 2.6e-8]
    ("qkv", "x3"): (2.1e-5, 2.5e-6),         # [5.4e-6 / 6.3e-7]
    ("rowln", "f32"): (2e-6, 1.3e-7),        # [8.2e-7 / 3.3e-8]
    ("rowln", "mm3"): (2e-5, 8.4e-8),        # [7.4e-6 / 2.1e-8]
    ("rowln", "x3"): (1.9e-5, 2.2e-6),       # [4.8e-6 / 5.6e-7]
    ("attention", "f32"): (8e-6, 3.6e-7),    # [3.8e-6 / 9.1e-8]  bf16x3 against float64 >= 1.8e-5 in every case
    ("attention", "mm3"): (2e-5, 4.8e-7),    # [7.8e-6 / 1.2e-7]
    ("attention", "x3"): (1e-4, 7.2e-6),     # [9.4e-5 / 1.8e-6]: logits of tens -- the split-bf16 scores' error, exponentiated
    ("ln_rot", "f32"): (5e-7, 3.6e-8),       # [1.3e-7 / 9.2e-9]
    ("ln_rot", "mm3"): (2e-5, 3.3e-8),       # [6.1e-6 / 8.2e-9]
    ("ln_rot", "x3"): (2.4e-5, 1.2e-6),      # [6.0e-6 / 2.9e-7]
    ("convert_pad", "f32"): (0.0, 0.0),      # [0 / 0]: a copy
    ("convert_pad", "mm3"): (0.0, 0.0),      # [0 / 0]: the same split
    ("convert_pad", "x3"): (1.6e-5, 4.2e-8), # [4.2e-6 / 1.1e-8]
    ("sinusoidal", "f32"): (2e-7, 4.8e-8),   # [5.2e-8 / 1.2e-8]
    ("sinusoidal", "mm3"): (2e-5, 4.1e-8),   # [7.6e-6 / 1.0e-8]
    ("sinusoidal", "x3"): (1.5e-5, 3.3e-6),  # [3.9e-6 / 8.4e-7]
    ("add_act", "f32"): (5e-7, 9.3e-8),      # [1.7e-7 / 2.3e-8]
    ("add_act", "mm3"): (2e-5, 1.3e-7),      # [6.1e-6 / 3.3e-8]
    ("add_act", "x3"): (2.3e-5, 1.1e-6),     # [5.8e-6 / 2.7e-7]
    ("step_prologue", "f32"): (1.5e-7, 1.6e-8),   # [4.4e-8 / 4.2e-9]
    ("step_prologue", "mm3"): (6e-6, 2e-8),       # [1.7e-6 / 4.9e-9]
    ("step_prologue", "x3"): (1.8e-5, 1.2e-6),    # [4.6e-6 / 3.1e-7]
}
LAUNCHERS = sorted({n for n, _ in BOUNDS})
# the whole guided denoiser evaluation against the oracle in float64, max-abs (f32 [3.8e-6], bf16x3 [3.7e-5])
FORWARD_BOUNDS = {"f32": 1e-5, "bf16x3": 1e-4}


# ---- the storage format ------------------------------------------------------------------------------------------------------------
def _np32(x):
    if torch.is_tensor(x):
        x = x.detach().cpu()
        x = x.numpy() if x.dtype == torch.float32 else x.to(torch.float32).numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


def bf16_bits(x):
    """float32 values -> uint16 bf16 bit patterns, round to nearest, ties to even (finite inputs)"""
    u = _np32(x).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    """uint16 bf16 bit patterns -> float32 values"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_rne(x):
    return bf16_value(bf16_bits(x))


def split(x):
    """float32 values -> (hi, lo) uint16 bit patterns"""
    x = _np32(x)
    hi = bf16_bits(x)
    return hi, bf16_bits(x - bf16_value(hi))


def encode(x):
    """float32 [..., K] (K % 4 == 0) -> the split storage as float32 bit patterns of the same shape: chunk [hi x4 | lo x4]"""
    x = _np32(x)
    if x.shape[-1] % 4:
        raise ValueError("encode: the last dimension must be a multiple of 4")
    hi, lo = split(x)
    q = x.shape[:-1] + (x.shape[-1] // 4, 4)
    return np.concatenate([hi.reshape(q), lo.reshape(q)], -1).view(np.float32).reshape(x.shape)


def parts(t):
    """split storage [..., K] (float32 bit patterns) -> (hi, lo) float64 arrays [..., K]"""
    t = _np32(t)
    q = t.view(np.uint16).reshape(t.shape[:-1] + (t.shape[-1] // 4, 8))
    hi = bf16_value(q[..., :4]).astype(np.float64).reshape(t.shape)
    lo = bf16_value(q[..., 4:]).astype(np.float64).reshape(t.shape)
    return hi, lo


def decode(t):
    """split storage -> float64 torch tensor hi + lo (exact)"""
    hi, lo = parts(t)
    return torch.from_numpy(hi + lo)


def non_canonical(t):
    """bool [..., K]: elements whose (hi, lo) no split of any float32 value produces.  hi must be a nearest bf16 of hi + lo (a tie is
    allowed: lo = bf16(v - hi) can round up to exactly half an ulp of hi while v itself was no tie) and lo a nearest bf16 of itself
    (always) -- so |lo| <= half an ulp of hi on the side lo points to."""
    hi, lo = parts(t)
    v = hi + lo
    r = bf16_rne(v.astype(np.float32)).astype(np.float64)          # v is exact in float32 when canonical (<= 17 significant bits)
    exact32 = v.astype(np.float32).astype(np.float64) == v
    tie = np.abs(v - hi) == np.abs(v - r)
    return ~exact32 | ((r != hi) & ~tie)


# ---- products --------------------------------------------------------------------------------------------------------------------
def _halves(x):
    hi, lo = split(x)
    shape = _np32(x).shape
    return (torch.from_numpy(bf16_value(hi).astype(np.float64).reshape(shape)),
            torch.from_numpy(bf16_value(lo).astype(np.float64).reshape(shape)))


def mm3(a, b, defect=None):
    """float32 values a [..., M, K], b [..., N, K] -> a_hi b_hi^T + a_hi b_lo^T + a_lo b_hi^T in float64"""
    ah, al = _halves(a)
    bh, bl = _halves(b)
    if defect == "w_lo":
        bl = torch.zeros_like(bl)
    if defect == "quad_swap":                                      # chunk 3 of every 32-element (128-byte) row segment
        k = torch.arange(ah.shape[-1])
        sw = ((k // 4) % 8) == 3
        ah, al = torch.where(sw, al, ah), torch.where(sw, ah, al)
    t = lambda u: u.transpose(-1, -2)                              # noqa: E731
    out = ah @ t(bh) + al @ t(bh)
    if defect != "cross":
        out = out + ah @ t(bl)
    return out


def f32(x):
    """a float64 value as the float32 the kernel holds"""
    return torch.as_tensor(x).to(torch.float32)


def _c(t):
    return t.detach().cpu().to(D)


def act64(v, act):
    from tcdiff_amd import _lib as L
    return {L.ACT_NONE: lambda u: u, L.ACT_RELU: F.relu, L.ACT_GELU: F.gelu, L.ACT_MISH: F.mish, L.ACT_SILU: F.silu}[act](v)


class Ref:
    def __init__(self, rounding=True, defect=None):
        if defect is not None and defect not in DEFECTS:
            raise ValueError(defect)
        self.rounding, self.defect = rounding, defect
        self.lr = LayerRef(rounding=False)

    def mm(self, a, b):
        """a [.., M, K] (x) b [.., N, K]^T: split-bf16 products of the float32 operands, or float64"""
        if self.rounding:
            return mm3(f32(a), f32(b), self.defect)
        return _c(a) @ _c(b).transpose(-1, -2)

    def store(self, v, tail_rows=None):
        """a split-format store of float64 values (the kernel's fp32 value, then hi + lo); tail_rows: bool [rows] of the last partial
        row block (tail_no_lo)"""
        if not self.rounding:
            return v
        hi, lo = _halves(f32(v))
        if self.defect == "act_lo":
            return hi
        if self.defect == "tail_no_lo" and tail_rows is not None:
            lo = torch.where(tail_rows.reshape(-1, *([1] * (lo.dim() - 1))), torch.zeros_like(lo), lo)
        return hi + lo

    # ---- gemm_tile -------------------------------------------------------------------------------------------------------------
    def gemm(self, A, W, M, *, bias=None, act=0, a_mod=0, A2=None, split_n=0, store=False, scale_cols=None):
        """C[M, N] = act(A[m % a_mod] W^T + bias) (columns >= split_n from A2); store: the split-format STORE_T output (row block 128)"""
        rows = torch.arange(M) % a_mod if a_mod else torch.arange(M)
        v = self.mm(A[rows], W)
        if A2 is not None:
            v[:, split_n:] = self.mm(A2[rows], W[split_n:])
        if bias is not None:
            v = v + _c(bias)
        v = act64(v, act)
        if scale_cols is not None:
            v = v * scale_cols
        if not store:
            return v
        tail = torch.arange(M) >= (M // 128) * 128
        return self.store(v, tail)

    def qkv_heads(self, A, W, Lq, nseq, *, A2=None, split_n=0, bias=None, scale_q=0.125, n_q=512):
        """the head-major Q / K / V token values [nseq, H, Lq, 64] per image of the QKV scatter (no hgroup); images in column order"""
        N = W.shape[0]
        sc = torch.ones(N, dtype=D)
        sc[:n_q] = scale_q
        v = self.gemm(A, W, nseq * Lq, bias=bias, A2=A2, split_n=split_n, store=True, scale_cols=sc)
        return [v[:, c:c + 512].reshape(nseq, Lq, 8, 64).permute(0, 2, 1, 3) for c in range(0, N, 512)]

    # ---- gemm_rowln ------------------------------------------------------------------------------------------------------------
    def rowln(self, A, W, M, *, a_mod=0, bias=None, ln=None, film=None, film_ld=0, xres=None, xres_mod=0, Lseq=1, nln=None,
              rope=None, out_mul=1, out_add=0, groups=1, store_h=False):
        """the epilogue chain of tcdiff_gemm_rowln: v = A W^T + bias; LN_POST (ln = (g, b, eps)); FILM ((scale + 1) v + shift of row
        m / Lseq, film [rows, film_ld]); + xres[m % xres_mod] (FILM or RES); x = v; NEXT_LN (nln) -> h; rotary -> rot.
        Returns {mo: output row indices, x, h, rot} per group concatenated (row block 64)"""
        rows = torch.arange(M) % a_mod if a_mod else torch.arange(M)
        out = {"mo": [], "x": [], "h": [], "rot": []}
        tail = torch.arange(M) >= (M // 64) * 64
        for g in range(groups):
            v = self.mm(A[rows], W[512 * g:512 * g + 512])
            if bias is not None:
                v = v + _c(bias[512 * g:512 * g + 512])
            if ln is not None:
                v = self.lr.ln(v, ln[0], ln[1], ln[2])
            m = torch.arange(M)
            if film is not None:
                fr = _c(film)[m // Lseq]
                v = (fr[:, :512] + 1) * v + fr[:, 512:1024]
            if xres is not None:
                v = _c(xres)[m % xres_mod if xres_mod else m] + v
            mo = m * out_mul + out_add + g
            out["mo"].append(mo)
            out["x"].append(v)
            u = v
            if nln is not None:
                u = self.lr.ln(v, nln[0], nln[1], nln[2])
                if rope is not None:
                    out["rot"].append(self.store(self.lr.rotate(u, rope, mo % Lseq), tail))
            if store_h:
                out["h"].append(self.store(u, tail))
        return {k: torch.cat(v) if v else None for k, v in out.items()}

    # ---- attention -------------------------------------------------------------------------------------------------------------
    def attention(self, q, k, v, Lk, n_shared=0):
        """q [nseq, H, Lq, 64], k / v [n_kv, H, >= Lk, 64] (float32 values of the images) -> O token rows [nseq Lq, 512]:
        S = q k^T, P = exp(S - max) unnormalised and split before P V, 1 / l last; the output split-stored (row block 32 per wave)"""
        nseq, H, Lq = q.shape[:3]
        kv = torch.tensor([0 if s < n_shared else s - n_shared + (1 if n_shared > 0 else 0) for s in range(nseq)])
        kk, vv = k[kv][:, :, :Lk], v[kv][:, :, :Lk]
        s = self.mm(q, kk)
        p = torch.exp(s - s.amax(-1, keepdim=True))
        den = p.sum(-1, keepdim=True)
        if self.rounding:
            ph, pl = _halves(f32(p))
            if self.defect == "p_hi":
                pl = torch.zeros_like(pl)
            vT = f32(vv.transpose(-1, -2))
            vh, vl = _halves(vT)
            t = lambda u: u.transpose(-1, -2)                      # noqa: E731
            o = ph @ t(vh) + pl @ t(vh) + (ph @ t(vl) if self.defect != "cross" else 0)
        else:
            o = p @ _c(vv)
        o = (o / den).permute(0, 2, 1, 3).reshape(nseq * Lq, H * 64)
        tail = (torch.arange(nseq * Lq) % Lq) >= (Lq // 128) * 128
        return self.store(o, tail)

    # ---- elementwise launchers -------------------------------------------------------------------------------------------------
    def ln_rot(self, x, g, b, eps, rope, pos):
        u = self.lr.ln(_c(x), g, b, eps)
        return {"y32": u, "h": self.store(u), "rot": self.store(self.lr.rotate(u, rope, pos))}

    def convert_pad(self, src, ld):
        v = torch.zeros(src.shape[0], ld, dtype=D)
        v[:, :src.shape[1]] = _c(src)
        return self.store(v)

    def sinusoidal(self, times, freq):
        ang = _c(times.cpu().to(torch.float32)[:, None] * freq.cpu()[None, :])         # the kernel's fp32 angle
        return self.store(torch.cat((ang.sin(), ang.cos()), -1))

    def add_act(self, a, ia, b, act):
        a = a.cpu()[ia.long().cpu()]
        v = (a + b.cpu() if self.rounding else _c(a) + _c(b)).to(D)        # the kernel's fp32 sum, then the activation
        v = act64(v, act)
        return {"out32": v, "out": self.store(v)}


# ---- regions ---------------------------------------------------------------------------------------------------------------------
def regions(M, N, *, row_block=128, seq_len=None):
    """(name, row mask or None, column slice): the whole tensor, the rows of the last partial row block (of every sequence of
    seq_len rows, or of the launch), every 128-column block, and the last partial column chunk (N % 4) when there is one"""
    out = [("all", None, slice(0, N))]
    pos = torch.arange(M) % seq_len if seq_len else torch.arange(M)
    Lr = seq_len if seq_len else M
    if Lr % row_block:
        out.append(("tail", pos >= (Lr // row_block) * row_block, slice(0, N)))
    if N > 128:
        out += [(f"cols{j}", None, slice(128 * j, min(N, 128 * j + 128))) for j in range((N + 127) // 128)]
    if N % 4:
        out.append(("chunk", None, slice(N - N % 4, N)))
    return out


def region_stats(got, ref, regs):
    """{region: (max-abs, mean-abs) / top magnitude of ref} of got - ref over the regions"""
    got, ref = _c(got).reshape(ref.shape[0], -1), _c(ref).reshape(ref.shape[0], -1)
    top = float(ref.abs().max()) or 1.0
    d = (got - ref).abs() / top
    st = {}
    for name, rows, cols in regs:
        part = d[:, cols] if rows is None else d[rows][:, cols]
        if part.numel():
            st[name] = (float(part.max()), float(part.mean()))
    return st


def worst(stats):
    return max(v[0] for v in stats.values()), max(v[1] for v in stats.values())


# ---- test data -------------------------------------------------------------------------------------------------------------------
def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def freqs512():
    return 1.0 / (10000 ** (torch.arange(0, 512, 2).float() / 512))


def rope_f32(n_pos):
    """the float32 rotary table [n_pos, 512] (cos, sin) of tcdiff_rope_table's fp32 angle; float64 of the same angles"""
    ang = (torch.arange(n_pos, dtype=torch.float32)[:, None] * freqs512()[None, :]).to(D)
    return torch.stack((ang.cos(), ang.sin()), -1).reshape(n_pos, 512).to(torch.float32)


def sin_freq():
    return torch.exp(torch.arange(256) * -(math.log(10000) / 255)).to(torch.float32)
