"""The two parity modes launcher by launcher against float64 (MI355X only): compute_dtype "f32" (exact fp32 MFMA) and "bf16x3" (fp32
storage, every product as three bf16 MFMAs on (hi, lo) splits, csrc/common.h MmaBF16x3), against tests/x3_ref.py.

For every launcher of the sampler's op-by-op path, both modes, region by region (the whole tensor, the last partial row block, each
128-column block, the last partial column chunk; max-abs and mean-abs scaled by the reference's top magnitude):

  * bf16x3 against the split-bf16 model of the same arithmetic (x3_ref.Ref(rounding=True)): only the fp32 summation order differs;
  * bf16x3 and f32 against the float64 evaluation of the fp32 inputs (Ref(rounding=False)): the parity budget.  Every f32 bound sits
    below the smallest bf16x3 error of the same case, so an f32 launcher that fell back to split-bf16 arithmetic fails.

Split-format outputs are read back through x3_ref.decode and must be canonical splits; padding is zero in both halves, and nothing
is written outside the addressed block.  convert_pad in bf16x3 must equal the host packer kernels.to_x3 bit for bit.  Last, one whole
guided denoiser evaluation per mode against the oracle in float64, on the op-by-op path.

Every split-bf16 k-loop reached here walks its k-steps in pairs (MmaBF16x3::mma2): K is a multiple of 32 (two pairs per 32-element
staged row) in gemm_tile / gemm_rowln, and attention's d = 64 and 32-key tiles are even in k-steps.  The single-k-step
MmaBF16x3::mma (odd tails) is not reachable from any launcher, so no test here can cover it."""
import math

import pytest
import torch
import torch.nn.functional as F

import x3_ref as XR

pytestmark = pytest.mark.gpu

from tcdiff_amd import _lib as L  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402

DEV = "cuda"
X3, F32 = L.DT_BF16X3, L.DT_F32
MODES = {F32: "f32", X3: "bf16x3"}

BOUNDS, FORWARD_BOUNDS = XR.BOUNDS, XR.FORWARD_BOUNDS

WORST = {}


def rnd(seed, *shape, scale=1.0):
    return XR.rnd(seed, *shape, scale=scale)


def operand(x, dt):
    """a float32 CPU tensor as the device operand of mode dt (bf16x3: the split image, packed by the reference's own encoder)"""
    if dt == X3:
        return torch.from_numpy(XR.encode(x)).to(DEV)
    return x.to(DEV)


def values(t, dt):
    """a T-typed device output as float64 values"""
    t = t.detach().cpu().contiguous()
    return XR.decode(t) if dt == X3 else t.to(torch.float64)


def assert_canonical(t, what):
    bad = XR.non_canonical(t.detach().cpu().contiguous())
    assert not bad.any(), f"{what}: {int(bad.sum())} elements are not a canonical (hi, lo) split"


def check(name, dt, got, ref64, mm3=None, regs=None):
    """compare got (float64 values) region by region; returns the stats against float64"""
    got = got.reshape(ref64.shape[0], -1)
    ref64 = ref64.reshape(ref64.shape[0], -1)
    regs = regs if regs is not None else XR.regions(ref64.shape[0], ref64.shape[1])
    out = {}
    kinds = [("x3" if dt == X3 else "f32", ref64)] + ([("mm3", mm3.reshape(ref64.shape[0], -1))] if dt == X3 and mm3 is not None
                                                      else [])
    for kind, ref in kinds:
        st = XR.region_stats(got, ref, regs)
        out[kind] = st
        bmax, bmean = BOUNDS[(name, kind)]
        w = WORST.setdefault((name, kind), {})
        for reg, (mx, mn) in st.items():
            pm, pn = w.get(reg, (0.0, 0.0))
            w[reg] = (max(pm, mx), max(pn, mn))
        print(f"{name:13s} {MODES[dt]:6s} vs {'float64' if kind != 'mm3' else 'mm3':7s} " +
              " ".join(f"{r}={mx:.2e}/{mn:.2e}" for r, (mx, mn) in st.items()))
        for reg, (mx, mn) in st.items():
            assert mx <= bmax and mn <= bmean, (name, MODES[dt], kind, reg, mx, mn, (bmax, bmean))
    return out


def separated(name, x3_stats):
    """the f32 bound of `name` lies below the smallest bf16x3 error (whole tensor, against float64) of the same case"""
    e = x3_stats["x3"]["all"][0]
    assert BOUNDS[(name, "f32")][0] < e, (name, BOUNDS[(name, "f32")][0], e)


# ---- gemm_tile ---------------------------------------------------------------------------------------------------------------------
GEMM_CASES = [(1, 512, 512, L.ACT_GELU), (2, 150, 192, L.ACT_NONE), (127, 1024, 1024, L.ACT_RELU), (129, 640, 2048, L.ACT_SILU),
              (450, 1536, 512, L.ACT_MISH), (14400, 512, 512, L.ACT_GELU), (300, 438, 896, L.ACT_RELU)]


@pytest.mark.parametrize("M,N,Kd,act", GEMM_CASES)
def test_gemm_tile_store_f32_and_t(M, N, Kd, act):
    """N = 150 and 438 (the music features' cond_projection.0, engine.encode_music) end in a partial chunk: in the split format its
    elements' hi and lo halves are written one by one and the halves of the columns past N keep what was there"""
    A, W, bias = rnd(1, M, Kd), rnd(2, N, Kd, scale=1 / math.sqrt(Kd)), rnd(3, N)
    r64, r3 = XR.Ref(False), XR.Ref(True)
    ref = r64.gemm(A, W, M, bias=bias, act=act)
    mm3_f = r3.gemm(A, W, M, bias=bias, act=act)
    mm3_t = r3.gemm(A, W, M, bias=bias, act=act, store=True)
    Np = K.round_up(N, 4)
    regs = XR.regions(M, N)
    stats = {}
    for dt in (X3, F32):
        for mode, name in ((L.EPI_STORE_F32, "gemm_f32"), (L.EPI_STORE_T, "gemm_t")):
            ldc = Np + 4
            out = torch.full((M + 1, ldc), 7.0, device=DEV)
            K.gemm_tile(dt, operand(A, dt), operand(W, dt), M, N, Kd, bias=bias.to(DEV), act=act, mode=mode, out=out, ldc=ldc)
            torch.cuda.synchronize()
            o = out.cpu()
            assert bool((o[:M, Np:] == 7.0).all()) and bool((o[M] == 7.0).all()), "wrote outside the M x N block"
            split_t = dt == X3 and mode == L.EPI_STORE_T
            if split_t and N % 4:
                halves = o[:M, Np - 4:Np].contiguous().view(torch.int16)
                sent = torch.full((1, 4), 7.0).view(torch.int16)
                for t in range(N % 4, 4):
                    assert torch.equal(halves[:, t], sent[:, t].expand(M)) and torch.equal(halves[:, 4 + t], sent[:, 4 + t].expand(M)), \
                        "a partial split chunk wrote the halves of a column past N"
            elif N % 4:
                assert bool((o[:M, N:Np] == 7.0).all()), "wrote outside the M x N block"
            t = o[:M, :Np] if split_t else o[:M, :N]
            if split_t:
                bad = XR.non_canonical(t.contiguous())[:, :N]
                assert not bad.any(), f"gemm_tile STORE_T: {int(bad.sum())} elements are not a canonical split"
            got = values(t, dt)[:, :N] if mode == L.EPI_STORE_T else t.double()
            stats[(dt, name)] = check(name, dt, got, ref, mm3_t if mode == L.EPI_STORE_T else mm3_f, regs)
    separated("gemm_f32", stats[(X3, "gemm_f32")])
    separated("gemm_t", stats[(X3, "gemm_t")])


def test_gemm_tile_split_and_amod():
    M, Kd, N, a_mod = 260, 192, 512, 100
    A1, A2, W = rnd(4, a_mod, Kd), rnd(5, a_mod, Kd), rnd(6, N, Kd, scale=1 / math.sqrt(Kd))
    kw = dict(a_mod=a_mod, A2=A2, split_n=256)
    ref, mm3 = XR.Ref(False).gemm(A1, W, M, **kw), XR.Ref(True).gemm(A1, W, M, **kw)
    st = {}
    for dt in (X3, F32):
        out = torch.full((M, N), 7.0, device=DEV)
        K.gemm_tile(dt, operand(A1, dt), operand(W, dt), M, N, Kd, A2=operand(A2, dt), split_n=256, a_mod=a_mod,
                    mode=L.EPI_STORE_F32, out=out, ldc=N)
        st[dt] = check("gemm_split", dt, out.cpu().double(), ref, mm3)
    separated("gemm_split", st[X3])


@pytest.mark.parametrize("Lq,nseq,Lp,tok_off,seq_off", [(70, 3, 128, 2, 1), (150, 2, 256, 0, 0)])
def test_gemm_tile_qkv_heads(Lq, nseq, Lp, tok_off, seq_off):
    H, Kd, M = 8, 512, nseq * Lq
    A1, A2 = rnd(7, M, Kd), rnd(8, M, Kd)
    W, bias = rnd(9, 1536, Kd, scale=1 / math.sqrt(Kd)), rnd(10, 1536)
    kw = dict(A2=A2, split_n=1024, bias=bias, scale_q=0.125, n_q=512)
    ref, mm3 = XR.Ref(False).qkv_heads(A1, W, Lq, nseq, **kw), XR.Ref(True).qkv_heads(A1, W, Lq, nseq, **kw)
    st = {}
    for dt in (X3, F32):
        imgs = [torch.full((nseq + seq_off + 1, H, Lp, 64), 7.0, device=DEV) for _ in range(3)]
        K.gemm_tile(dt, operand(A1, dt), operand(W, dt), M, 1536, Kd, A2=operand(A2, dt), split_n=1024, bias=bias.to(DEV),
                    mode=L.EPI_QKV_HEADS, out=imgs[0], out_k=imgs[1], out_v=imgs[2], scale_q=0.125, Lseq=Lq, Lp=Lp, H=H, n_q=512,
                    n_k=512, tok_off=tok_off, seq_off=seq_off)
        torch.cuda.synchronize()
        got, r64, r3 = [], [], []
        for img, a, b in zip(imgs, ref, mm3):
            img = img.cpu()
            blk = img[seq_off:seq_off + nseq, :, tok_off:tok_off + Lq]
            keep = torch.ones_like(img, dtype=torch.bool)
            keep[seq_off:seq_off + nseq, :, tok_off:tok_off + Lq] = False
            assert bool((img[keep] == 7.0).all()), "the QKV scatter wrote outside its block"
            if dt == X3:
                assert_canonical(blk, "QKV image")
            got.append(values(blk, dt).permute(0, 2, 1, 3).reshape(M, 512))
            r64.append(a.permute(0, 2, 1, 3).reshape(M, 512))
            r3.append(b.permute(0, 2, 1, 3).reshape(M, 512))
        cat = lambda xs: torch.cat(xs, 1)                          # noqa: E731
        st[dt] = check("qkv", dt, cat(got), cat(r64), cat(r3), XR.regions(M, 1536))
    separated("qkv", st[X3])


# ---- gemm_rowln --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kd", [512, 1024])
def test_gemm_rowln_full_chain(Kd):
    """bias -> LN_POST -> FILM -> + residual -> x; NEXT_LN -> h, rotary -> rot (the decoder layer's fc epilogue)"""
    Lq, nseq = 90, 3
    M = nseq * Lq
    A, W, bias = rnd(20, M, Kd), rnd(21, 512, Kd, scale=1 / math.sqrt(Kd)), rnd(22, 512)
    g1, b1, g2, b2 = 1 + 0.1 * rnd(23, 512), 0.1 * rnd(24, 512), 1 + 0.1 * rnd(25, 512), 0.1 * rnd(26, 512)
    film, xres, rope = rnd(27, nseq, 1024, scale=0.5), rnd(28, M, 512), XR.rope_f32(Lq)
    kw = dict(bias=bias, ln=(g1, b1, 1e-6), film=film, xres=xres, Lseq=Lq, nln=(g2, b2, 1e-5), rope=rope, store_h=True)
    ref, mm3 = XR.Ref(False).rowln(A, W, M, **kw), XR.Ref(True).rowln(A, W, M, **kw)
    regs = XR.regions(M, 512, row_block=64)
    st = {}
    for dt in (X3, F32):
        xout = torch.full((M, 512), 7.0, device=DEV)
        h, r = torch.full((M, 512), 7.0, device=DEV), torch.full((M, 512), 7.0, device=DEV)
        K.gemm_rowln(dt, operand(A, dt), operand(W, dt), M, Kd, bias=bias.to(DEV), ln_g=g1.to(DEV), ln_b=b1.to(DEV), ln_eps=1e-6,
                     film=film.to(DEV), film_ld=1024, xres=xres.to(DEV), xout=xout, Lseq=Lq, nln_g=g2.to(DEV), nln_b=b2.to(DEV),
                     nln_eps=1e-5, hout=h, rout=r, rope=rope.to(DEV),
                     flags=L.ROW_BIAS | L.ROW_LN_POST | L.ROW_FILM | L.ROW_STORE_X | L.ROW_NEXT_LN | L.ROW_STORE_H | L.ROW_STORE_ROT)
        torch.cuda.synchronize()
        if dt == X3:
            assert_canonical(h.cpu(), "rowln h")
            assert_canonical(r.cpu(), "rowln rot")
        got = torch.cat([xout.cpu().double(), values(h, dt), values(r, dt)], 1)
        cat = lambda d: torch.cat([d["x"], d["h"], d["rot"]], 1)   # noqa: E731
        st[dt] = check("rowln", dt, got, cat(ref), cat(mm3), regs + [("x", None, slice(0, 512)), ("h", None, slice(512, 1024)),
                                                                       ("rot", None, slice(1024, 1536))])
    separated("rowln", st[X3])


def test_gemm_rowln_shared_rows_out_mul_and_groups():
    """a_mod / xres_mod (a guided layer 0's shared rows), out_mul / out_add (the fusion projection's interleaved rows), groups"""
    M, Kd, G = 200, 512, 3
    A, W, bias = rnd(30, M, Kd), rnd(31, G * 512, Kd, scale=1 / math.sqrt(Kd)), rnd(32, G * 512)
    xres = rnd(33, 100, 512)
    g2, b2, rope = 1 + 0.1 * rnd(36, 512), 0.1 * rnd(37, 512), XR.rope_f32(60)
    st = {}
    for dt in (X3, F32):
        # residual with modulo rows + plain T copy
        kw = dict(a_mod=150, bias=bias[:512], xres=xres, xres_mod=100, Lseq=50, store_h=True)
        ref, mm3 = XR.Ref(False).rowln(A, W[:512], M, **kw), XR.Ref(True).rowln(A, W[:512], M, **kw)
        xout, h = torch.full((M, 512), 7.0, device=DEV), torch.full((M, 512), 7.0, device=DEV)
        K.gemm_rowln(dt, operand(A, dt), operand(W[:512], dt), M, Kd, bias=bias[:512].to(DEV), xres=xres.to(DEV), xres_mod=100,
                     a_mod=150, xout=xout, hout=h, Lseq=50, flags=L.ROW_BIAS | L.ROW_RES | L.ROW_STORE_X | L.ROW_STORE_H)
        if dt == X3:
            assert_canonical(h.cpu(), "rowln h (shared rows)")
        st[dt] = check("rowln", dt, torch.cat([xout.cpu().double(), values(h, dt)], 1), torch.cat([ref["x"], ref["h"]], 1),
                       torch.cat([mm3["x"], mm3["h"]], 1), XR.regions(M, 1024, row_block=64))
        # grouped, interleaved output rows, next LN + rotary
        kw = dict(bias=bias, Lseq=60, nln=(g2, b2, 1e-5), rope=rope, out_mul=G, groups=G, store_h=True)
        ref, mm3 = XR.Ref(False).rowln(A, W, M, **kw), XR.Ref(True).rowln(A, W, M, **kw)
        xg = torch.full((G * M, 512), 7.0, device=DEV)
        hg, rg = torch.full((G * M, 512), 7.0, device=DEV), torch.full((G * M, 512), 7.0, device=DEV)
        K.gemm_rowln(dt, operand(A, dt), operand(W, dt), M, Kd, bias=bias.to(DEV), xout=xg, hout=hg, rout=rg, Lseq=60,
                     nln_g=g2.to(DEV), nln_b=b2.to(DEV), nln_eps=1e-5, rope=rope.to(DEV), out_mul=G, groups=G,
                     flags=L.ROW_BIAS | L.ROW_STORE_X | L.ROW_NEXT_LN | L.ROW_STORE_H | L.ROW_STORE_ROT)
        mo = ref["mo"]
        got = torch.cat([xg.cpu().double()[mo], values(hg, dt)[mo], values(rg, dt)[mo]], 1)
        cat = lambda d: torch.cat([d["x"], d["h"], d["rot"]], 1)   # noqa: E731
        check("rowln", dt, got, cat(ref), cat(mm3), XR.regions(G * M, 1536, row_block=64))
    separated("rowln", st[X3])


# ---- attention ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk,nseq,n_shared,gain", [(450, 450, 3, 0, 1.0), (450, 152, 4, 2, 1.0), (120, 62, 2, 1, 1.0),
                                                      (150, 150, 2, 0, 3.0), (513, 1025, 1, 0, 1.0), (60, 77, 2, 0, 4.0)])
def test_attention(Lq, Lk, nseq, n_shared, gain):
    """gain scales Q: at 3 and 4 the logits reach tens, the running max moves across key tiles (online-softmax rescale)"""
    H = 8
    Lpq, Lpk = K.round_up(Lq, 128), K.round_up(Lk, 128)
    n_kv = nseq if n_shared == 0 else nseq - n_shared + 1
    q = rnd(40, nseq, H, Lq, 64, scale=0.5 * gain)
    k, v = rnd(41, n_kv, H, Lk, 64), rnd(42, n_kv, H, Lk, 64)
    if gain > 1:
        k[:, :, Lk - 3] = 2.0 * q[0, :, 5].unsqueeze(0)            # one dominant key in the last, partial tile
    ref, mm3 = XR.Ref(False).attention(q, k, v, Lk, n_shared), XR.Ref(True).attention(q, k, v, Lk, n_shared)
    pad = lambda x, Lp: F.pad(x, (0, 0, 0, Lp - x.shape[2]))       # noqa: E731
    st = {}
    for dt in (X3, F32):
        O = torch.full((nseq * Lq + 1, 512), 7.0, device=DEV)
        K.attention(dt, operand(pad(q, Lpq), dt), operand(pad(k, Lpk), dt), operand(pad(v, Lpk), dt), O, nseq, H, Lq, Lk, Lpq,
                    Lpk, 512, n_shared=n_shared)
        o = O.cpu()
        assert bool((o[-1] == 7.0).all()), "attention wrote past its rows"
        if dt == X3:
            assert_canonical(o[:-1], "attention O")
        st[dt] = check("attention", dt, values(o[:-1], dt), ref, mm3, XR.regions(nseq * Lq, 512, row_block=128, seq_len=Lq))
    separated("attention", st[X3])


# ---- elementwise launchers ---------------------------------------------------------------------------------------------------------
def test_ln_rot():
    rows, Lq = 333, 50
    x = rnd(11, rows, 512, scale=3.0) + 0.7
    g, b = 1 + 0.1 * rnd(12, 512), 0.1 * rnd(13, 512)
    rope = XR.rope_f32(64)
    pos = torch.arange(rows) % Lq + 3
    ref, mm3 = XR.Ref(False).ln_rot(x, g, b, 1e-5, rope, pos), XR.Ref(True).ln_rot(x, g, b, 1e-5, rope, pos)
    st = {}
    for dt in (X3, F32):
        h, r = torch.full((rows, 512), 7.0, device=DEV), torch.full((rows, 512), 7.0, device=DEV)
        y = torch.full((rows, 512), 7.0, device=DEV)
        K.ln_rot(dt, x.to(DEV), rows, g.to(DEV), b.to(DEV), 1e-5, h=h, rot=r, y32=y, rope=rope.to(DEV), pos_mod=Lq, pos_base=3)
        torch.cuda.synchronize()
        if dt == X3:
            assert_canonical(h.cpu(), "ln_rot h")
            assert_canonical(r.cpu(), "ln_rot rot")
        # y32 is fp32 in both modes: held to the f32 bound
        check("ln_rot", F32, y.cpu().double(), ref["y32"])
        got = torch.cat([values(h, dt), values(r, dt)], 1)
        st[dt] = check("ln_rot", dt, got, torch.cat([ref["h"], ref["rot"]], 1), torch.cat([mm3["h"], mm3["rot"]], 1))
    separated("ln_rot", st[X3])


def _ties(n, seed):
    """float32 values with exact bf16 ties (both parities of hi), values whose hi rounds into the next binade, and random values"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0x3C00, 0x4400, (n,), generator=g, dtype=torch.int32)
    u = base << 16
    kind = torch.arange(n) % 4
    u = torch.where(kind == 0, u | 0x8000, u)                      # hi + half an ulp: a tie, even or odd hi
    u = torch.where(kind == 1, (u | 0x7FFF) | 0x007F0000, u)      # mantissa all ones: rounds up into the next binade
    f = u.view(torch.float32)
    f = torch.where(kind == 2, torch.randn(n, generator=g) * 10.0 ** torch.randint(-8, 8, (n,), generator=g).float(), f)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return f * sign


def test_convert_pad_equals_the_host_packer_and_pads_with_zero():
    B, S, Cd, ld = 3, 10, 438, 880
    cond = _ties(B * (2 * S + 1) * Cd, 50).reshape(B, 2 * S + 1, Cd)
    src = cond[:, :-1].reshape(B * S, 2 * Cd)
    for dt in (X3, F32):
        dst = torch.full((B * S + 1, ld), 7.0, device=DEV)
        K.convert_pad(dt, cond.to(DEV), dst, B * S, 2 * Cd, ld, rows_per_batch=S, batch_stride=(2 * S + 1) * Cd, row_stride=2 * Cd)
        d = dst.cpu()
        assert bool((d[-1] == 7.0).all()), "convert_pad wrote past its rows"
        d = d[:-1]
        if dt == X3:
            want = K.to_x3(F.pad(src, (0, ld - 2 * Cd)))
            assert torch.equal(d.view(torch.int32), want.view(torch.int32)), "device split != host packer"
            assert torch.equal(d.view(torch.int32), torch.from_numpy(XR.encode(F.pad(src, (0, ld - 2 * Cd)))).view(torch.int32))
            assert int(d[:, 2 * Cd:].view(torch.int32).abs().max()) == 0, "padding not zero in both halves"
            assert_canonical(d, "convert_pad")
        else:
            assert torch.equal(d[:, :2 * Cd], src) and float(d[:, 2 * Cd:].abs().max()) == 0
        check("convert_pad", dt, values(d, dt), XR.Ref(False).convert_pad(src, ld), XR.Ref(True).convert_pad(src, ld))


def test_sinusoidal_and_add_act():
    times = torch.tensor([0, 1, 37, 500, 999, 20], dtype=torch.int32)
    f = XR.sin_freq()
    a, bb = rnd(52, 5, 512), rnd(53, 6, 512)
    ia = torch.tensor([4, 0, 0, 2, 1, 3], dtype=torch.int32)
    for dt in (X3, F32):
        emb = torch.full((7, 512), 7.0, device=DEV)
        K.sinusoidal(dt, times.to(DEV), 6, f.to(DEV), emb)
        e = emb.cpu()
        assert bool((e[-1] == 7.0).all())
        if dt == X3:
            assert_canonical(e[:-1], "sinusoidal")
        check("sinusoidal", dt, values(e[:-1], dt), XR.Ref(False).sinusoidal(times, f), XR.Ref(True).sinusoidal(times, f))
        for act in (L.ACT_MISH, L.ACT_SILU, L.ACT_GELU):
            o, o32 = torch.full((7, 512), 7.0, device=DEV), torch.full((7, 512), 7.0, device=DEV)
            K.add_act(dt, a.to(DEV), ia.to(DEV), bb.to(DEV), 6, act, out=o, out32=o32)
            o, o32 = o.cpu(), o32.cpu()
            assert bool((o[-1] == 7.0).all()) and bool((o32[-1] == 7.0).all())
            ref, mm3 = XR.Ref(False).add_act(a, ia, bb, act), XR.Ref(True).add_act(a, ia, bb, act)
            if dt == X3:
                assert_canonical(o[:-1], "add_act")
            check("add_act", F32, o32[:-1].double(), ref["out32"])
            check("add_act", dt, values(o[:-1], dt), ref["out"], mm3["out"])


def test_scatter_time_kv_and_step_prologue():
    """the time-token rows move as whole split chunks (bit for bit); step_prologue's FiLM input is mish(t_base[t] + hidden) split, its
    x copy the split of x with the ld_xin pad zero in both halves; nothing else of the caches is touched"""
    NL, n_t, n_kv, H, Lp, S, n_seq, rows, nf, ld = 2, 5, 3, 8, 128, 60, 3, 130, 151, 192
    tab32 = rnd(60, NL, n_t, 2, 1024)
    t_base, hidden, x = rnd(61, n_t, 512), rnd(62, n_seq, 512), rnd(63, rows, nf)
    tseq = torch.tensor([4, 2], dtype=torch.int32)
    for dt in (X3, F32):
        tab = operand(tab32, dt)
        tidx = torch.tensor([4, 0, 2], dtype=torch.int32, device=DEV)
        Kc = torch.full((NL, n_kv, H, Lp, 64), 7.0, device=DEV)
        Vc = Kc.clone()
        K.scatter_time_kv(dt, tab, n_t, tidx, Kc, Vc, NL, n_kv, H, Lp, S)
        tb = tab.cpu().reshape(NL, n_t, 2, 2, 8, 64)
        Kh, Vh = Kc.cpu(), Vc.cpu()
        for s in range(n_kv):
            t = int(tidx[s])
            for rr in range(2):
                assert torch.equal(Kh[:, s, :, S + rr].view(torch.int32), tb[:, t, rr, 0].view(torch.int32))
                assert torch.equal(Vh[:, s, :, S + rr].view(torch.int32), tb[:, t, rr, 1].view(torch.int32))
        keep = torch.ones_like(Kh, dtype=torch.bool)
        keep[:, :, :, S:S + 2] = False
        assert bool((Kh[keep] == 7.0).all()) and bool((Vh[keep] == 7.0).all())

        counter = torch.zeros(8, dtype=torch.int32, device=DEV)
        film_in = torch.full((n_seq + 1, 512), 7.0, device=DEV)
        xin = torch.full((rows + 1, ld), 7.0, device=DEV)
        tid = torch.zeros(n_seq, dtype=torch.int32, device=DEV)
        Kc.fill_(7.0)
        Vc.fill_(7.0)
        K.step_prologue(dt, counter, tseq.to(DEV), tid, t_base.to(DEV), hidden.to(DEV), film_in, n_seq, tab, n_t, Kc, Vc, None, None,
                        NL, n_kv, H, Lp, 0, S, x.to(DEV), xin, rows, nf, ld)
        torch.cuda.synchronize()
        t = int(tseq[0])
        assert tid.cpu().tolist() == [t] * n_seq
        fi, xi = film_in.cpu(), xin.cpu()
        assert bool((fi[-1] == 7.0).all()) and bool((xi[-1] == 7.0).all())
        fi, xi = fi[:-1], xi[:-1]
        for kv in range(n_kv):
            assert torch.equal(Kc.cpu()[:, kv, :, S].view(torch.int32), tb[:, t, 0, 0].view(torch.int32))
        v = (t_base[t][None] + hidden).double()
        r64 = XR.act64(v, L.ACT_MISH)
        r3 = XR.Ref(True).store(XR.act64((t_base[t][None] + hidden).to(torch.float64), L.ACT_MISH))
        check("step_prologue", dt, values(fi, dt), r64, r3)
        xr64, xr3 = XR.Ref(False).convert_pad(x, ld), XR.Ref(True).convert_pad(x, ld)
        check("step_prologue", dt, values(xi, dt), xr64, xr3, XR.regions(rows, ld))
        if dt == X3:
            assert_canonical(fi, "step_prologue film_in")
            assert_canonical(xi, "step_prologue xin")
            assert int(xi[:, nf + 1:].view(torch.int32).abs().max()) == 0, "the ld_xin pad is not zero in both halves"
            assert torch.equal(xi.view(torch.int32), K.to_x3(F.pad(x, (0, ld - nf))).view(torch.int32))


# ---- refused combinations ----------------------------------------------------------------------------------------------------------
def test_refused_combinations():
    a = torch.zeros(256, 256, device=DEV)
    with pytest.raises(L.TcdiffError):                            # x3 has no split-K
        L.check(L.load().tcdiff_gemm_splitk(X3, a.data_ptr(), a.data_ptr(), 64, 64, 64, 64, 64, a.data_ptr(), 64, 2,
                                            K.stream()), "splitk")
    with pytest.raises(L.TcdiffError):                            # nor the training step's fused epilogues
        K.gemm_tile(X3, a, a, 64, 64, 64, mode=L.EPI_STORE_T, out=a, ldc=64, out2=a, ldc2=64)
    with pytest.raises(L.TcdiffError):
        K.gemm_tile(X3, a, a, 64, 64, 64, mode=L.EPI_STORE_T, out=a, ldc=64, act_src=a, ld_src=64)
    with pytest.raises(L.TcdiffError):                            # K % 32
        K.gemm_tile(X3, a, a, 64, 64, 48, mode=L.EPI_STORE_F32, out=a, ldc=64)
    with pytest.raises(L.TcdiffError):
        K.gemm_rowln(X3, a, a, 64, 48, flags=L.ROW_STORE_X, xout=a, Lseq=1)
    with pytest.raises(L.TcdiffError):                            # split-format rows must hold whole chunks
        K.convert_pad(X3, a, a, 8, 10, 14)
    with pytest.raises(L.TcdiffError):
        z = torch.zeros(64, dtype=torch.int32, device=DEV)
        K.step_prologue(X3, z, z, z, a, a, a, 1, a, 1, a, a, None, None, 1, 1, 8, 128, 0, 0, a, a, 2, 10, 14)
    # STORE_T of the split format: a row stride that would start a row inside a chunk
    for N, ldc in ((152, 154), (150, 150), (151, 151)):
        out = torch.full((64, 256), 7.0, device=DEV)
        with pytest.raises(L.TcdiffError):
            K.gemm_tile(X3, a, a, 64, N, 64, mode=L.EPI_STORE_T, out=out, ldc=ldc)
        assert bool((out.cpu() == 7.0).all())
    # ... which f32 keeps (an element per 4-byte slot)
    out = torch.full((64, 256), 7.0, device=DEV)
    K.gemm_tile(F32, a, a, 64, 150, 64, mode=L.EPI_STORE_T, out=out, ldc=154)
    o = out.cpu().reshape(-1)[:64 * 154].reshape(64, 154)           # rows of ldc = 154
    assert float(o[:, :150].abs().max()) == 0 and bool((o[:, 150:] == 7.0).all())


# ---- one whole denoiser evaluation per mode ----------------------------------------------------------------------------------------
def _oracle_f64(monkeypatch, sd, xT, cond, tt):
    """oracle.guided_forward on the float64 copy of the weights: inputs are cast to the weight's dtype at every linear (the oracle
    casts the music features to float32 first, exactly), and the timestep embedding takes sin / cos in float64 of the float32 angle"""
    from oracle import tcdiff_oracle as O
    lin = O.linear

    def s64(times, dim):
        half = dim // 2
        f = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
        e = (times[:, None] * f[None, :]).to(torch.float64)
        return torch.cat((e.sin(), e.cos()), dim=-1)
    with monkeypatch.context() as m:
        m.setattr(O, "linear", lambda x, sd_, prefix, bias=True: lin(x.to(sd_[prefix + ".weight"].dtype), sd_, prefix, bias))
        m.setattr(O, "sinusoidal_emb", s64)
        sd64 = {k: (v.to(torch.float64) if v.is_floating_point() else v) for k, v in sd.items()}
        return O.guided_forward(sd64, xT.to(torch.float64), cond.to(torch.float64), tt, 2)


@pytest.mark.parametrize("dn,S", [(2, 60), (3, 150)])
def test_whole_guided_forward_against_the_oracle_in_float64(monkeypatch, dn, S):
    from oracle import tcdiff_oracle as O
    from tcdiff_amd.model import DanceDecoder
    sd = O.synth_state_dict(dn=dn, seq_len=S)
    cond = torch.stack([O.synth_cond(c, S) for c in (0, 1)])
    xT = torch.stack([O.synth_xT(c, dn * S) for c in (0, 1)])
    tt = torch.tensor([500, 20])
    ref = _oracle_f64(monkeypatch, sd, xT, cond, tt)
    Lq = dn * S
    regs = [("all", None, slice(0, 151)), ("tail", (torch.arange(2 * Lq) % Lq) >= (Lq // 16) * 16, slice(0, 151))]
    regs += [(f"dancer{d}", (torch.arange(2 * Lq) % dn) == d, slice(0, 151)) for d in range(dn)]
    regs += [("contact", None, slice(0, 4)), ("root", None, slice(4, 7)), ("rot6d", None, slice(7, 151)),
             ("cols1", None, slice(128, 151)), ("chunk", None, slice(148, 151))]
    errs = {}
    for compute in ("f32", "bf16x3"):
        model = DanceDecoder(nfeats=151, seq_len=S, latent_dim=512, ff_size=1024, num_layers=8, num_heads=8, dropout=0.1,
                             cond_feature_dim=438, activation=F.gelu, required_dancer_num=dn, compute_dtype=compute).to(DEV).eval()
        model.load_state_dict(sd, strict=True)
        got = model.guided_forward(xT.to(DEV), cond.to(DEV), tt.to(DEV), 2)
        assert not model.engine(2).use_chain
        d = (got.detach().cpu().double() - ref).reshape(2 * Lq, 151).abs()
        st = {n: float((d[:, c] if r is None else d[r][:, c]).max()) for n, r, c in regs}
        errs[compute] = st
        print(f"whole guided forward {dn}x{S} [{compute}] max-abs vs float64 oracle: " +
              " ".join(f"{n}={v:.2e}" for n, v in st.items()))
        WORST.setdefault(("forward", compute), {})[f"{dn}x{S}"] = (st["all"], 0.0)
        assert max(st.values()) <= FORWARD_BOUNDS[compute], (compute, st)
    assert FORWARD_BOUNDS["f32"] < errs["bf16x3"]["all"], errs


def test_zz_report_worst():
    """the worst error per launcher, check and region over this module's run"""
    for (name, kind), w in sorted(WORST.items()):
        print(f"WORST {name:13s} {kind:6s} " + " ".join(f"{r}={mx:.2e}/{mn:.2e}" for r, (mx, mn) in sorted(w.items())))
