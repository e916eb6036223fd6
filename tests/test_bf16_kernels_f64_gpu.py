"""compute_dtype "bf16" launcher by launcher against float64 (MI355X only): the mode the benchmark runs, against tests/bf16_ref.py.

Every output of every case, region by region (the whole tensor, the rows of the last partial row block, each 128-column block, the
last partial 8-column chunk; max-abs and mean-abs scaled by the reference's top magnitude), twice:

  * against the model of the same arithmetic (bf16_ref.Ref(rounding=True): bf16 hand-offs where the kernel has them, float64 between
    them) -- what is left is the fp32 summation order and the rounding flips it causes;
  * against float64 of the same operand values (Ref(rounding=False)) -- the whole cost of the mode.

Every output buffer carries a sentinel row after it and sentinel columns between N and ldc.  Where a launcher offers an fp32 and a
bf16 store of the same value (gemm_tile, gemm_small, gemm_rows, gemm_rowln's x / h copy, ln_rot's y32 / h, add_act), the bf16 store
must equal the round-to-nearest-even bf16 of the fp32 store bit for bit.  One launcher does not meet that: gemm_tile with GELU.  Its
fp32 store evaluates common.h gelu_erf per element (max(x, 0) - |0.5 x r|: two roundings at the end), its bf16 store the packed
gelu_erf2 (fma(-0.5 |x|, r, fma(x, 0.5, 0.5 |x|)): one), so the two fp32 values in front of the stores can be one fp32 ulp apart,
and of 2^16 such elements about one lies on the other side of a bf16 rounding boundary (observed: 4 of 5.2 M).  There the bf16 store
is held to one bf16 ulp per element and to at most 2^-14 of the elements (an fp32 difference of up to four ulps).

A case that is meant to reach one kernel restates the launcher's selection predicate from this chip's CU count
(bf16_ref.small_product, deep_pipeline, rows_mt, resident) and skips, with the numbers, where the predicate chooses another.

Padding is really masked: attention (bf16 streaming and K/V-resident, f32, bf16x3) gives the same bits with zero padding rows and
with finite poison in them -- K rows past Lk that would win every softmax, V rows of 100, Q rows of 50.  The contract stays "rows
past Lk must be finite": a masked weight of zero times an Inf or NaN in V is NaN by construction."""
import pytest
import torch

import bf16_ref as BR
import x3_ref as XR

pytestmark = pytest.mark.gpu

from tcdiff_amd import _lib as L  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402

DEV = "cuda"
BF, DT = torch.bfloat16, L.DT_BF16
BOUNDS = BR.BOUNDS
WORST = {}
SENT = 7.0


def n_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def dev_bf(t):
    return None if t is None else t.to(DEV).to(BF)


def check(name, kind, got, model, f64, regs=None):
    """compare got region by region with the model and with float64; every figure is printed before anything is asserted"""
    f64 = f64.reshape(f64.shape[0], -1)
    got = got.detach().cpu().double().reshape(f64.shape[0], -1)
    regs = regs if regs is not None else BR.regions(f64.shape[0], f64.shape[1])
    bad = []
    for against, ref in (("model", model), ("f64", f64)):
        st = BR.region_stats(got, ref.reshape(f64.shape[0], -1), regs)
        bmax, bmean = BOUNDS[(name, kind, against)]
        w = WORST.setdefault((name, kind, against), {})
        for reg, (mx, mn) in st.items():
            cls = "cols" if reg.startswith("cols") else reg
            pm, pn = w.get(cls, (0.0, 0.0))
            w[cls] = (max(pm, mx), max(pn, mn))
            if not (mx <= bmax and mn <= bmean):
                bad.append((name, kind, against, reg, mx, mn, (bmax, bmean)))
        print(f"{name:13s} {kind:4s} vs {against:5s} " + " ".join(f"{r}={mx:.2e}/{mn:.2e}" for r, (mx, mn) in st.items()))
    assert not bad, bad


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                                              b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


def assert_bf16_is_rne_of_f32(ob, o32, what):
    """the bf16 store of a launch is the round-to-nearest-even bf16 of the fp32 store of the same launch arguments"""
    assert same_bits(ob, o32.to(BF)), f"{what}: the bf16 store is not bf16_rne of the fp32 store " \
        f"({int((ob.float() != o32.to(BF).float()).sum())} elements differ)"


def assert_bf16_within_one_ulp_of_f32(ob, o32, what):
    """gemm_tile with GELU (module docstring): the two stores round fp32 values one fp32 ulp apart"""
    a, b = ob.contiguous().view(torch.int16).int(), o32.to(BF).contiguous().view(torch.int16).int()
    n = int((a != b).sum())
    print(f"{what}: {n} of {a.numel()} bf16 elements are not bf16_rne of the fp32 store")
    assert int((a - b).abs().max()) <= 1, f"{what}: a bf16 store is more than one bf16 ulp from bf16_rne of the fp32 store"
    assert n <= a.numel() * 2.0 ** -14, f"{what}: {n} of {a.numel()} elements differ from bf16_rne of the fp32 store"


def sentinels_intact(o, M, N, what):
    o = o.float().cpu()
    assert bool((o[:M, N:] == SENT).all()) and bool((o[M:] == SENT).all()), f"{what} wrote outside its M x N block"


# ---- gemm_tile: the 128 x 128 kernel, both pipelines --------------------------------------------------------------------------------
_TILE_IDS = [f"{c['M'] if i != 8 else 'long'}x{c['N']}x{c['K']}" for i, c in enumerate(BR.gemm_tile_cases())]


@pytest.mark.parametrize("i", range(len(_TILE_IDS)), ids=_TILE_IDS)
def test_gemm_tile(i):
    c = BR.gemm_tile_cases(n_cu())[i]
    M, N, Kd, lda = c["M"], c["N"], c["K"], c["lda"]
    deep = BR.deep_pipeline(M, N, Kd, n_cu())
    if c["deep"] is not None and deep != c["deep"]:
        pytest.skip(f"{-(-N // 128) * -(-M // 128)} tiles of {Kd // 64} k-tiles on {n_cu()} CUs take the "
                    f"{'four' if deep else 'two'}-stage pipeline, the case is meant for the other")
    d = BR.gemm_inputs(M, N, Kd, a_mod=c["a_mod"], split_n=c["split_n"], lda=lda)
    v = BR.gemm_ref(BR.Ref(False), d, M, act=c["act"], a_mod=c["a_mod"], split_n=c["split_n"])
    A, A2, W, bias = dev_bf(d["A"]), dev_bf(d["A2"]), dev_bf(d["W"]), d["bias"].to(DEV)
    off = d["off"]
    outs = {}
    for store in c["stores"]:
        out = torch.full((M + 1, c["ldc"]), SENT, device=DEV, dtype=torch.float32 if store == "f32" else BF)
        K.gemm_tile(DT, A[:, off:], W, M, N, Kd, lda=lda, A2=None if A2 is None else A2[:, off:], split_n=c["split_n"],
                    a_mod=c["a_mod"], bias=bias, act=c["act"], mode=L.EPI_STORE_F32 if store == "f32" else L.EPI_STORE_T, out=out,
                    ldc=c["ldc"])
        torch.cuda.synchronize()
        sentinels_intact(out, M, N, f"gemm_tile {store}")
        outs[store] = out[:M, :N]
        check("gemm_tile", store, outs[store], BR.Ref(True).rb(v) if store == "bf16" else v, v, BR.regions(M, N))
    if len(outs) == 2 and c["act"] != L.ACT_GELU:
        assert_bf16_is_rne_of_f32(outs["bf16"], outs["f32"], "gemm_tile")
    elif len(outs) == 2:
        assert_bf16_within_one_ulp_of_f32(outs["bf16"], outs["f32"], "gemm_tile GELU")


def test_gemm_tile_qkv_heads():
    """the head-major scatter with a token and a sequence offset: nothing of the images outside the written rows is touched"""
    Lq, nseq, Lp, tok_off, seq_off, H, Kd = 70, 3, 128, 2, 1, 8, 512
    M = nseq * Lq
    d = BR.gemm_inputs(M, 1536, Kd, split_n=1024, seed=7)
    kw = dict(A2=d["A2"], split_n=1024, bias=d["bias"], scale_q=0.125, n_q=512)
    ref, model = BR.Ref(False).qkv_heads(d["A"], d["W"], Lq, nseq, **kw), BR.Ref(True).qkv_heads(d["A"], d["W"], Lq, nseq, **kw)
    imgs = [torch.full((nseq + seq_off + 1, H, Lp, 64), SENT, device=DEV, dtype=BF) for _ in range(3)]
    K.gemm_tile(DT, dev_bf(d["A"]), dev_bf(d["W"]), M, 1536, Kd, A2=dev_bf(d["A2"]), split_n=1024, bias=d["bias"].to(DEV),
                mode=L.EPI_QKV_HEADS, out=imgs[0], out_k=imgs[1], out_v=imgs[2], scale_q=0.125, Lseq=Lq, Lp=Lp, H=H, n_q=512, n_k=512,
                tok_off=tok_off, seq_off=seq_off)
    torch.cuda.synchronize()
    got = []
    for img in imgs:
        img = img.float().cpu()
        keep = torch.ones_like(img, dtype=torch.bool)
        keep[seq_off:seq_off + nseq, :, tok_off:tok_off + Lq] = False
        assert bool((img[keep] == SENT).all()), "the QKV scatter wrote outside its block"
        got.append(img[seq_off:seq_off + nseq, :, tok_off:tok_off + Lq].permute(0, 2, 1, 3).reshape(M, 512))
    rows = lambda xs: torch.cat([x.permute(0, 2, 1, 3).reshape(M, 512) for x in xs], 1)   # noqa: E731
    check("qkv", "bf16", torch.cat(got, 1), rows(model), rows(ref), BR.regions(M, 1536))


# ---- gemm_small_kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,Kd,act,with_bias,a_mod,selected", BR.gemm_small_cases())
def test_gemm_small(M, N, Kd, act, with_bias, a_mod, selected):
    """small_m = True: 32 x 32 tiles, K dealt to eight waves.  The last case (K > 2048) must stay on the 128 x 128 kernel and is held
    to that kernel's bounds"""
    ldc = N + 4
    sel = BR.small_product(M, N, Kd, n_cu(), ldc=ldc)
    if sel != selected:
        pytest.skip(f"on {n_cu()} CUs the launcher's predicate gives small_product = {sel} for {M} x {N} x {Kd}")
    name, rb = ("gemm_small", 32) if selected else ("gemm_tile", 128)
    d = BR.gemm_inputs(M, N, Kd, a_mod=a_mod)
    v = BR.gemm_ref(BR.Ref(False), d, M, act=act, bias=with_bias, a_mod=a_mod)
    outs = {}
    for store in ("f32", "bf16"):
        out = torch.full((M + 1, ldc), SENT, device=DEV, dtype=torch.float32 if store == "f32" else BF)
        K.gemm_tile(DT, dev_bf(d["A"]), dev_bf(d["W"]), M, N, Kd, bias=d["bias"].to(DEV) if with_bias else None, act=act,
                    mode=L.EPI_STORE_F32 if store == "f32" else L.EPI_STORE_T, out=out, ldc=ldc, a_mod=a_mod, small_m=True)
        torch.cuda.synchronize()
        sentinels_intact(out, M, N, f"{name} {store}")
        outs[store] = out[:M, :N]
        check(name, store, outs[store], BR.Ref(True).rb(v) if store == "bf16" else v, v, BR.regions(M, N, row_block=rb))
    assert_bf16_is_rne_of_f32(outs["bf16"], outs["f32"], name)


# ---- gemm_rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Kd,split_n", BR.GEMM_ROWS_NK)
@pytest.mark.parametrize("M", BR.GEMM_ROWS_M)
def test_gemm_rows(M, N, Kd, split_n):
    """every row-block size (mt = 1, 2, 4 and the launcher's own choice), with a bias; then without one and with operands that
    are column slices of wider matrices (lda > K)"""
    d = BR.gemm_inputs(M, N, Kd, split_n=split_n, lda=Kd + 512, seed=4)
    off, ldc = d["off"], N + 8
    ws = K.row_streams(d["W"].to(DEV))
    A, A2 = dev_bf(d["A"]), dev_bf(d["A2"])
    a2 = None if A2 is None else A2[:, off:]
    Ac, A2c = A[:, off:].contiguous(), None if A2 is None else a2.contiguous()
    for with_bias in (True, False):
        v = BR.gemm_ref(BR.Ref(False), d, M, bias=with_bias, split_n=split_n)
        bias = d["bias"].to(DEV) if with_bias else None
        for mt in (1, 2, 4, 0) if with_bias else (0,):
            mt_eff = mt or BR.rows_mt(M, n_cu())
            regs = BR.regions(M, N, row_block=16 * mt_eff)
            outs = {}
            for store in ("f32", "bf16"):
                out = torch.full((M + 1, ldc), SENT, device=DEV, dtype=torch.float32 if store == "f32" else BF)
                kw = dict(mode=L.EPI_STORE_F32 if store == "f32" else L.EPI_STORE_T, bias=bias, out=out, ldc=ldc, mt=mt, split_n=split_n)
                if with_bias:
                    K.gemm_rows(Ac, ws, M, N, Kd, A2=A2c, **kw)
                else:
                    K.gemm_rows(A[:, off:], ws, M, N, Kd, lda=Kd + 512, A2=a2, **kw)
                torch.cuda.synchronize()
                sentinels_intact(out, M, N, f"gemm_rows {store} mt={mt}")
                outs[store] = out[:M, :N]
                check("gemm_rows", store, outs[store], BR.Ref(True).rb(v) if store == "bf16" else v, v, regs)
            assert_bf16_is_rne_of_f32(outs["bf16"], outs["f32"], f"gemm_rows mt={mt}")


def test_gemm_rows_qkv_heads():
    Lq, nseq, Lp, H, Kd = 70, 3, 128, 8, 512
    M = nseq * Lq
    d = BR.gemm_inputs(M, 1536, Kd, split_n=1024, seed=8)
    kw = dict(A2=d["A2"], split_n=1024, bias=d["bias"], scale_q=0.125, n_q=512)
    ref, model = BR.Ref(False).qkv_heads(d["A"], d["W"], Lq, nseq, **kw), BR.Ref(True).qkv_heads(d["A"], d["W"], Lq, nseq, **kw)
    rows = lambda xs: torch.cat([x.permute(0, 2, 1, 3).reshape(M, 512) for x in xs], 1)   # noqa: E731
    ws = K.row_streams(d["W"].to(DEV))
    for mt in (1, 2, 4, 0):
        imgs = [torch.full((nseq + 1, H, Lp, 64), SENT, device=DEV, dtype=BF) for _ in range(3)]
        K.gemm_rows(dev_bf(d["A"]), ws, M, 1536, Kd, A2=dev_bf(d["A2"]), split_n=1024, mode=L.EPI_QKV_HEADS, bias=d["bias"].to(DEV),
                    out=imgs[0], out_k=imgs[1], out_v=imgs[2], scale_q=0.125, Lseq=Lq, Lp=Lp, H=H, n_q=512, n_k=512, mt=mt)
        torch.cuda.synchronize()
        got = []
        for img in imgs:
            img = img.float().cpu()
            assert bool((img[:nseq, :, Lq:] == SENT).all()) and bool((img[nseq] == SENT).all()), "the QKV scatter wrote outside its rows"
            got.append(img[:nseq, :, :Lq].permute(0, 2, 1, 3).reshape(M, 512))
        check("qkv", "bf16", torch.cat(got, 1), rows(model), rows(ref), BR.regions(M, 1536, row_block=16 * (mt or BR.rows_mt(M, n_cu()))))


# ---- gemm_rowln --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BR.ROWLN_NAMES)
def test_gemm_rowln(name):
    """bias -> LN_POST -> FILM -> + residual -> x (fp32); NEXT_LN -> h, rotary -> rot (bf16); a_mod / xres_mod, out_mul / groups;
    low_variance: rows of variance 1e-4 in front of both LayerNorms, where each eps matters"""
    d, kw, M, Kd = BR.rowln_case(name)
    ref, model = BR.Ref(False).rowln(d["A"], d["W"], M, **kw), BR.Ref(True).rowln(d["A"], d["W"], M, **kw)
    G, out_mul = kw.get("groups", 1), kw.get("out_mul", 1)
    R = M * out_mul
    ln, nln, film, xres, rope = kw.get("ln"), kw.get("nln"), kw.get("film"), kw.get("xres"), kw.get("rope")
    flags = L.ROW_BIAS | L.ROW_STORE_X | L.ROW_STORE_H
    flags |= (L.ROW_LN_POST if ln else 0) | (L.ROW_FILM if film is not None else L.ROW_RES if xres is not None else 0)
    flags |= (L.ROW_NEXT_LN if nln else 0) | (L.ROW_STORE_ROT if nln and rope is not None else 0)
    dv = lambda t: None if t is None else t.to(DEV)                # noqa: E731
    xout = torch.full((R + 1, 512), SENT, device=DEV)
    h, r = torch.full((R + 1, 512), SENT, device=DEV, dtype=BF), torch.full((R + 1, 512), SENT, device=DEV, dtype=BF)
    K.gemm_rowln(DT, dev_bf(d["A"]), dev_bf(d["W"]), M, Kd, flags=flags, a_mod=kw.get("a_mod", 0), bias=dv(kw["bias"]),
                 ln_g=dv(ln[0]) if ln else None, ln_b=dv(ln[1]) if ln else None, ln_eps=ln[2] if ln else 1e-6, film=dv(film),
                 film_ld=1024 if film is not None else 0, xres=dv(xres), xres_mod=kw.get("xres_mod", 0), xout=xout, Lseq=kw["Lseq"],
                 nln_g=dv(nln[0]) if nln else None, nln_b=dv(nln[1]) if nln else None, nln_eps=nln[2] if nln else 1e-5, hout=h,
                 rout=r if flags & L.ROW_STORE_ROT else None, rope=dv(rope) if flags & L.ROW_STORE_ROT else None, out_mul=out_mul,
                 out_add=0, groups=G)
    torch.cuda.synchronize()
    for o in (xout, h):
        assert bool((o[R].float() == SENT).all()), "gemm_rowln wrote past its rows"
    mo = ref["mo"]
    assert sorted(mo.tolist()) == list(range(R))
    tail = (torch.arange(M) >= (M // 64) * 64).repeat(G)

    def regs(ncols):
        return [(n, tail if n == "tail" else rw, cs) for n, rw, cs in BR.regions(M, ncols, row_block=64)]
    check("gemm_rowln", "f32", xout.cpu()[mo], model["x"], ref["x"], regs(512))
    if flags & L.ROW_STORE_ROT:
        assert bool((r[R].float() == SENT).all()), "gemm_rowln wrote past its rows"
        cat = lambda u: torch.cat([u["h"], u["rot"]], 1)           # noqa: E731
        check("gemm_rowln", "bf16", torch.cat([h.float().cpu()[mo], r.float().cpu()[mo]], 1), cat(model), cat(ref),
              regs(1024) + [("h", None, slice(0, 512)), ("rot", None, slice(512, 1024))])
    else:
        check("gemm_rowln", "bf16", h.float().cpu()[mo], model["h"], ref["h"], regs(512))
    if not nln:                                                    # h is the bf16 copy of x
        assert_bf16_is_rne_of_f32(h[:R], xout[:R], "gemm_rowln x / h")


# ---- ln_rot ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in BR.LN_ROT])
def test_ln_rot(name):
    c = BR.ln_rot_case(name)
    rows, rope = c["rows"], c["rope"]
    ref, model = (BR.Ref(rd).ln_rot(c["x"], c["g"], c["b"], c["eps"], rope, c["pos"]) for rd in (False, True))
    h, r = torch.full((rows + 1, 512), SENT, device=DEV, dtype=BF), torch.full((rows + 1, 512), SENT, device=DEV, dtype=BF)
    y = torch.full((rows + 1, 512), SENT, device=DEV)
    K.ln_rot(DT, c["x"].to(DEV), rows, c["g"].to(DEV), c["b"].to(DEV), c["eps"], h=h, rot=r if rope is not None else None, y32=y,
             rope=None if rope is None else rope.to(DEV), pos_mod=c["Lq"], pos_base=3)
    torch.cuda.synchronize()
    for o in (h, r, y):
        assert bool((o[rows].float() == SENT).all()), "ln_rot wrote past its rows"
    regs = BR.regions(rows, 512, row_block=rows + 1)
    check("ln_rot", "f32", y[:rows], model["y32"], ref["y32"], regs)
    if rope is not None:
        cat = lambda u: torch.cat([u["h"], u["rot"]], 1)           # noqa: E731
        check("ln_rot", "bf16", torch.cat([h[:rows], r[:rows]], 1).float(), cat(model), cat(ref), BR.regions(rows, 1024, row_block=rows + 1))
    else:
        assert bool((r.float() == SENT).all()), "ln_rot wrote a rotary output it was not given"
        check("ln_rot", "bf16", h[:rows].float(), model["h"], ref["h"], regs)
    assert_bf16_is_rne_of_f32(h[:rows], y[:rows], "ln_rot y32 / h")


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def run_attention(dt, Q, Kp, Vp, nseq, Lq, Lk, n_shared, ng=0):
    """one launch on the padded images (device operands of mode dt); returns O [nseq Lq, 512] with its sentinel row checked"""
    O = torch.full((nseq * Lq + 1, 512), SENT, device=DEV, dtype=K.TORCH_DT[dt])
    K.attention(dt, Q, Kp, Vp, O, nseq, 8, Lq, Lk, Q.shape[2], Kp.shape[2], 512, n_shared=n_shared, ng=ng)
    torch.cuda.synchronize()
    assert bool((O[-1].float() == SENT).all()), "attention wrote past its rows"
    return O[:-1]


_ATT_REFS = {}


def attention_case(case, Lp_q, ng):
    Lq, Lk, nseq, n_shared, gain = case
    assert BR.resident(Lp_q) == (ng is not None)
    Q, Kp, Vp = BR.attn_inputs(*case, Lp_q=Lp_q)
    if (case, Lp_q) not in _ATT_REFS:
        _ATT_REFS[(case, Lp_q)] = tuple(BR.attn_ref(BR.Ref(rd), Q, Kp, Vp, Lq, Lk, n_shared) for rd in (True, False))
    model, ref = _ATT_REFS[(case, Lp_q)]
    O = run_attention(DT, dev_bf(Q), dev_bf(Kp), dev_bf(Vp), nseq, Lq, Lk, n_shared, ng or 0)
    check(BR.attn_name(gain), "bf16", O.float(), model, ref, BR.attn_regions(Lq, nseq))


@pytest.mark.parametrize("case", BR.ATTN_STREAM, ids=lambda c: "-".join(map(str, c)))
def test_attention_streaming(case):
    """attention_kernel<MmaBF16>: Lp_q < 512.  Whole and partial last tiles, a second query block, the rescale across tiles (gain 4:
    one dominant key in the last partial tile)"""
    attention_case(case, BR.round_up(case[0], 128), None)


@pytest.mark.parametrize("ng", [1, 2])
@pytest.mark.parametrize("case", BR.ATTN_RES, ids=lambda c: "-".join(map(str, c)))
def test_attention_resident(case, ng):
    """attention_res_kernel (the benchmarked one), both row groupings forced, the Q image padded to 512 rows also for a small Lq: an
    idle second row group (Lq 1, 32), a second and third query block (257, 513), a last tile of <= 32 and of > 32 keys, whole
    512-key chunks (Lk 512, 1024), a second chunk of 1 key, of 33 keys and full, and with gain 4 a maximum that grows in the first
    tile of the second chunk"""
    attention_case(case, max(512, BR.round_up(case[0], 128)), ng)


@pytest.mark.parametrize("dt", [L.DT_BF16, L.DT_F32, L.DT_BF16X3], ids=["bf16", "f32", "bf16x3"])
@pytest.mark.parametrize("case", BR.ATTN_POISON, ids=lambda c: "-".join(map(str, c)))
def test_attention_masks_its_padding(case, dt):
    """the same output bits with zero padding and with finite poison in every padding row of Q, K and V (bf16: the streaming kernel
    and, where the case is padded to 512 query rows, the resident one in both row groupings)"""
    Lq, Lk, nseq, n_shared, gain = case

    def operand(x):
        if dt == L.DT_BF16:
            return dev_bf(x)
        return torch.from_numpy(XR.encode(x)).to(DEV) if dt == L.DT_BF16X3 else x.to(DEV)
    forms = [(BR.round_up(Lq, 128), 0)]
    if dt == L.DT_BF16:
        forms = forms if BR.resident(forms[0][0]) else forms + [(512, 1), (512, 2)]
    for Lp_q, ng in forms:
        outs = []
        for poison in (False, True):
            Q, Kp, Vp = BR.attn_inputs(*case, Lp_q=Lp_q, poison=poison, rounded=dt == L.DT_BF16)
            assert bool(torch.isfinite(Q).all() and torch.isfinite(Kp).all() and torch.isfinite(Vp).all())
            outs.append(run_attention(dt, operand(Q), operand(Kp), operand(Vp), nseq, Lq, Lk, n_shared, ng))
        assert bool(torch.isfinite(outs[0].float()).all())
        assert same_bits(outs[0], outs[1]), f"Lp_q {Lp_q} ng {ng}: {int((outs[0] != outs[1]).sum())} output elements depend on the padding rows"


# ---- the small launchers -----------------------------------------------------------------------------------------------------------
def _ties(n, seed):
    """float32 values with exact bf16 ties (both parities), values that round up into the next binade, random values, +-0"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0x3C00, 0x4400, (n,), generator=g, dtype=torch.int32) << 16
    kind = torch.arange(n) % 4
    u = torch.where(kind == 0, u | 0x8000, u)
    u = torch.where(kind == 1, (u | 0x7FFF) | 0x007F0000, u)
    f = u.view(torch.float32)
    f = torch.where(kind == 2, torch.randn(n, generator=g) * 10.0 ** torch.randint(-8, 8, (n,), generator=g).float(), f)
    f = f * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    f[::97] = 0.0
    f[1::97] = -0.0
    return f


def bits16(t):
    return torch.from_numpy(XR.bf16_bits(t).astype("int16")).reshape(tuple(t.shape))


def test_convert_pad_is_bf16_rne_and_pads_with_zero():
    """the strided view of engine.encode_music (frame pairs of a [B, 2 S + 1, Cd] tensor): every output is bf16_rne(src) bit for bit"""
    B, S, Cd, ld = 3, 10, 438, 896
    cond = _ties(B * (2 * S + 1) * Cd, 50).reshape(B, 2 * S + 1, Cd)
    src = cond[:, :-1].reshape(B * S, 2 * Cd)
    dst = torch.full((B * S + 1, ld), SENT, device=DEV, dtype=BF)
    K.convert_pad(DT, cond.to(DEV), dst, B * S, 2 * Cd, ld, rows_per_batch=S, batch_stride=(2 * S + 1) * Cd, row_stride=2 * Cd)
    d = dst.cpu()
    assert bool((d[-1].float() == SENT).all()), "convert_pad wrote past its rows"
    assert torch.equal(d[:-1, :2 * Cd].contiguous().view(torch.int16), bits16(src)), "convert_pad is not bf16_rne(src)"
    assert int(d[:-1, 2 * Cd:].contiguous().view(torch.int16).abs().max()) == 0, "padding not zero"


def test_sinusoidal_and_add_act():
    times = torch.tensor([0, 1, 37, 500, 999, 20], dtype=torch.int32)
    f = BR.sin_freq()
    emb = torch.full((7, 512), SENT, device=DEV, dtype=BF)
    K.sinusoidal(DT, times.to(DEV), 6, f.to(DEV), emb)
    assert bool((emb[-1].float() == SENT).all())
    check("sinusoidal", "bf16", emb[:-1].float(), BR.Ref(True).sinusoidal(times, f), BR.Ref(False).sinusoidal(times, f))
    a, bb = BR.rnd(52, 5, 512), BR.rnd(53, 6, 512)
    ia = torch.tensor([4, 0, 0, 2, 1, 3], dtype=torch.int32)
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_GELU, L.ACT_MISH, L.ACT_SILU):
        o, o32 = torch.full((7, 512), SENT, device=DEV, dtype=BF), torch.full((7, 512), SENT, device=DEV)
        K.add_act(DT, a.to(DEV), ia.to(DEV), bb.to(DEV), 6, act, out=o, out32=o32)
        assert bool((o[-1].float() == SENT).all()) and bool((o32[-1] == SENT).all())
        ref, model = BR.Ref(False).add_act(a, ia, bb, act), BR.Ref(True).add_act(a, ia, bb, act)
        check("add_act", "f32", o32[:-1], model["out32"], ref["out32"])
        check("add_act", "bf16", o[:-1].float(), model["out"], ref["out"])
        assert_bf16_is_rne_of_f32(o[:-1], o32[:-1], "add_act")


def test_scatter_time_kv_and_step_prologue():
    """the time-token rows are copies (bit for bit) and nothing else of the caches is touched; step_prologue's FiLM input is
    mish(t_base[t] + hidden) stored as bf16, its x copy bf16_rne(x) with the ld_xin pad zero"""
    NL, n_t, n_kv, H, Lp, S, n_seq, rows, nf, ld = 2, 5, 3, 8, 128, 60, 3, 130, 151, 192
    tab = dev_bf(BR.rnd(60, NL, n_t, 2, 1024))
    t_base, hidden, x = BR.rnd(61, n_t, 512), BR.rnd(62, n_seq, 512), _ties(rows * nf, 63).reshape(rows, nf)
    tseq = torch.tensor([4, 2], dtype=torch.int32)
    tidx = torch.tensor([4, 0, 2], dtype=torch.int32, device=DEV)
    Kc = torch.full((NL, n_kv, H, Lp, 64), SENT, device=DEV, dtype=BF)
    Vc = Kc.clone()
    K.scatter_time_kv(DT, tab, n_t, tidx, Kc, Vc, NL, n_kv, H, Lp, S)
    tb = tab.cpu().reshape(NL, n_t, 2, 2, 8, 64)
    Kh, Vh = Kc.cpu(), Vc.cpu()
    for s in range(n_kv):
        t = int(tidx[s])
        for rr in range(2):
            assert same_bits(Kh[:, s, :, S + rr], tb[:, t, rr, 0]) and same_bits(Vh[:, s, :, S + rr], tb[:, t, rr, 1])
    keep = torch.ones_like(Kh, dtype=torch.bool)
    keep[:, :, :, S:S + 2] = False
    assert bool((Kh[keep].float() == SENT).all()) and bool((Vh[keep].float() == SENT).all())

    counter = torch.zeros(8, dtype=torch.int32, device=DEV)
    film_in = torch.full((n_seq + 1, 512), SENT, device=DEV, dtype=BF)
    xin = torch.full((rows + 1, ld), SENT, device=DEV, dtype=BF)
    tid = torch.zeros(n_seq, dtype=torch.int32, device=DEV)
    Kc.fill_(SENT)
    Vc.fill_(SENT)
    K.step_prologue(DT, counter, tseq.to(DEV), tid, t_base.to(DEV), hidden.to(DEV), film_in, n_seq, tab, n_t, Kc, Vc, None, None,
                    NL, n_kv, H, Lp, 0, S, x.to(DEV), xin, rows, nf, ld)
    torch.cuda.synchronize()
    t = int(tseq[0])
    assert tid.cpu().tolist() == [t] * n_seq
    fi, xi, Kh, Vh = film_in.cpu(), xin.cpu(), Kc.cpu(), Vc.cpu()
    assert bool((fi[-1].float() == SENT).all()) and bool((xi[-1].float() == SENT).all())
    for kv in range(n_kv):
        for rr in range(2):
            assert same_bits(Kh[:, kv, :, S + rr], tb[:, t, rr, 0]) and same_bits(Vh[:, kv, :, S + rr], tb[:, t, rr, 1])
    assert bool((Kh[keep].float() == SENT).all()) and bool((Vh[keep].float() == SENT).all())
    ia = torch.full((n_seq,), t, dtype=torch.int32)
    ref, model = BR.Ref(False).add_act(t_base, ia, hidden, L.ACT_MISH), BR.Ref(True).add_act(t_base, ia, hidden, L.ACT_MISH)
    check("step_prologue", "bf16", fi[:-1].float(), model["out"], ref["out"])
    assert torch.equal(xi[:-1, :nf].contiguous().view(torch.int16), bits16(x)), "step_prologue's x copy is not bf16_rne(x)"
    assert int(xi[:-1, nf:].contiguous().view(torch.int16).abs().max()) == 0, "the ld_xin pad is not zero"


def test_zz_report_worst():
    """the worst error per launcher, output kind, reference and region class over this module's run"""
    for (name, kind, against), w in sorted(WORST.items()):
        print(f"WORST {name:13s} {kind:4s} vs {against:5s} " + " ".join(f"{r}={mx:.2e}/{mn:.2e}" for r, (mx, mn) in sorted(w.items())))
