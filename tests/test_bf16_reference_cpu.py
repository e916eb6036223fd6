"""tests/bf16_ref.py -- the float64 reference the bf16 launchers are held to on the GPU (tests/test_bf16_kernels_f64_gpu.py) -- pinned
before any GPU run: without rounding every restatement is the plain float64 torch expression (attention: softmax(q k^T) v for every
tile and chunk split of the GPU cases), its rounding is torch's own bf16 cast bit for bit, the float32 stand-in of an honest kernel
lies inside every GPU bound at every GPU case, and each emulated kernel defect moves the region it touches by at least ten times
that region's bound (max or mean: after a bf16 store the max is single rounding flips and the mean is the sharp statistic)."""
import pytest
import torch
import torch.nn.functional as F

import bf16_ref as BR
import x3_ref as XR
from tcdiff_amd import _lib as L

D = torch.float64
N_CU = 256           # the MI355X's CU count: the GPU module sizes its long-k-loop case from the chip it runs on


# ---- without rounding: plain float64 ----------------------------------------------------------------------------------------------
def test_gemm_without_rounding_is_float64():
    r = BR.Ref(False)
    d = BR.gemm_inputs(130, 256, 192, a_mod=50, split_n=128, lda=256)
    got = BR.gemm_ref(r, d, 130, act=L.ACT_GELU, a_mod=50, split_n=128)
    idx = torch.arange(130) % 50
    A, A2, W = d["A"][:, 64:].to(D), d["A2"][:, 64:].to(D), d["W"].to(D)
    want = torch.cat([A[idx] @ W[:128].T, A2[idx] @ W[128:].T], 1) + d["bias"].to(D)
    assert float((got - F.gelu(want)).abs().max()) < 1e-12
    # the model differs from it by the bf16 store alone, and an fp32 store not at all
    assert torch.equal(BR.gemm_ref(BR.Ref(True), d, 130, act=L.ACT_GELU, a_mod=50, split_n=128), got)
    assert torch.equal(BR.gemm_ref(BR.Ref(True), d, 130, act=L.ACT_GELU, a_mod=50, split_n=128, store=True), BR.Ref(True).rb(got))
    # QKV scatter: head h of image j holds columns 512 j + 64 h
    dq = BR.gemm_inputs(120, 1536, 192, split_n=1024, seed=5)
    q, k, v = r.qkv_heads(dq["A"], dq["W"], 60, 2, A2=dq["A2"], split_n=1024, bias=dq["bias"])
    full = torch.cat([dq["A"].to(D) @ dq["W"].to(D)[:1024].T, dq["A2"].to(D) @ dq["W"].to(D)[1024:].T], 1) + dq["bias"].to(D)
    assert float((q[1, 3, 7] - full[67, 192:256] * 0.125).abs().max()) < 1e-12
    assert float((v[0, 7, 59] - full[59, 1024 + 448:1536]).abs().max()) < 1e-12


@pytest.mark.parametrize("name", BR.ROWLN_NAMES)
def test_rowln_without_rounding_is_the_parity_reference(name):
    """x3_ref.Ref(rounding=False).rowln is pinned to the oracle's LayerNorm, FiLM affine and rotary by test_x3_reference_cpu.py"""
    d, kw, M, Kd = BR.rowln_case(name)
    got = BR.Ref(False).rowln(d["A"], d["W"], M, **kw)
    want = XR.Ref(False).rowln(d["A"], d["W"], M, **kw)
    for key in ("x", "h", "rot"):
        assert (got[key] is None) == (want[key] is None)
        if got[key] is not None:
            assert float((got[key] - want[key]).abs().max()) < 1e-12 * max(1.0, float(want[key].abs().max()))
    assert torch.equal(got["mo"], want["mo"])


def test_small_launchers_without_rounding_are_float64():
    r = BR.Ref(False)
    c = BR.ln_rot_case("333")
    got = r.ln_rot(c["x"], c["g"], c["b"], c["eps"], c["rope"], c["pos"])
    u = F.layer_norm(c["x"].to(D), (512,), c["g"].to(D), c["b"].to(D), 1e-5)
    assert float((got["y32"] - u).abs().max()) < 1e-12 and torch.equal(got["h"], got["y32"])
    want = XR.Ref(False).ln_rot(c["x"], c["g"], c["b"], c["eps"], c["rope"], c["pos"])
    assert float((got["rot"] - want["rot"]).abs().max()) < 1e-12
    times = torch.tensor([0, 3, 999], dtype=torch.int32)
    ang = (times.float()[:, None] * BR.sin_freq()[None, :]).to(D)
    assert float((r.sinusoidal(times, BR.sin_freq()) - torch.cat((ang.sin(), ang.cos()), -1)).abs().max()) < 1e-15
    a, b = BR.rnd(1, 4, 512), BR.rnd(2, 3, 512)
    ia = torch.tensor([3, 0, 2])
    assert float((r.add_act(a, ia, b, L.ACT_MISH)["out"] - F.mish(a.to(D)[ia] + b.to(D))).abs().max()) < 1e-12
    src = BR.rnd(3, 5, 151)
    cp = r.convert_pad(src, 192)
    assert torch.equal(cp[:, :151], src.to(D)) and float(cp[:, 151:].abs().max()) == 0


def _att_cases():
    return [(c, BR.round_up(c[0], 128)) for c in BR.ATTN_STREAM] + [(c, max(512, BR.round_up(c[0], 128))) for c in BR.ATTN_RES]


@pytest.mark.parametrize("case,Lp_q", _att_cases(), ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_attention_without_rounding_is_softmax(case, Lp_q):
    """the online softmax over 64-key tiles -- every tile and chunk split of the GPU cases -- is softmax(q k^T) v to 1e-12"""
    Lq, Lk, nseq, n_shared, gain = case
    Q, Kp, Vp = BR.attn_inputs(*case, Lp_q=Lp_q)
    got = BR.attn_ref(BR.Ref(False), Q, Kp, Vp, Lq, Lk, n_shared)
    kv = torch.tensor([0 if s < n_shared else s - n_shared + (1 if n_shared > 0 else 0) for s in range(nseq)])
    q, k, v = Q[:, :, :Lq].to(D), Kp.to(D)[kv][:, :, :Lk], Vp.to(D)[kv][:, :, :Lk]
    want = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).permute(0, 2, 1, 3).reshape(nseq * Lq, 512)
    assert float((got - want).abs().max()) < 1e-12
    if gain > 1:                                                   # the dominant key really moves the maximum in a late tile
        s = q @ k.transpose(-1, -2)
        assert bool((s[..., :64].amax(-1) < s.amax(-1) - 8).any())


# ---- rounding ----------------------------------------------------------------------------------------------------------------------
def special_values():
    """as tests/test_x3_reference_cpu.py: random values across exponents, exact ties of both parities, values that carry into the
    next binade, +-0, float32 subnormals, values near 2^126"""
    g = torch.Generator().manual_seed(0)
    rnd = torch.randn(4096, generator=g) * torch.pow(2.0, torch.randint(-120, 120, (4096,), generator=g).float())
    base = torch.randint(0x0080, 0x7F00, (2048,), generator=g, dtype=torch.int32) << 16
    ties = (base | 0x8000).view(torch.float32)
    up = (base | 0x7FFF | 0x007F0000).view(torch.float32)
    sub = torch.randint(1, 0x007FFFFF, (512,), generator=g, dtype=torch.int32).view(torch.float32)
    big = torch.pow(2.0, torch.tensor(126.0)) * (1 + torch.rand(256, generator=g))
    return torch.cat([rnd, ties, -ties, up, -up, sub, -sub, big, -big, torch.tensor([0.0, -0.0, 1.0, -1.0])])


def test_rounding_is_torchs_bf16_cast_bit_for_bit():
    x = special_values()
    want = x.to(torch.bfloat16)
    got = torch.from_numpy(BR.bf16_rne(x))
    assert torch.equal(got.view(torch.int32), want.to(torch.float32).view(torch.int32))
    assert torch.equal(BR.Ref(True).rb(x.to(D)).to(torch.float32).view(torch.int32), want.to(torch.float32).view(torch.int32))
    assert torch.equal(BR.standin().rb(x).view(torch.int32), want.to(torch.float32).view(torch.int32))
    u = x.view(torch.int32)
    tie = (u & 0xFFFF) == 0x8000
    assert int(tie.sum()) > 1000 and not bool(((got.view(torch.int32)[tie] >> 16) & 1).any())          # ties to even
    assert bool(((got.view(torch.int32)[(u & 0x7FFFFF) == 0x7FFFFF] >> 16) & 0x7F == 0).all())          # carried into the next binade
    z = torch.from_numpy(BR.bf16_rne(torch.tensor([0.0, -0.0]))).view(torch.int32).tolist()
    assert z == [0, -2 ** 31]                                                                          # +-0 keep their sign
    # truncation (the p_trunc defect) never rounds up
    t = torch.from_numpy(BR.bf16_trunc(x))
    assert bool((t.abs() <= x.abs()).all()) and bool((t.view(torch.int32) & 0xFFFF == 0).all())
    assert BR.Ref(False).rb(x.to(D)) is not None and torch.equal(BR.Ref(False).rb(x.to(D)), x.to(D))


# ---- every GPU case through a Ref: (launcher, kind, output, regions) ---------------------------------------------------------------
def _gemm_outputs(name, inputs, M, N, rb, stores, **kw):
    def run(r):
        v = BR.gemm_ref(r, inputs(), M, **kw)
        return [(name, s, v if s == "f32" else r.rb(v), BR.regions(M, N, row_block=rb)) for s in stores]
    return run


def _rowln_outputs(name):
    def run(r):
        d, kw, M, Kd = BR.rowln_case(name)
        o = r.rowln(d["A"], d["W"], M, **kw)
        G = kw.get("groups", 1)
        tail = (torch.arange(M) >= (M // 64) * 64).repeat(G)
        regs = lambda n: [(nm, tail if nm == "tail" else rw, cs) for nm, rw, cs in BR.regions(M, n, row_block=64)]     # noqa: E731
        if o["rot"] is not None:
            return [("gemm_rowln", "f32", o["x"], regs(512)),
                    ("gemm_rowln", "bf16", torch.cat([o["h"], o["rot"]], 1), regs(1024) + [("h", None, slice(0, 512)),
                                                                                          ("rot", None, slice(512, 1024))])]
        return [("gemm_rowln", "f32", o["x"], regs(512)), ("gemm_rowln", "bf16", o["h"], regs(512))]
    return run


def _ln_rot_outputs(name):
    def run(r):
        c = BR.ln_rot_case(name)
        o = r.ln_rot(c["x"], c["g"], c["b"], c["eps"], c["rope"], c["pos"])
        rows = c["rows"]
        t = torch.cat([o["h"], o["rot"]], 1) if c["rope"] is not None else o["h"]
        return [("ln_rot", "f32", o["y32"], BR.regions(rows, 512, row_block=rows + 1)),
                ("ln_rot", "bf16", t, BR.regions(rows, t.shape[1], row_block=rows + 1))]
    return run


def _attn_outputs(case, Lp_q, poison=False):
    def run(r):
        Lq, Lk, nseq, n_shared, gain = case
        Q, Kp, Vp = BR.attn_inputs(*case, Lp_q=Lp_q, poison=poison)
        return [(BR.attn_name(gain), "bf16", BR.attn_ref(r, Q, Kp, Vp, Lq, Lk, n_shared), BR.attn_regions(Lq, nseq))]
    return run


def _qkv_outputs(seed, rb):
    def run(r):
        d = BR.gemm_inputs(210, 1536, 512, split_n=1024, seed=seed)
        imgs = r.qkv_heads(d["A"], d["W"], 70, 3, A2=d["A2"], split_n=1024, bias=d["bias"])
        return [("qkv", "bf16", torch.cat([x.permute(0, 2, 1, 3).reshape(210, 512) for x in imgs], 1), BR.regions(210, 1536, row_block=rb))]
    return run


def _small_outputs(r):
    times = torch.tensor([0, 1, 37, 500, 999, 20], dtype=torch.int32)
    out = [("sinusoidal", "bf16", r.sinusoidal(times, BR.sin_freq()), BR.regions(6, 512))]
    a, bb = BR.rnd(52, 5, 512), BR.rnd(53, 6, 512)
    ia = torch.tensor([4, 0, 0, 2, 1, 3], dtype=torch.int32)
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_GELU, L.ACT_MISH, L.ACT_SILU):
        o = r.add_act(a, ia, bb, act)
        out += [("add_act", "f32", o["out32"], BR.regions(6, 512)), ("add_act", "bf16", o["out"], BR.regions(6, 512))]
    t_base, hidden = BR.rnd(61, 5, 512), BR.rnd(62, 3, 512)
    out.append(("step_prologue", "bf16", r.add_act(t_base, torch.full((3,), 4), hidden, L.ACT_MISH)["out"], BR.regions(3, 512)))
    return out


def all_cases():
    cs = {}
    for c in BR.gemm_tile_cases(N_CU):
        d = lambda c=c: BR.gemm_inputs(c["M"], c["N"], c["K"], a_mod=c["a_mod"], split_n=c["split_n"], lda=c["lda"])     # noqa: E731
        cs[f"gemm_tile-{c['M']}x{c['N']}x{c['K']}"] = _gemm_outputs("gemm_tile", d, c["M"], c["N"], 128, c["stores"], act=c["act"],
                                                                    a_mod=c["a_mod"], split_n=c["split_n"])
    for M, N, Kd, act, with_bias, a_mod, selected in BR.gemm_small_cases():
        name, rb = ("gemm_small", 32) if selected else ("gemm_tile", 128)
        cs[f"{name}-{M}x{N}x{Kd}"] = _gemm_outputs(name, lambda M=M, N=N, Kd=Kd, a_mod=a_mod: BR.gemm_inputs(M, N, Kd, a_mod=a_mod), M, N, rb, ("f32", "bf16"), act=act,
                                                   bias=with_bias, a_mod=a_mod)
    for M in BR.GEMM_ROWS_M:
        for N, Kd, split_n in BR.GEMM_ROWS_NK:
            d = lambda M=M, N=N, Kd=Kd, split_n=split_n: BR.gemm_inputs(M, N, Kd, split_n=split_n, lda=Kd + 512, seed=4)     # noqa: E731
            for with_bias in (True, False):
                cs[f"gemm_rows-{M}x{N}x{Kd}-{'bias' if with_bias else 'plain'}"] = _gemm_outputs(
                    "gemm_rows", d, M, N, 16, ("f32", "bf16"), bias=with_bias, split_n=split_n)
    cs["qkv-tile"], cs["qkv-rows"] = _qkv_outputs(7, 128), _qkv_outputs(8, 16)
    for n in BR.ROWLN_NAMES:
        cs["gemm_rowln-" + n] = _rowln_outputs(n)
    for n in [c[0] for c in BR.LN_ROT]:
        cs["ln_rot-" + n] = _ln_rot_outputs(n)
    for case, Lp_q in _att_cases():
        cs["attention-" + "-".join(map(str, case)) + f"-{Lp_q}"] = _attn_outputs(case, Lp_q)
    cs["small"] = _small_outputs
    return cs


CASES = all_cases()
_MEMO = {}


def outputs(cid, rounding, defect=None):
    key = (cid, rounding, defect)
    if key not in _MEMO:
        _MEMO[key] = CASES[cid](BR.Ref(rounding, defect))
    return _MEMO[key]


def test_every_bound_has_a_case_and_every_case_a_bound():
    keys = {(n, k) for cid in CASES for n, k, _, _ in outputs(cid, False)}
    assert {(n, k, a) for n, k in keys for a in ("model", "f64")} == set(BR.BOUNDS)
    for (name, kind, against), (bmax, bmean) in BR.BOUNDS.items():
        assert 0 <= bmean <= bmax
        if kind == "f32" and name.startswith("gemm") and name != "gemm_rowln":
            assert bmax <= 1e-5                                    # an fp32 sum of exact products against float64: the project's figure
        if kind == "f32":
            assert BR.BOUNDS[(name, kind, "model")] <= BR.BOUNDS[(name, kind, "f64")]
        if kind == "bf16" and against == "model":
            assert bmax <= BR.ONE_ULP                              # one rounding flip of the largest element


# ---- the stand-in stays within every bound at every GPU case --------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
def test_standin_is_within_every_bound(cid):
    got = CASES[cid](BR.standin())
    bad = []
    for against, refs in (("model", outputs(cid, True)), ("f64", outputs(cid, False))):
        for (name, kind, g, regs), (_, _, ref, _) in zip(got, refs):
            st = BR.region_stats(g, ref, regs)
            bmax, bmean = BR.BOUNDS[(name, kind, against)]
            print(f"{cid}: {name} {kind} vs {against} " + " ".join(f"{r}={mx:.2e}/{mn:.2e}" for r, (mx, mn) in st.items()))
            bad += [(name, kind, against, reg, mx, mn, (bmax, bmean)) for reg, (mx, mn) in st.items() if mx > bmax or mn > bmean]
    assert not bad, bad


# ---- each emulated defect moves its region by at least 10x the bound -------------------------------------------------------------------
DEFECT_TABLE = [
    # defect, case, launcher, kind, region
    ("acc_bf16", "gemm_tile-2x512x2048", "gemm_tile", "f32", "all"),
    ("acc_bf16", "gemm_tile-2x512x2048", "gemm_tile", "bf16", "all"),
    ("acc_bf16", "gemm_tile-127x1024x64", "gemm_tile", "f32", "tail"),                  # one k-tile: the defect's smallest size
    ("acc_bf16", "gemm_small-150x1024x576", "gemm_small", "bf16", "all"),
    ("acc_bf16", "gemm_rows-917x512x1024-bias", "gemm_rows", "bf16", "tail"),
    ("gelu_tanh", "gemm_tile-1x512x512", "gemm_tile", "f32", "all"),
    ("gelu_tanh", "gemm_tile-%dx2048x512" % BR.long_loop_rows(2048, N_CU), "gemm_tile", "bf16", "all"),
    ("gelu_tanh", "gemm_small-7x64x64", "gemm_small", "f32", "all"),
    ("bias_chunk", "gemm_tile-130x150x192", "gemm_tile", "f32", "chunk"),
    ("bias_chunk", "gemm_tile-130x150x192", "gemm_tile", "bf16", "chunk"),
    ("bias_chunk", "gemm_tile-300x151x512", "gemm_tile", "f32", "chunk"),
    ("p_trunc", "attention-450-450-1-0-1-512", "attention", "bf16", "all"),
    ("p_trunc", "attention-129-97-4-2-1-256", "attention", "bf16", "tail"),
    ("no_rescale_chunk", "attention-64-545-1-0-4-512", "attention_big", "bf16", "all"),
    ("eps_swap", "gemm_rowln-low_variance", "gemm_rowln", "f32", "all"),
    ("eps_swap", "gemm_rowln-low_variance", "gemm_rowln", "bf16", "h"),
    ("eps_swap", "ln_rot-333-low", "ln_rot", "f32", "all"),
    ("eps_swap", "ln_rot-333-low", "ln_rot", "bf16", "all"),
    ("rope_tail_shift", "gemm_rowln-full-512-270", "gemm_rowln", "bf16", "tail"),
    ("rope_tail_shift", "gemm_rowln-groups", "gemm_rowln", "bf16", "rot"),
]


def moved(defect, cid, name, kind, region):
    """(max, mean) by which the defect moves the region, over the model's top magnitude, and the region's bound"""
    got, ref = outputs(cid, True, defect), outputs(cid, True)
    (g, regs), r = [(t, rg) for n, k, t, rg in got if (n, k) == (name, kind)][0], [t for n, k, t, _ in ref if (n, k) == (name, kind)][0]
    return BR.region_stats(g, r, regs)[region], BR.BOUNDS[(name, kind, "model")]


@pytest.mark.parametrize("defect,cid,name,kind,region", DEFECT_TABLE)
def test_each_emulated_defect_exceeds_its_region_bound(defect, cid, name, kind, region):
    (mx, mn), (bmax, bmean) = moved(defect, cid, name, kind, region)
    print(f"{defect} on {cid} {kind}/{region}: moves {mx:.2e} / {mn:.2e} = {mx / bmax:.1f} x / {mn / bmean:.1f} x the bound "
          f"({bmax:.1e}, {bmean:.1e})")
    assert mx >= 10 * bmax or mn >= 10 * bmean, (defect, mx, mn, bmax, bmean)


def test_every_defect_is_in_the_table_and_none_is_the_reference():
    assert {d for d, *_ in DEFECT_TABLE} | {"mask_off_by_one"} == set(BR.DEFECTS)
    for cid in ("gemm_tile-130x150x192", "attention-33-513-1-0-1-512", "gemm_rowln-low_variance", "ln_rot-333-low"):
        for (_, _, a, _), (_, _, b, _) in zip(CASES[cid](BR.Ref(True, defect=None)), outputs(cid, True)):
            assert torch.equal(a, b)
    with pytest.raises(ValueError):
        BR.Ref(True, defect="nonsense")


@pytest.mark.parametrize("case", BR.ATTN_POISON, ids=lambda c: "-".join(map(str, c)))
def test_mask_off_by_one_needs_the_poison(case):
    """With zero padding, one more key in the softmax is one more weight among Lk with a zero value row.  Against float64 that stays
    inside every bound (it is a fraction of what rounding P costs), and against the model it stays under the ten bounds that
    count as caught here -- inside the bound itself at Lk = 513 -- so zero-padded tests cannot be relied on to see it: that is why
    the GPU module poisons the padding.  With the poison it moves every row by orders of magnitude."""
    Lp_q = 512
    bmax, bmean = BR.BOUNDS[("attention", "bf16", "model")]
    fmax, fmean = BR.BOUNDS[("attention", "bf16", "f64")]
    for poison in (False, True):
        (_, _, ref, regs), = _attn_outputs(case, Lp_q, poison)(BR.Ref(True))
        (_, _, f64, _), = _attn_outputs(case, Lp_q, poison)(BR.Ref(False))
        (_, _, got, _), = _attn_outputs(case, Lp_q, poison)(BR.Ref(True, "mask_off_by_one"))
        mx, mn = BR.region_stats(got, ref, regs)["all"]
        print(f"mask_off_by_one on {case}, {'poisoned' if poison else 'zero'} padding: moves {mx:.2e} / {mn:.2e}; bound {bmax:.1e} / {bmean:.1e}")
        if poison:
            assert mx > 10 * bmax and mn > 10 * bmean
        else:
            assert all(a <= fmax and b <= fmean for a, b in BR.region_stats(got, f64, regs).values())
            assert mx <= bmax and mn < 10 * bmean
            if case[1] > 512:
                assert mn <= bmean
    # the reference itself masks: the poison does not move it by a bit
    a, = _attn_outputs(case, Lp_q, False)(BR.Ref(True))
    b, = _attn_outputs(case, Lp_q, True)(BR.Ref(True))
    assert torch.equal(a[2], b[2])


def test_eps_swap_needs_low_variance_rows():
    """at the row variance of the older tests (about 2 in front of the first LayerNorm, 1 in front of ln_rot's) swapping 1e-6 and
    1e-5 stays inside the bounds of the bf16 outputs; on rows of variance 1e-4 it exceeds them more than ten times"""
    for cid, name, region in (("gemm_rowln-full-512-270", "gemm_rowln", "h"), ("ln_rot-333", "ln_rot", "all")):
        (mx, mn), (bmax, bmean) = moved("eps_swap", cid, name, "bf16", region)
        print(f"eps_swap on {cid}: moves {mx:.2e} / {mn:.2e}; bound {bmax:.1e} / {bmean:.1e}")
        assert mx <= bmax and mn <= bmean
    for cid, name, region in (("gemm_rowln-low_variance", "gemm_rowln", "h"), ("ln_rot-333-low", "ln_rot", "all")):
        (mx, mn), (bmax, bmean) = moved("eps_swap", cid, name, "bf16", region)
        print(f"eps_swap on {cid}: moves {mx:.2e} / {mn:.2e}; bound {bmax:.1e} / {bmean:.1e}")
        assert mx > 10 * bmax or mn > 10 * bmean
