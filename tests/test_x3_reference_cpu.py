"""tests/x3_ref.py -- the float64 split-bf16 reference the parity-mode launchers are held to on the GPU
(tests/test_parity_kernels_f64_gpu.py) -- pinned before any GPU run: its split is the host packer kernels.to_x3 bit for bit, every
restatement without rounding is the operation in float64, and each emulated kernel defect moves the region it touches by at least
ten times that region's GPU bound."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import x3_ref as XR
from oracle import tcdiff_oracle as O
from tcdiff_amd import _lib as L
from tcdiff_amd import kernels as K

D = torch.float64


def _bits(x):
    return torch.as_tensor(x).contiguous().view(torch.int32)


def special_values():
    """random values across exponents, exact ties with even and odd hi, hi rounding up into the next binade, +-0, float32
    subnormals, values near 2^126"""
    g = torch.Generator().manual_seed(0)
    rnd = torch.randn(4096, generator=g) * torch.pow(2.0, torch.randint(-120, 120, (4096,), generator=g).float())
    base = torch.randint(0x0080, 0x7F00, (2048,), generator=g, dtype=torch.int32) << 16
    ties = (base | 0x8000).view(torch.float32)                                   # hi + half an ulp of hi: both parities of hi
    up = (base | 0x7FFF | 0x007F0000).view(torch.float32)                        # all-ones mantissa: hi is the next power of two
    lo_tie = (base | 0x0080).view(torch.float32)                                 # x - hi = 2^-16 ulp-ish: lo itself exact
    sub = torch.randint(1, 0x007FFFFF, (512,), generator=g, dtype=torch.int32).view(torch.float32)
    big = torch.pow(2.0, torch.tensor(126.0)) * (1 + torch.rand(256, generator=g))
    x = torch.cat([rnd, ties, -ties, up, -up, lo_tie, sub, -sub, big, -big, torch.tensor([0.0, -0.0, 1.0, -1.0])])
    return x[: x.numel() // 4 * 4]


def test_host_packer_is_the_reference_split_bit_for_bit():
    x = special_values()
    assert torch.equal(_bits(K.to_x3(x)), _bits(torch.from_numpy(XR.encode(x))))
    hi, lo = XR.split(x)
    # ties to even: hi's last bit is 0 wherever x sat exactly half-way
    u = x.view(torch.int32).numpy()
    tie = (u & 0xFFFF) == 0x8000
    assert tie.sum() > 1000 and not (hi[tie] & 1).any()
    assert (hi[(u & 0x7FFFFF) == 0x7FFFFF] & 0x7F == 0).all()                 # rounded up into the next binade
    # +-0 keep their sign in hi, lo = +0
    z = np.array([0.0, -0.0], dtype=np.float32)
    zh, zl = XR.split(z)
    assert zh.tolist() == [0x0000, 0x8000] and zl.tolist() == [0, 0]


def test_split_round_trip_and_refusals():
    g = torch.Generator().manual_seed(1)
    x = torch.sign(torch.randn(1 << 16, generator=g)) * torch.pow(2.0, torch.empty(1 << 16).uniform_(-100, 125.99, generator=g))
    back = K.from_x3(K.to_x3(x)).to(D)
    assert float(((back - x.to(D)).abs() / x.to(D).abs()).max()) <= 2.0 ** -17
    assert float(((XR.decode(XR.encode(x)) - x.to(D)).abs() / x.to(D).abs()).max()) <= 2.0 ** -17
    assert not XR.non_canonical(XR.encode(special_values())).any()
    with pytest.raises(ValueError):
        K.to_x3(torch.zeros(3, 6))
    with pytest.raises(ValueError):
        XR.encode(np.zeros((3, 6), dtype=np.float32))


def test_non_canonical_flags_swapped_quads_and_oversized_lo():
    x = torch.randn(64, 128) * 3
    e = XR.encode(x).view(np.uint16).reshape(64, 32, 8).copy()
    e[:, 3] = np.concatenate([e[:, 3, 4:], e[:, 3, :4]], -1)                    # hi / lo quads swapped in chunk 3
    bad = XR.non_canonical(e.view(np.float32).reshape(64, 128))
    nz = x.reshape(64, 32, 4)[:, 3] != 0
    assert bad.reshape(64, 32, 4)[:, 3][nz.numpy()].all() and not bad.reshape(64, 32, 4)[:, :3].any()


# ---- restatements without rounding are the operations in float64 -------------------------------------------------------------------
def test_restatements_without_rounding_are_float64():
    r = XR.Ref(rounding=False)
    A, W, b = XR.rnd(1, 130, 192), XR.rnd(2, 256, 192), XR.rnd(3, 256)
    A2 = XR.rnd(4, 50, 192)
    idx = torch.arange(130) % 50
    got = r.gemm(A[:50], W, 130, bias=b, act=L.ACT_GELU, a_mod=50, A2=A2, split_n=128)
    want = torch.cat([A.to(D)[idx] @ W.to(D)[:128].T, A2.to(D)[idx] @ W.to(D)[128:].T], 1) + b.to(D)
    assert float((got - F.gelu(want)).abs().max()) < 1e-12
    # QKV scatter: head h of image j holds columns 512 j + 64 h
    Wq, bq = XR.rnd(5, 1536, 192), XR.rnd(6, 1536)
    q, k, v = r.qkv_heads(A[:120], Wq, 60, 2, A2=A2.repeat(3, 1)[:120], split_n=1024, bias=bq)
    full = torch.cat([A.to(D)[:120] @ Wq.to(D)[:1024].T, A2.repeat(3, 1).to(D)[:120] @ Wq.to(D)[1024:].T], 1) + bq.to(D)
    assert float((q[1, 3, 7] - full[67, 192:256] * 0.125).abs().max()) < 1e-12
    assert float((v[0, 7, 59] - full[59, 1024 + 448:1536]).abs().max()) < 1e-12
    # attention: softmax over the first Lk keys, n_shared sequences on slot 0
    qq, kk, vv = XR.rnd(7, 3, 8, 40, 64, scale=0.3), XR.rnd(8, 2, 8, 70, 64), XR.rnd(9, 2, 8, 70, 64)
    o = r.attention(qq, kk, vv, 61, n_shared=2)
    kv = torch.tensor([0, 0, 1])
    want = torch.softmax(qq.to(D) @ kk.to(D)[kv, :, :61].transpose(-1, -2), -1) @ vv.to(D)[kv, :, :61]
    assert float((o - want.permute(0, 2, 1, 3).reshape(120, 512)).abs().max()) < 1e-12


def test_rowln_and_ln_rot_without_rounding_are_the_oracle():
    """the epilogue chain with the oracle's own LayerNorm, FiLM affine and rotary (float64 state dict of the model)"""
    sd = {k: v.to(D) for k, v in O.synth_state_dict(dn=2, seq_len=60).items() if v.is_floating_point()}
    p = "seqTransDecoder.stack.2."
    M, Lq = 120, 60
    A, xres, t = XR.rnd(1, M, 512), XR.rnd(2, M, 512).to(D), XR.rnd(3, 2, 512).to(D)
    W = sd[p + "self_attn.fc.weight"].to(torch.float32)
    film = torch.cat([u[:, 0] for u in O.film(t, sd, p + "film1")], -1)
    rope = XR.rope_f32(Lq)
    r = XR.Ref(rounding=False)
    got = r.rowln(A, W, M, ln=(sd[p + "self_attn.layer_norm.weight"], sd[p + "self_attn.layer_norm.bias"], 1e-6), film=film,
                  xres=xres, Lseq=Lq, nln=(sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-5), rope=rope, store_h=True)
    v = O.layer_norm(A.to(D) @ W.to(D).T, sd, p + "self_attn.layer_norm", 1e-6)
    x = xres + O.affine(v.reshape(2, Lq, 512), O.film(t, sd, p + "film1")).reshape(M, 512)
    assert float((got["x"] - x).abs().max()) < 1e-12
    u = O.layer_norm(x, sd, p + "norm2", 1e-5)
    assert float((got["h"] - u).abs().max()) < 1e-12
    freqs = sd["rotary.freqs"]
    rot = O.rotary(u.reshape(2, Lq, 512), freqs.to(torch.float32)).reshape(M, 512)
    assert float((got["rot"] - rot).abs().max()) < 1e-6 * float(rot.abs().max())     # the rotary table's float32 angle
    lr = r.ln_rot(x.to(torch.float32), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-5, rope, torch.arange(M) % Lq)
    assert float((lr["y32"] - O.layer_norm(x.to(torch.float32).to(D), sd, p + "norm2", 1e-5)).abs().max()) < 1e-12


def test_small_restatements_without_rounding():
    r = XR.Ref(rounding=False)
    times = torch.tensor([0, 3, 999], dtype=torch.int32)
    emb = r.sinusoidal(times, XR.sin_freq())
    assert float((emb - O.sinusoidal_emb(times, 512).to(D)).abs().max()) < 1e-6               # the oracle takes sin / cos in float32
    a, b = XR.rnd(1, 4, 512), XR.rnd(2, 3, 512)
    ia = torch.tensor([3, 0, 2])
    got = r.add_act(a, ia, b, L.ACT_MISH)["out"]
    assert float((got - O.mish(a.to(D)[ia] + b.to(D))).abs().max()) < 1e-12
    src = XR.rnd(3, 5, 151)
    cp = r.convert_pad(src, 192)
    assert torch.equal(cp[:, :151], src.to(D)) and float(cp[:, 151:].abs().max()) == 0


# ---- the x3 model's own distance from float64: the parity budget ---------------------------------------------------------------------
def _cases():
    """(name, launcher, region rows mask or None, f(ref) -> output) for the defect table and the budget"""
    A, W, b = XR.rnd(11, 129, 512), XR.rnd(12, 256, 512, scale=1 / math.sqrt(512)), XR.rnd(13, 256)
    q, k, v = XR.rnd(14, 2, 8, 150, 64, scale=0.5), XR.rnd(15, 2, 8, 152, 64), XR.rnd(16, 2, 8, 152, 64)
    return {
        "gemm_f32": (lambda r: r.gemm(A, W, 129, bias=b, act=L.ACT_GELU), XR.regions(129, 256)),
        "gemm_t": (lambda r: r.gemm(A, W, 129, bias=b, act=L.ACT_GELU, store=True), XR.regions(129, 256)),
        "attention": (lambda r: r.attention(q, k, v, 150), XR.regions(300, 512, seq_len=150)),
    }


def test_x3_model_distance_from_float64_is_inside_the_budget():
    """Ref(rounding=True) against Ref(rounding=False): what split-bf16 arithmetic costs by itself; the GPU's "x3" bounds sit above it
    (the kernel adds only fp32 summation order) and the ceiling of 1e-4 above both"""
    for name, (f, regs) in _cases().items():
        st = XR.region_stats(f(XR.Ref(True)), f(XR.Ref(False)), regs)
        mx, mn = XR.worst(st)
        print(f"x3 model vs float64 [{name}]: max {mx:.2e} mean {mn:.2e}")
        assert mx < 1e-4 and mx <= XR.BOUNDS[(name, "x3")][0] and mx > XR.BOUNDS[(name, "f32")][0]


# ---- each emulated defect moves its region by at least 10x the GPU bound ---------------------------------------------------------------
DEFECT_TABLE = [
    # defect, launcher case, region, bound kind
    ("act_lo", "gemm_t", "all", "mm3"),
    ("w_lo", "gemm_f32", "all", "mm3"),
    ("cross", "gemm_f32", "all", "mm3"),
    ("quad_swap", "gemm_f32", "all", "mm3"),
    ("tail_no_lo", "gemm_t", "tail", "mm3"),
    ("p_hi", "attention", "all", "mm3"),
    ("cross", "attention", "all", "mm3"),
    # f32_as_x3 is not in this table: relative to the top magnitude, split-bf16 products are only 2-3x further from float64 than
    # exact fp32 ones at these shapes (gemm: 2.5e-6 against 1.2e-6 on an MI355X), so no bound that holds fp32 can be a tenth of
    # that.  It is caught instead by the separation every GPU case asserts: its f32 bound lies below the bf16x3 error it measures
    # (test_f32_as_x3_exceeds_the_f32_bound below checks the same on the reference).
]


@pytest.mark.parametrize("defect,case,region,kind", DEFECT_TABLE)
def test_each_emulated_defect_exceeds_its_region_bound(defect, case, region, kind):
    f, regs = _cases()[case]
    got, ref = f(XR.Ref(True, defect=defect)), f(XR.Ref(True))
    mx = XR.region_stats(got, ref, regs)[region][0]
    bound = XR.BOUNDS[(case, kind)][0]
    print(f"{defect} on {case}/{region}: moves {mx:.2e} = {mx / bound:.1f} x the bound {bound:.1e}")
    assert mx >= 10 * bound, (defect, mx, bound)


def test_f32_as_x3_exceeds_the_f32_bound():
    for name, (f, regs) in _cases().items():
        mx = XR.region_stats(f(XR.Ref(True)), f(XR.Ref(False)), regs)["all"][0]
        print(f"f32_as_x3 on {name}: moves {mx:.2e} = {mx / XR.BOUNDS[(name, 'f32')][0]:.1f} x the f32 bound")
        assert mx > XR.BOUNDS[(name, "f32")][0]


def test_no_defect_is_the_reference():
    for name, (f, regs) in _cases().items():
        assert XR.worst(XR.region_stats(f(XR.Ref(True, defect=None)), f(XR.Ref(True)), regs))[0] == 0.0
    with pytest.raises(ValueError):
        XR.Ref(True, defect="nonsense")
