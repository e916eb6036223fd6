"""tests/layer_ref.py -- the float64 decoder-layer reference every launch form of the layer is held to on the GPU
(tests/test_layer_f64_gpu.py) -- pinned to the oracle's decoder layer (which tests/test_oracle_golden.py pins to the real model), and
shown to have power: each plausible kernel defect it can emulate moves the region it touches by more than that region's GPU bound."""
import pytest
import torch

import layer_ref as LR
from oracle import tcdiff_oracle as O

D = torch.float64


@pytest.fixture(scope="module")
def sd64():
    return {k: v.to(D) for k, v in O.synth_state_dict(dn=3, seq_len=150).items() if v.is_floating_point()}


def _oracle_case(sd64, l, nseq, Lq, Lk, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(nseq, Lq, 512, generator=g, dtype=D)
    mem = torch.randn(nseq, Lk, 512, generator=g, dtype=D)
    t = torch.randn(nseq, 512, generator=g, dtype=D)
    return x, mem, t


@pytest.mark.parametrize("l,nseq,Lq,Lk", [(3, 2, 150, 62), (0, 1, 137, 152)])
def test_reference_layer_equals_the_oracle_decoder_layer(sd64, l, nseq, Lq, Lk):
    """rounding off: the reference's front (norm1, rotary, w_qs / w_ks / w_vs) and its layer (self-attention from those Q / K / V,
    cross-attention from the caches of the memory, feed-forward, linear3; the next layer's Q / K / V; the folded final layer) are
    the oracle's decoder layer in float64"""
    freqs = sd64["rotary.freqs"]
    x, mem, t = _oracle_case(sd64, l, nseq, Lq, Lk, 11 + l)
    want = O.decoder_layer(x, mem, t, sd64, f"seqTransDecoder.stack.{l}", freqs, 8)
    w, nxt = LR.layer_weights(sd64, l), LR.layer_weights(sd64, l + 1)
    r = LR.Ref(rounding=False)
    rope = LR.rope_table(freqs, Lq)
    rows = x.reshape(-1, 512)
    q, k, v = (LR.heads(u, nseq, Lq) for u in r.front(rows, w, rope, Lq))
    Kc, Vc = LR.cross_kv(mem, w, freqs)
    film = LR.film_rows(sd64, l, t)
    got = r.layer(w, rows, film, Kc, Vc, rope, Lq, nseq, q=q, k=k, v=v, q_scale=1.0, n_shared=1, nxt=nxt)
    dx = float((got["x"] - want.reshape(-1, 512)).abs().max())
    print(f"layer {l}, {nseq} x {Lq}, Lk {Lk}: reference x' vs oracle decoder_layer: max-abs {dx:.1e} (|x'| max {float(want.abs().max()):.2f})")
    assert dx <= 1e-10
    # the next layer's Q / K / V: the oracle's self-attention projections of the next layer on x'
    hn = O.layer_norm(want, sd64, f"seqTransDecoder.stack.{l + 1}.norm1", 1e-5)
    qk = O.rotary(hn, freqs)
    pn = f"seqTransDecoder.stack.{l + 1}.self_attn"
    for nm, ref in (("q", qk @ sd64[pn + ".w_qs.weight"].t() / 8), ("k", qk @ sd64[pn + ".w_ks.weight"].t()),
                    ("v", hn @ sd64[pn + ".w_vs.weight"].t())):
        assert float((got[nm] - ref.reshape(-1, 512)).abs().max()) <= 1e-10, nm
    # the last layer's linear3 folded with final_layer (engine.py) equals final_layer(linear3(...))
    fold = LR.fold_final(w, sd64["final_layer.weight"], sd64["final_layer.bias"])
    out = r.layer(w, rows, film, Kc, Vc, rope, Lq, nseq, q=q, k=k, v=v, last="fold", fold=fold)["out"][:, :151]
    ref = O.linear(want, sd64, "final_layer").reshape(-1, 151)
    assert float((out - ref).abs().max()) <= 1e-10
    out3 = r.layer(w, rows, film, Kc, Vc, rope, Lq, nseq, q=q, k=k, v=v, last="l3")["out"]
    assert torch.equal(out3, got["x"])


@pytest.mark.parametrize("B", [1, 2])
def test_reference_shared_rows_of_a_guided_layer_0_equal_the_oracle(sd64, B):
    """a guided layer 0 (both branches stacked: 2 B sequences; the self-attention and the residual rows of the first B shared, a_mod /
    xres_mod; the first n_shared = B sequences on cache slot 0, the null conditioning) against the oracle on the duplicated rows"""
    l, Lq, Lk = 0, 120, 62
    freqs = sd64["rotary.freqs"]
    x, mem, t = _oracle_case(sd64, l, 2 * B, Lq, Lk, 29 + B)
    x = torch.cat([x[:B], x[:B]])                          # the branches see the same x_t
    kv = torch.tensor([0] * B + list(range(1, B + 1)))     # sequence -> cache slot (n_shared = B)
    slots = mem[:B + 1]
    want = O.decoder_layer(x, slots[kv], t, sd64, f"seqTransDecoder.stack.{l}", freqs, 8).reshape(-1, 512)
    w = LR.layer_weights(sd64, l)
    r = LR.Ref(rounding=False)
    rope = LR.rope_table(freqs, Lq)
    Rs = B * Lq
    q, k, v = (LR.heads(u, B, Lq) for u in r.front(x[:B].reshape(-1, 512), w, rope, Lq))
    Kc, Vc = LR.cross_kv(slots, w, freqs)
    got = r.layer(w, x[:B].reshape(-1, 512), LR.film_rows(sd64, l, t), Kc, Vc, rope, Lq, 2 * B, q=q, k=k, v=v, n_shared=B,
                  shared_rows=Rs)
    assert float((got["x"] - want).abs().max()) <= 1e-10


def _case(Lq, nseq, Lk, n_shared, gain=1.0):
    w, nxt = LR.random_layer(1000, gain), LR.random_layer(2000, gain)
    inp = LR.random_inputs(3000, Lq, nseq, Lk, n_shared)
    rope = LR.rope_table(LR.freqs(), Lq + 1)
    rb = LR.Ref().rb
    q, k, v = (LR.heads(rb(u), nseq, Lq) for u in LR.Ref().front(inp["xres"], w, rope, Lq))    # the bf16 images of the layer before
    return w, nxt, inp, rope, (q, k, v)


def _run(defect, Lq, nseq, Lk, n_shared, gain=1.0):
    w, nxt, inp, rope, (q, k, v) = _case(Lq, nseq, Lk, n_shared, gain)
    return LR.Ref(defect=defect).layer(w, inp["xres"], inp["film"], inp["Kc"], inp["Vc"], rope, Lq, nseq, q=q, k=k, v=v, Lk=Lk,
                                       n_shared=n_shared, nxt=nxt)


# (defect, shape (Lq, n_seq, Lk, n_shared), output, region it must move past the GPU bound)
DEFECTS = [
    ("sa_drop_tail_tile", (137, 2, 152, 1), "x", "all"),
    ("sa_drop_tail_tile", (185, 2, 62, 2), "x", "all"),
    (("ksplit", "sfc", 1), (150, 3, 62, 1), "x", "all"),
    (("ksplit", "cfc", 2), (150, 3, 62, 1), "x", "all"),
    (("ksplit", "ff2", 3), (150, 3, 62, 1), "x", "all"),
    (("pair_partials", 1), (150, 3, 152, 2), "x", "all"),
    ("rope_tail_shift", (450, 2, 152, 1), "q", "tail"),
    ("rope_tail_shift", (450, 2, 152, 1), "k", "tail"),
    ("film_tail_neighbour", (450, 2, 62, 2), "x", "tail"),
    ("xatt_unmasked", (120, 2, 62, 1), "x", "all"),
    ("xatt_unmasked", (450, 1, 152, 1), "x", "all"),
]


@pytest.mark.parametrize("defect,shape,out,region", DEFECTS, ids=[f"{d if isinstance(d, str) else '-'.join(map(str, d))}-{s[0]}x{s[1]}-{o}"
                                                                 for d, s, o, _ in DEFECTS])
def test_each_emulated_defect_exceeds_its_region_bound(defect, shape, out, region):
    Lq, nseq, Lk, n_shared = shape
    good, bad = _run(None, *shape), _run(defect, *shape)
    kind = "x" if out == "x" else "img"
    st = LR.region_stats(bad[out], good[out], Lq, nseq)
    mx, mn = LR.BOUNDS[(kind, 1)]
    print(f"{defect} at {shape}: {out} moves by " + ", ".join(f"{k} {v[0]:.1e}/{v[1]:.1e}" for k, v in st.items())
          + f" (bound {mx:.0e}/{mn:.0e})")
    assert region in LR.exceeded(st, kind, 1), (region, st[region])
    if region == "tail":                 # and only there: a whole-tensor mean would average it away
        assert st["all"][1] < st["tail"][1] / 4


def test_no_defect_is_the_reference():
    """the clean reference is deterministic (the defect runs compare against it)"""
    a, b = _run(None, 137, 2, 62, 1), _run(None, 137, 2, 62, 1)
    assert all(torch.equal(a[k], b[k]) for k in a)
