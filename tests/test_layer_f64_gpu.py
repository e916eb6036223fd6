"""Every launch form of the decoder layer against the float64 reference of tests/layer_ref.py (pinned to the oracle by
tests/test_layer_reference_cpu.py) -- not against another kernel of this library.  Each case feeds the kernel and the reference the
same bf16 Q / K / V (written by a preceding fused launch, or by part 0 for a guided layer 0) and compares x', the next layer's Q / K / V
images and the rows of a *_LAST form region by region: the rows of every sequence's last partial 16-row block, every 128-column
quarter (one member's columns of x'; one head pair of an image) and the whole tensor.  One bound per shape for every form."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import layer_ref as LR  # noqa: E402
from tcdiff_amd import _lib as L  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402
from tcdiff_amd.engine import DenoiserEngine as E  # noqa: E402

DEV = "cuda"
bf = torch.bfloat16


def n_cu():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def stream(w, nxt=None, l3=None):
    """the fused launch's weight stream (8 waves): fc, w_qs of the cross-attention, its fc, linear1 / linear2, linear3 (or the folded
    final layer), the next layer's w_qs / w_ks / w_vs"""
    g = lambda t: t.to(DEV, bf)
    parts = [E._stages_n512(g(w["sfc"])), E._stages_n512(g(w["cq"])), E._stages_n512(g(w["cfc"]))]
    parts += E._ffn_order(E._stages_ff1(g(w["ff1"])), E._stages_ff2(g(w["ff2"])))
    parts.append(E._stages_n512(g(w["l3"] if l3 is None else l3)))
    if nxt is not None:
        parts += [E._stages_n512(g(nxt["qkv"][i * 512:(i + 1) * 512])) for i in range(3)]
    return torch.cat(parts, 1).contiguous()


def layer_kw(w, inp, nxt, b3=None):
    """the launch arguments of one layer: FiLM rows pre-folded with the LayerNorm weights / linear2 bias around them"""
    d = lambda t: t.to(DEV, torch.float32).contiguous()
    fm = inp["film"].to(DEV)
    ff = torch.cat([K.fold_film(fm[:, 0], d(w["sln_g"]), d(w["sln_b"])), K.fold_film(fm[:, 1], d(w["cln_g"]), d(w["cln_b"])),
                    K.fold_film(fm[:, 2], None, d(w["b2"]))], 1).contiguous()
    return dict(ln_eps=1e-6, film=ff, film_ld=3072, n2_g=d(w["n2_g"]), n2_b=d(w["n2_b"]), filmb=ff[:, 1024:], n3_g=d(w["n3_g"]),
                n3_b=d(w["n3_b"]), b1=d(w["b1"]), film3=ff[:, 2048:], n4_g=d(w["n4_g"]), n4_b=d(w["n4_b"]),
                b3=d(w["b3"] if b3 is None else b3), nn_g=None if nxt is None else d(nxt["n1_g"]),
                nn_b=None if nxt is None else d(nxt["n1_b"]), scale_q=0.125, H=8)


def cross_frags(inp, Lk):
    """the cross-attention caches as fragment images, key slots past Lk included (their poison must stay masked)"""
    nkt, n_kv = inp["nkt"], inp["n_kv"]
    Lpc = K.round_up(Lk, 128)
    Kc = torch.zeros(n_kv, 8, Lpc, 64, device=DEV, dtype=bf)
    Vc = torch.zeros_like(Kc)
    Kc[:, :, :32 * nkt], Vc[:, :, :32 * nkt] = inp["Kc"].to(DEV, bf), inp["Vc"].to(DEV, bf)
    Kf = torch.zeros(n_kv, 8, nkt * 2048, device=DEV, dtype=bf)
    Vf = torch.zeros_like(Kf)
    K.pack_kv_frags(Kc, Vc, Kf, Vf, n_kv, 8, Lpc, nkt, 0, 32 * nkt)
    return Kf, Vf


def frag_bufs(nseq, Lq, rows):
    nbs, skt = (Lq + rows - 1) // rows, (Lq + 31) // 32
    # (poisoned, not zeroed: every slot the consumer reads must have been WRITTEN -- a masked P = 0 times a NaN V is still NaN)
    return (torch.zeros(nseq * nbs, 8, 4, 2, 64, 8, device=DEV, dtype=bf),
            torch.full((nseq, 8, skt * 2048), float("nan"), device=DEV, dtype=bf),
            torch.full((nseq, 8, skt * 2048), float("nan"), device=DEV, dtype=bf), skt)


def unpack(qf, kf, vf, nseq, Lq, rows):
    """fragment images -> head-major float64 Q (times 1 / sqrt(d_k), the log2(e) taken out), K, V"""
    q = LR.unpack_q(qf, nseq, Lq, rows).cpu().double() / LR.LOG2E
    return q, LR.unpack_kv(kf, LR.kf_index, Lq).cpu().double(), LR.unpack_kv(vf, LR.vf_index, Lq).cpu().double()


def launch(form, mode, M, Lq, ws, X, kw):
    """one layer in `form`: ("fused", mt) in place on X[0]; "split" parts 1 -> 2 -> 3 -> 4 / "merged" 12 -> 3 -> 4 from X[0] (X[1], X[2]
    the other buffers).  Returns the buffer that holds x'."""
    A = torch.zeros(M, 512, device=DEV, dtype=bf)                    # (the self-attention comes from the fragments: A is not read)
    if form[0] == "fused":
        K.chain(mode, M, Lq, A, ws, xres=X[0], xout=X[0], mt=form[1], **kw)
        return X[0]
    P = [torch.zeros(M // Lq * ((Lq + 15) // 16), 4, 16, 512, device=DEV) for _ in range(2)]
    if form[0] == "merged":
        K.chain(mode, M, Lq, A, ws, split_part=12, p_out=P[1], xres=X[0], xout=X[1], mt=1, **kw)
    else:
        K.chain(mode, M, Lq, A, ws, split_part=1, p_out=P[0], xres=X[0], xout=X[1], mt=1, **kw)
        K.chain(mode, M, Lq, A, ws, split_part=2, p_in=P[0], p_out=P[1], xres=X[0], xout=X[1], mt=1, **kw)
    flat = dict(kw, xres_mod=0, xres_rowmajor=False)
    K.chain(mode, M, Lq, A, ws, split_part=3, p_in=P[1], p_out=P[0], xres=X[1], xout=X[2], mt=1, **flat)
    K.chain(mode, M, Lq, A, ws, split_part=4, p_in=P[0], xres=X[2], xout=X[1], mt=1, **flat)
    return X[1]


def check(name, got, ref, kind, Lq, nseq, gain, bad):
    st = LR.region_stats(got, ref, Lq, nseq)
    worst = max(st.items(), key=lambda kv: kv[1][1])
    print(f"  {name}: all {st['all'][0]:.2e}/{st['all'][1]:.2e}, worst region {worst[0]} {worst[1][0]:.2e}/{worst[1][1]:.2e}"
          + (f", tail {st['tail'][0]:.2e}/{st['tail'][1]:.2e}" if "tail" in st else ""))
    assert torch.isfinite(got).all(), name
    ex = LR.exceeded(st, kind, gain)
    if ex:
        bad.append((name, ex))


# (Lq, n_seq, Lk, n_shared, qk_gain): 450 = 28 x 16 + 2 (a 2-row last block), 137 / 185: L % 32 in 1..15 / 17..31 (the last key tile's
# first / second half), 120 / 150: the small configurations; 62 / 152 keys: 2 / 5 cross-attention key tiles
SHAPES = [(120, 2, 62, 1, 1), (150, 3, 152, 2, 1), (450, 1, 152, 1, 1), (450, 2, 62, 2, 1), (137, 2, 152, 1, 1), (185, 2, 62, 2, 1),
          (150, 3, 62, 1, 4), (450, 2, 152, 2, 4)]
FORMS = [("fused", 1), ("fused", 2), ("fused", 4), ("split",), ("merged",)]


def _producer(seed, w, inp, Lq, nseq, Kf, Vf, Lk, n_shared, rows, rope_cb):
    """a preceding fused launch (its own random weights, attention-output rows in) that writes this layer's residual rows and its
    Q / K / V fragment images (w_qs / w_ks / w_vs and norm1 of w)"""
    M = nseq * Lq
    wp = LR.random_layer(seed)
    inp_p = LR.random_inputs(seed + 1, Lq, nseq, Lk, n_shared)
    g = torch.Generator().manual_seed(seed + 2)
    Oa = (0.5 * torch.randn(M, 512, generator=g)).to(DEV, bf)
    X = K.to_cb(inp_p["xres"].to(DEV))
    qf, kf, vf, skt = frag_bufs(nseq, Lq, rows)
    K.chain(L.CHAIN_FULL, M, Lq, Oa, stream(wp, w), xres=X, xout=X, mt=rows // 16, seq_blocks=True, qf_out=qf, kf_out=kf, vf_out=vf,
            out_nkt=skt, kf=Kf, vf=Vf, n_shared=n_shared, nkt=inp["nkt"], Lk=Lk, rope=rope_cb, Lp=K.round_up(Lq, 128),
            **layer_kw(wp, inp_p, w))
    return X, qf, kf, vf, skt


def run_case(Lq, nseq, Lk, n_shared, gain, form, last=None):
    M = nseq * Lq
    rows = 16 * form[1] if form[0] == "fused" else 16
    if form[0] != "fused" and 4 * nseq * ((Lq + 15) // 16) > n_cu():
        pytest.skip(f"{4 * nseq * ((Lq + 15) // 16)} workgroups of the small-job form exceed this chip's {n_cu()} CUs")
    w, nxt = LR.random_layer(1000, gain), (None if last else LR.random_layer(2000))
    inp = LR.random_inputs(3000, Lq, nseq, Lk, n_shared)
    rope = torch.empty(Lq, 512, device=DEV)
    K.rope_table(LR.freqs().to(DEV), rope, Lq)
    rope_cb = K.to_cb(rope)
    Kf, Vf = cross_frags(inp, Lk)
    X0, qf, kf, vf, skt = _producer(4000, w, inp, Lq, nseq, Kf, Vf, Lk, n_shared, rows, rope_cb)
    xres = K.from_cb(X0, M).cpu().double()
    q, k, v = unpack(qf, kf, vf, nseq, Lq, rows)
    fold = LR.fold_final(w, inp["Wf"], inp["bf"]) if last == "fold" else None
    ws = stream(w, nxt, l3=None if fold is None else fold[0].float())
    kw = dict(layer_kw(w, inp, nxt, b3=None if fold is None else fold[1].float()), kf=Kf, vf=Vf, n_shared=n_shared, nkt=inp["nkt"],
              Lk=Lk, rope=rope_cb, Lp=K.round_up(Lq, 128), seq_blocks=True, sa_q=qf, sa_kf=kf, sa_vf=vf, sa_nkt=skt)
    if last is None:
        qf2, kf2, vf2, _ = frag_bufs(nseq, Lq, rows)
        kw.update(qf_out=qf2, kf_out=kf2, vf_out=vf2, out_nkt=skt)
    elif last == "l3":
        out = torch.zeros(M, 512, device=DEV, dtype=bf)
        kw.update(h_out=out)
    else:
        out = torch.full((M, 152), float("nan"), device=DEV)
        kw.update(h_out=out, out_ld=152)
    X = [X0, torch.zeros_like(X0), torch.zeros_like(X0)]
    xo = launch(form, L.CHAIN_FULL_LAST if last else L.CHAIN_FULL, M, Lq, ws, X, kw)
    torch.cuda.synchronize()
    ref = LR.Ref().layer(w, xres, inp["film"], inp["Kc"], inp["Vc"], rope, Lq, nseq, q=q, k=k, v=v, Lk=Lk, n_shared=n_shared,
                         nxt=nxt, last=last, fold=fold)
    print(f"{form} {nseq} x {Lq}, Lk {Lk}, n_shared {n_shared}, gain {gain}, last {last}:")
    bad = []
    if last is None:
        check("x'", K.from_cb(xo, M), ref["x"], "x", Lq, nseq, gain, bad)
        for nm, img in zip("qkv", unpack(qf2, kf2, vf2, nseq, Lq, rows)):
            check(nm, LR.tokens(img, nseq, Lq), ref[nm], "img", Lq, nseq, gain, bad)
    elif last == "l3":
        check("out", out.float(), ref["out"], "out", Lq, nseq, gain, bad)
    else:
        check("out", out[:, :151], ref["out"][:, :151], "out", Lq, nseq, gain, bad)
    assert not bad, bad


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("Lq,nseq,Lk,n_shared,gain", SHAPES)
def test_layer_form_against_the_float64_reference(Lq, nseq, Lk, n_shared, gain, form):
    run_case(Lq, nseq, Lk, n_shared, gain, form)


@pytest.mark.parametrize("form", [("fused", 1), ("fused", 4), ("split",), ("merged",)], ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("last", ["l3", "fold"])
@pytest.mark.parametrize("Lq,nseq,Lk,n_shared,gain", [(450, 1, 152, 1, 1), (137, 2, 62, 2, 1)])
def test_last_layer_form_against_the_float64_reference(Lq, nseq, Lk, n_shared, gain, last, form):
    """CHAIN_FULL_LAST: linear3 rows (bf16), or the final layer folded into linear3 (engine.py: W_f W_3, fp32 rows of 152)"""
    run_case(Lq, nseq, Lk, n_shared, gain, form, last)


@pytest.mark.parametrize("form", [("split",), ("merged",)], ids=lambda f: f[0])
@pytest.mark.parametrize("Lq,B", [(150, 1), (120, 2), (450, 1)])
def test_guided_layer_0_with_shared_rows_against_the_float64_reference(Lq, B, form):
    """A guided layer 0 through the fragment front: part 0 writes Q / K / V of the B clips from row-major token rows, then part 1 / 12,
    3, 4 run both branches (2 B sequences) with the self-attention and the residual rows of the first B shared (a_mod / xres_mod,
    row-major xres) and the first B sequences on the null-conditioning cache slot (n_shared = B)."""
    nseq, Lk, gain = 2 * B, 152, 1
    M, Rs = nseq * Lq, B * Lq
    if 4 * nseq * ((Lq + 15) // 16) > n_cu():
        pytest.skip(f"{4 * nseq * ((Lq + 15) // 16)} workgroups of the small-job form exceed this chip's {n_cu()} CUs")
    w, nxt = LR.random_layer(1100), LR.random_layer(2100)
    inp = LR.random_inputs(3100, Lq, nseq, Lk, B, shared_seqs=B)
    rope = torch.empty(Lq, 512, device=DEV)
    K.rope_table(LR.freqs().to(DEV), rope, Lq)
    rope_cb = K.to_cb(rope)
    Kf, Vf = cross_frags(inp, Lk)
    xs = inp["xres"].to(DEV)                                    # [Rs, 512] row-major fp32 token rows (the fusion projection's)
    Wf3 = torch.zeros(512, 1024, device=DEV, dtype=bf)          # (the front stream's first 32 stages: unused by part 0)
    wsf = torch.cat([E._stages_n512(Wf3)] + [E._stages_n512(w["qkv"][i * 512:(i + 1) * 512].to(DEV, bf)) for i in range(3)], 1).contiguous()
    qf, kf, vf, skt = frag_bufs(B, Lq, 16)
    K.chain(L.CHAIN_FRONT, Rs, Lq, None, wsf, split_part=0, xres=xs, nn_g=w["n1_g"].to(DEV), nn_b=w["n1_b"].to(DEV), nn_eps=1e-5,
            rope=rope_cb, qf_out=qf, kf_out=kf, vf_out=vf, out_nkt=skt, scale_q=0.125, H=8)
    q, k, v = unpack(qf, kf, vf, B, Lq, 16)
    qf2, kf2, vf2, _ = frag_bufs(nseq, Lq, 16)
    kw = dict(layer_kw(w, inp, nxt), kf=Kf, vf=Vf, n_shared=B, nkt=inp["nkt"], Lk=Lk, rope=rope_cb, Lp=K.round_up(Lq, 128),
              seq_blocks=True, sa_q=qf, sa_kf=kf, sa_vf=vf, sa_nkt=skt, a_mod=Rs, xres_mod=Rs, xres_rowmajor=True,
              qf_out=qf2, kf_out=kf2, vf_out=vf2, out_nkt=skt)
    X = [xs, torch.zeros(64, M, 8, device=DEV), torch.zeros(64, M, 8, device=DEV)]
    xo = launch(form, L.CHAIN_FULL, M, Lq, stream(w, nxt), X, kw)
    torch.cuda.synchronize()
    ref = LR.Ref().layer(w, inp["xres"], inp["film"], inp["Kc"], inp["Vc"], rope, Lq, nseq, q=q, k=k, v=v, Lk=Lk, n_shared=B,
                         shared_rows=Rs, nxt=nxt)
    # part 0's images themselves: the reference's front on the same rows
    bad = []
    print(f"guided layer 0, {form[0]}, B {B} x {Lq}:")
    for nm, img, r in zip("qkv", (q, k, v), LR.Ref().front(inp["xres"], w, rope, Lq)):
        check("part 0 " + nm, LR.tokens(img, B, Lq), r, "img", Lq, B, gain, bad)
    check("x'", K.from_cb(xo, M), ref["x"], "x", Lq, nseq, gain, bad)
    for nm, img in zip("qkv", unpack(qf2, kf2, vf2, nseq, Lq, 16)):
        check(nm, LR.tokens(img, nseq, Lq), ref[nm], "img", Lq, nseq, gain, bad)
    assert not bad, bad
