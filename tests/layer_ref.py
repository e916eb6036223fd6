"""A float64 evaluation of one decoder layer as the chain kernels compute it (model/model.py:97-107,323-344,374-401): the reference
that every launch form of the layer (csrc/chain.hip, csrc/chain_split.hip) is held to by tests/test_layer_f64_gpu.py, pinned to
oracle.tcdiff_oracle.decoder_layer by tests/test_layer_reference_cpu.py.

Inputs are the raw layer weights (unpacked, unfolded), raw FiLM rows (scale | shift per block), LayerNorm vectors, the
cross-attention K / V caches, the rotary table and -- for the self-attention -- this layer's Q / K / V as the bf16 values the
previous launch wrote.  With ``rounding`` the reference rounds to bf16 exactly where the kernel hands a value to an MFMA (GEMM and
attention operands, the weights themselves) and nowhere else; without it, it is the model's arithmetic in float64.

``defect`` emulates a plausible kernel defect (tests/test_layer_reference_cpu.py shows that each one moves the region it touches
by more than the GPU bound for that region).  Not a test module: no test_* name, nothing collected here."""
import numpy as np
import torch
import torch.nn.functional as F

D = torch.float64
H = 8
LOG2E = 1.4426950408889634        # the fragment-order Q carries log2(e) / sqrt(d_k): the in-launch softmax works in the exp2 domain
LN2 = 1.0 / LOG2E


# ---- element maps of the fragment images (csrc/ops.hip kf_index / vf_index; tests/test_chain_layout_cpu.py checks them against
# plain matrix products)
def kf_index(key, d):
    kt, k32, d32 = key >> 5, key & 31, d & 31
    g, jj = (d32 & 15) >> 2, 4 * (d32 >> 4) + (d32 & 3)
    return (((kt * 2 + (k32 >> 4)) * 2 + (d >> 5)) * 64 + g * 16 + (k32 & 15)) * 8 + jj


def vf_index(key, d):
    kt, k32 = key >> 5, key & 31
    g, jj = (k32 & 15) >> 2, 4 * (k32 >> 4) + (k32 & 3)
    return ((kt * 4 + (d >> 4)) * 64 + g * 16 + (d & 15)) * 8 + jj


def unpack_kv(img, fn, nkeys):
    """[n_seq, H, nkt * 2048] fragment image -> [n_seq, H, nkeys, 64]"""
    key, d = np.meshgrid(np.arange(nkeys), np.arange(64), indexing="ij")
    idx = torch.from_numpy(fn(key, d).astype(np.int64)).to(img.device)
    return img[:, :, idx.reshape(-1)].reshape(img.shape[0], img.shape[1], nkeys, 64)


def unpack_q(qf, nseq, Lq, rows):
    """[blocks, 8 waves, 4 (rows / 16 of them used), 2, 64 lanes, 8] -> [n_seq, H, Lq, 64] (the valid rows of every block)"""
    nbs = (Lq + rows - 1) // rows
    q = qf[:, :, :rows // 16].reshape(nseq, nbs, 8, rows // 16, 2, 4, 16, 2, 4)            # seq, block, head, mt, s, g, c, jj >> 2, jj & 3
    # row = rows b + 16 mt + c ; d = 32 s + 16 (jj >> 2) + 4 g + (jj & 3)
    q = q.permute(0, 2, 1, 3, 6, 4, 7, 5, 8).reshape(nseq, 8, nbs * rows, 64)
    return q[:, :, :Lq]


def tokens(img, nseq, Lq):
    """head-major [n_seq, H, >= Lq, 64] -> token rows [n_seq Lq, 512]"""
    return img[:, :, :Lq].permute(0, 2, 1, 3).reshape(nseq * Lq, 512)


def heads(rows, nseq, Lq):
    """token rows [n_seq Lq, 512] -> head-major [n_seq, H, Lq, 64]"""
    return rows.reshape(nseq, Lq, H, 64).permute(0, 2, 1, 3)


# ---- inputs
def rope_table(freqs, n_pos):
    """[n_pos, 512] (cos, sin) of angle pos * freqs[j] for every pair j -- what kernels.rope_table writes"""
    ang = torch.arange(n_pos, dtype=D)[:, None] * freqs.to(D)[None, :]
    return torch.stack((ang.cos(), ang.sin()), -1).reshape(n_pos, 512)


_NAMES = dict(qkv=None, sfc="self_attn.fc.weight", sln_g="self_attn.layer_norm.weight", sln_b="self_attn.layer_norm.bias",
              cq="multihead_attn.w_qs.weight", ck="multihead_attn.w_ks.weight", cv="multihead_attn.w_vs.weight",
              cfc="multihead_attn.fc.weight", cln_g="multihead_attn.layer_norm.weight", cln_b="multihead_attn.layer_norm.bias",
              ff1="linear1.weight", b1="linear1.bias", ff2="linear2.weight", b2="linear2.bias", l3="linear3.weight",
              b3="linear3.bias", **{f"n{i}_{x}": f"norm{i}.{'weight' if x == 'g' else 'bias'}" for i in range(1, 5) for x in "gb"})


def layer_weights(sd, l):
    """the raw weights of decoder layer l of a DanceDecoder state dict, by the names this module uses"""
    p = f"seqTransDecoder.stack.{l}."
    w = {k: sd[p + n] for k, n in _NAMES.items() if n is not None}
    w["qkv"] = torch.cat([sd[p + f"self_attn.w_{x}s.weight"] for x in "qkv"], 0)
    return w


def film_rows(sd, l, t):
    """[n_seq, 3, 1024] raw FiLM rows (scale | shift of film1, film2, film3) of layer l for the time conditioning t [n_seq, 512]"""
    from oracle import tcdiff_oracle as O
    blocks = [torch.cat([u[:, 0] for u in O.film(t, sd, f"seqTransDecoder.stack.{l}.film{i}")], -1) for i in (1, 2, 3)]
    return torch.stack(blocks, 1)


def fold_final(w, Wf, bfin):
    """the last layer's linear3 folded with final_layer as the engine builds it (engine.py _build_chain_streams): W_f W_3 in the first
    nf of 512 output rows, W_f b_3 + b_f; float64"""
    nf = Wf.shape[0]
    Wo = torch.zeros(512, 512, dtype=D)
    Wo[:nf] = Wf.to(D).cpu() @ w["l3"].to(D).cpu()
    bo = torch.zeros(512, dtype=D)
    bo[:nf] = Wf.to(D).cpu() @ w["b3"].to(D).cpu() + bfin.to(D).cpu()
    return Wo, bo


# ---- the layer
class Ref:
    def __init__(self, rounding=True, defect=None):
        self.rounding, self.defect = rounding, defect

    def rb(self, t):
        """a bf16 hand-off (an fp32 value rounded to an MFMA operand); identity without rounding"""
        return t.float().to(torch.bfloat16).to(D) if self.rounding else t

    def c(self, t):
        return t.detach().cpu().to(D)

    def wt(self, t):
        """a GEMM weight as the kernel streams it"""
        return self.rb(self.c(t))

    def is_(self, name):
        d = self.defect
        return d is not None and (d == name or (isinstance(d, tuple) and d[0] == name))

    @staticmethod
    def tail_rows(M, Lq):
        """bool [M]: rows of the last partial 16-row block of their sequence (none when 16 divides Lq)"""
        pos = torch.arange(M) % Lq
        return pos >= (Lq // 16) * 16

    def rotate(self, u, rope, pos):
        cs = self.c(rope)[pos].reshape(-1, 256, 2)
        up = u.reshape(-1, 256, 2)
        return torch.stack((up[..., 0] * cs[..., 0] - up[..., 1] * cs[..., 1], up[..., 1] * cs[..., 0] + up[..., 0] * cs[..., 1]),
                           -1).reshape(-1, 512)

    def positions(self, M, Lq):
        pos = torch.arange(M) % Lq
        if self.is_("rope_tail_shift"):          # the last partial block's rows rotated by their neighbour's angle
            pos = torch.where(self.tail_rows(M, Lq), pos + 1, pos)
        return pos

    @staticmethod
    def ln(v, g, b, eps):
        return F.layer_norm(v, (512,), g.detach().cpu().to(D), b.detach().cpu().to(D), eps)

    def front(self, x, w, rope, Lq):
        """norm1, rotary, w_qs / w_ks / w_vs of layer w on residual rows x [M, 512] -> token rows q (times 1 / sqrt(d_k)), k, v
        (what the previous launch computes for this layer)"""
        x = self.c(x)
        hn = self.ln(x, w["n1_g"], w["n1_b"], 1e-5)
        rn, hb = self.rb(self.rotate(hn, rope, self.positions(x.shape[0], Lq))), self.rb(hn)
        Wq = self.wt(w["qkv"])
        return (rn @ Wq[:512].t()) * 0.125, rn @ Wq[512:1024].t(), hb @ Wq[1024:].t()

    def _attend(self, sc, v, valid, den_mask=None):
        """softmax(sc) v over the keys `valid`; the kernel's P is the UNNORMALISED exp (a bf16 MFMA operand), 1 / l comes last"""
        sc = sc.masked_fill(~valid, float("-inf"))
        pu = torch.exp(sc - sc.amax(-1, keepdim=True))
        den = pu.sum(-1, keepdim=True) if den_mask is None else (pu * den_mask).sum(-1, keepdim=True)
        pv = self.rb(pu) @ v if v.dim() == pu.dim() else (self.rb(pu).unsqueeze(-2) @ v).squeeze(-2)    # (per-row keys: cross-attention)
        return pv / den

    def self_attention(self, q, k, v, Lq, q_scale):
        """q, k, v: head-major [n_seq, H, Lq, 64] (the bf16 values of the images); scores = q k^T q_scale -> O rows [n_seq Lq, 512]"""
        q, k, v = self.c(q), self.c(k), self.c(v)
        nseq = q.shape[0]
        sc = torch.einsum("shqd,shkd->shqk", q, k) * q_scale
        key = torch.arange(Lq)
        valid = torch.ones(Lq, dtype=torch.bool)
        if self.is_("sa_drop_tail_tile"):         # the keys of a partial last 32-key tile skipped
            valid = key < (Lq // 32) * 32
        den_mask = None
        if self.is_("pair_partials"):            # one head pair normalised by three of its four wave partials (key tile t -> wave t % 4)
            p = self.defect[1]
            den_mask = torch.ones(1, H, 1, Lq, dtype=D)
            den_mask[0, 2 * p:2 * p + 2, 0, (key // 32) % 4 == 3] = 0.0
        o = self._attend(sc, v, valid.reshape(1, 1, 1, Lq).expand(nseq, H, Lq, Lq), den_mask)
        return self.rb(tokens(o, nseq, Lq))

    def _k_split(self, a, name):
        if self.is_("ksplit") and self.defect[1] == name:     # one member's 128-column slice of the contraction missing
            m = self.defect[2]
            a = a.clone()
            a[:, 128 * m:128 * m + 128] = 0.0
        return a

    def layer(self, w, xres, film, Kc, Vc, rope, Lq, nseq, *, q=None, k=None, v=None, o=None, q_scale=1.0, Lk=None,
              n_shared=1, shared_rows=0, nxt=None, last=None, fold=None):
        """One decoder layer on M = n_seq Lq rows.

        xres [shared_rows or M, 512]: the residual rows in; film [n_seq, 3, 1024] raw FiLM rows; Kc / Vc [n_kv, H, keys, 64] the
        cross-attention caches (keys >= Lk: padding the kernel masks); rope [>= Lq, 512].  The self-attention either from
        q / k / v (head-major, the first shared_rows / Lq sequences when shared_rows, scores q k^T q_scale) or from attention-output
        rows o.  shared_rows (a_mod / xres_mod of a guided layer 0): row m reads O and xres row m % shared_rows.  n_shared: the
        first n_shared sequences use cache slot 0, sequence s >= n_shared slot s - n_shared + 1.
        nxt: the next layer's weights (its norm1 and w_qs / w_ks / w_vs) -> q, k, v token rows of the next layer; last: "l3" (the
        linear3 rows) or "fold" (the folded final layer, fold = (W_o, b_o) of fold_final) -> out rows.  Returns a dict with x (x')."""
        M = nseq * Lq
        seq = torch.arange(M) // Lq
        tail = self.tail_rows(M, Lq)
        pos = self.positions(M, Lq)
        fm = self.c(film)
        if self.is_("film_tail_neighbour"):       # the last block's rows take the neighbouring sequence's FiLM row
            fm = fm[torch.where(tail, (seq + 1) % nseq, seq)]
        else:
            fm = fm[seq]
        aff = lambda y, blk: (fm[:, blk, :512] + 1) * y + fm[:, blk, 512:]
        ln = self.ln
        rows = torch.arange(M) % shared_rows if shared_rows else torch.arange(M)
        if o is None:
            o = self.self_attention(q, k, v, Lq, q_scale)
        o = self.rb(self.c(o))[rows]
        x = self.c(xres)[rows]
        x = x + aff(ln(self._k_split(o, "sfc") @ self.wt(w["sfc"]).t(), w["sln_g"], w["sln_b"], 1e-6), 0)
        # cross-attention: Q from norm2 + rotary, K / V from the caches
        r2 = self.rb(self.rotate(ln(x, w["n2_g"], w["n2_b"], 1e-5), rope, pos))
        qc = self.rb((r2 @ self.wt(w["cq"]).t()) * 0.125).reshape(M, H, 64)
        Kc, Vc = self.c(Kc), self.c(Vc)
        Lk = Kc.shape[2] if Lk is None else Lk
        nk = Lk + 1 if self.is_("xatt_unmasked") else Lk          # one key past Lk not masked
        kv = torch.where(seq < n_shared, torch.zeros_like(seq), seq - n_shared + 1)
        sc = torch.einsum("mhd,mhkd->mhk", qc, Kc[kv, :, :nk])
        oc = self.rb(self._attend(sc, Vc[kv, :, :nk], torch.ones(1, 1, nk, dtype=torch.bool)).reshape(M, 512))
        x = x + aff(ln(self._k_split(oc, "cfc") @ self.wt(w["cfc"]).t(), w["cln_g"], w["cln_b"], 1e-6), 1)
        # feed-forward
        h3 = self.rb(ln(x, w["n3_g"], w["n3_b"], 1e-5))
        a1 = self.rb(F.gelu(h3 @ self.wt(w["ff1"]).t() + self.c(w["b1"])))
        x = x + aff(self._k_split(a1, "ff2") @ self.wt(w["ff2"]).t() + self.c(w["b2"]), 2)
        h4 = self.rb(ln(x, w["n4_g"], w["n4_b"], 1e-5))
        res = {}
        if last == "fold":
            res["out"] = h4 @ self.rb(fold[0]).t() + fold[1]
            return res
        xn = h4 @ self.wt(w["l3"]).t() + self.c(w["b3"])         # linear3, NO residual (model/model.py:344)
        if last == "l3":
            res["out"] = xn
            return res
        res["x"] = xn
        if nxt is not None:
            res["q"], res["k"], res["v"] = self.front(xn, nxt, rope, Lq)
        return res


def cross_kv(mem, w, freqs):
    """the cross-attention caches of a memory [n_kv, Lk, 512] (model/model.py:331,387-388): K = w_ks(rotary(mem)), V = w_vs(mem),
    head-major [n_kv, H, Lk, 64], float64"""
    mem = mem.to(D)
    n, Lk = mem.shape[:2]
    r = Ref(rounding=False)
    rot = r.rotate(mem.reshape(-1, 512), rope_table(freqs, Lk), torch.arange(n * Lk) % Lk)
    K = rot @ w["ck"].to(D).t()
    V = mem.reshape(-1, 512) @ w["cv"].to(D).t()
    return heads(K, n, Lk), heads(V, n, Lk)


# ---- regions and bounds
def regions(Lq, nseq):
    """(name, row mask or None, column slice): the whole tensor, the rows of every sequence's last partial 16-row block, and every
    128-column quarter (of x': one member's columns; of a Q / K / V image: one head pair)"""
    M = nseq * Lq
    out = [("all", None, slice(0, 512))]
    if Lq % 16:
        out.append(("tail", Ref.tail_rows(M, Lq), slice(0, 512)))
    out += [(f"cols{j}", None, slice(128 * j, 128 * j + 128)) for j in range(4)]
    return out


def region_stats(got, ref, Lq, nseq):
    """{region: (max-abs, mean-abs)} of got - ref over [M, <= 512] rows (a quarter past the last column is left out)"""
    d = (got.to(D).cpu() - ref.to(D).cpu()).abs()
    st = {}
    for name, rows, cols in regions(Lq, nseq):
        part = d[:, cols] if rows is None else d[rows][:, cols]
        if part.numel():
            st[name] = (float(part.max()), float(part.mean()))
    return st


# Bounds of every launch form of the layer against this reference (tests/test_layer_f64_gpu.py), per region, the same for the fused
# and the split forms and for both logit scales: (max-abs, mean-abs).  What is left against float64 are bf16 hand-offs that land on the
# other side of a rounding boundary (one ulp = 2^-8 relative), spread over a row by the next GEMM, plus the images' own bf16 rounding.
# Measured on MI355X, worst over every form, shape and region: x' 2.0e-2 / 3.1e-3, Q / K / V images 2.7e-2 / 3.9e-3, linear3 / folded
# final rows 2.1e-2 / 3.0e-3 -- at qk_gain 4 (nearly one-hot self-attention rows) no more than at 1 (x' 1.9e-2 / 2.7e-3, images
# 2.6e-2 / 3.6e-3).
_B = {"x": (3e-2, 4e-3), "img": (5e-2, 4e-3), "out": (3e-2, 4e-3)}
BOUNDS = {(kind, gain): b for kind, b in _B.items() for gain in (1, 4)}


def exceeded(stats, kind, gain):
    """the regions whose max or mean exceeds the bound of `kind` ("x", "img", "out") at qk_gain `gain`"""
    mx, mn = BOUNDS[(kind, gain)]
    return {k: v for k, v in stats.items() if v[0] > mx or v[1] > mn}


# ---- random layers (bf16-representable weights: what the kernels stream), shared by the CPU and GPU tests
def _rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def random_layer(seed, qk_gain=1.0):
    """raw weights of one decoder layer (the float32 values of bf16 GEMM weights); qk_gain scales w_qs / w_ks (logits far outside
    the range the lazy running maximum absorbs, nearly one-hot rows)"""
    g = torch.Generator().manual_seed(seed)
    bfr = lambda t: t.to(torch.bfloat16).float()
    w = {n: bfr(_rnd(g, *s, scale=s[1] ** -0.5)) for n, s in (("qkv", (1536, 512)), ("sfc", (512, 512)), ("cq", (512, 512)),
                                                           ("cfc", (512, 512)), ("ff1", (1024, 512)), ("ff2", (512, 1024)),
                                                           ("l3", (512, 512)))}
    w["qkv"][:1024] *= qk_gain
    for n in ("n1", "n2", "n3", "n4", "sln", "cln"):
        w[n + "_g"], w[n + "_b"] = 1.0 + 0.1 * _rnd(g, 512), 0.1 * _rnd(g, 512)
    w["b1"], w["b2"], w["b3"] = 0.05 * _rnd(g, 1024), 0.1 * _rnd(g, 512), 0.1 * _rnd(g, 512)
    return w


def random_inputs(seed, Lq, nseq, Lk, n_shared, shared_seqs=None):
    """FiLM rows [n_seq, 3, 1024], residual rows [M, 512], cross-attention caches [n_kv, H, 32 nkt, 64] (bf16 values) whose key slots
    past Lk hold large finite poison (a correct kernel masks them), the final layer (W_f, b_f)"""
    g = torch.Generator().manual_seed(seed)
    nkt = (Lk + 31) // 32
    n_kv = nseq - n_shared + 1
    bfr = lambda t: t.to(torch.bfloat16).float()
    Kc, Vc = bfr(_rnd(g, n_kv, H, 32 * nkt, 64)), bfr(_rnd(g, n_kv, H, 32 * nkt, 64))
    Kc[:, :, Lk:] *= 4.0
    Vc[:, :, Lk:] *= 4.0
    rows = (shared_seqs or nseq) * Lq
    return dict(film=0.3 * _rnd(g, nseq, 3, 1024), xres=_rnd(g, rows, 512), Kc=Kc, Vc=Vc,
                Wf=bfr(_rnd(g, 151, 512, scale=512 ** -0.5)), bf=0.1 * _rnd(g, 151), nkt=nkt, n_kv=n_kv)


def freqs():
    return 1.0 / (10000 ** (torch.arange(0, 512, 2).float() / 512))
