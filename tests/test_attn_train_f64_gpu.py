"""Train-mode attention, forward and backward, against float64 region by region (MI355X only): tcdiff_attention_train and
tcdiff_attention_bwd (csrc/attention_train.hip, the TRAIN half of csrc/attn_res.h) against tests/attn_train_ref.py.

Every output of every case -- O, O + O_lo, lse; delta, dQ, dK, dV -- region by region (the whole tensor, each (sequence, head) block,
the rows of each sequence's last partial 32-row group and last partial 128-row block; for dK / dV the last partial 32-key group;
max-abs and mean-abs scaled by the reference's top magnitude), twice: against the model of the same arithmetic
(Ref(rounding=True)) and against float64 of the same operand values (Ref(rounding=False)).  Rules of every case:

  * sentinels: O (and O_lo) in a buffer with ldo > 64 H and a row after it, dQ in a 1536-wide buffer at column 0, dK | dV
    interleaved at ld = 1024, a NaN in every pad slot of lse and delta -- all must survive;
  * padding: the pad rows of Q', K, V hold finite poison (K rows that would win every softmax, V rows of 100, Q' rows of 50), delta
    is NaN-filled before the call, dO's pad rows are zero as tcdiff_hip.h requires -- and every output is bit-identical to the run
    with all-zero padding and zeroed workspaces;
  * a backward case takes O, O_lo and lse from the kernel's own forward (held to the reference by the forward cases), so its
    figures are the backward's own error; it runs twice and the bits must be equal;
  * O is bit-identical with and without the second image O_lo.

A case that is meant to reach one kernel restates the launcher's predicate (attn_train_ref.resident_fwd, resident_fwd_ng,
resident_bwd) and skips, with the numbers, where this chip's CU count picks another; on 256 CUs none skips (asserted by the
report).  The mask probes make each of the six regenerated keep bits observable on its own: see attn_train_ref.probe_inputs."""
import math

import pytest
import torch

import attn_train_ref as AR

pytestmark = pytest.mark.gpu

from tcdiff_amd import kernels as K  # noqa: E402

DEV = "cuda"
SENT = 7.0
WORST, SKIPPED, FROB = {}, [], {}
FWD, BWD = AR.fwd_cases(), AR.bwd_cases()
LD_DQ, LD_DKV = 1536, 1024


def n_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def mode(kind):
    dt = K.dtype_id(kind)
    return dt, K.TORCH_DT[dt]


def seed_dev():
    return torch.tensor(AR.SEED, dtype=torch.int32, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def skip(c, why):
    SKIPPED.append((AR.case_id(c), why))
    pytest.skip(why)


def forward(c, imgs, n, Lp_q, Lp_k, *, poison, olo=True, ldo=None):
    """one tcdiff_attention_train launch into sentinel buffers -> (O [n Lq, 64 H], O_lo or None, lse buffer [n, H, Lp_q])"""
    dt, T = mode(c["kind"])
    H, Lq, Lk, ldo = c["H"], c["Lq"], c["Lk"], ldo or c["ldo"]
    Q, Kp, Vp = (t.to(DEV).to(T) for t in imgs[:3])
    M = n * Lq
    O = torch.full((M + 1, ldo), SENT, device=DEV, dtype=T)
    Olo = torch.full((M + 1, ldo), SENT, device=DEV, dtype=T) if olo and c["kind"] == "bf16" else None
    lse = torch.full((n, H, Lp_q), math.nan if poison else 0.0, device=DEV)
    thr, sc = K.drop_params(c["p"])
    K.attention_train(dt, Q, Kp, Vp, O, lse, n, H, Lq, Lk, Lp_q, Lp_k, ldo, seed_dev(), AR.SITE, thr, sc, O_lo=Olo)
    torch.cuda.synchronize()
    for name, buf in (("O", O), ("O_lo", Olo)):
        if buf is not None:
            f = buf.float()
            assert bool((f[:M, 64 * H:] == SENT).all()) and bool((f[M:] == SENT).all()), f"{name} was written outside its block"
    if poison:
        assert bool(lse[:, :, Lq:].isnan().all()), "lse was written in its pad slots"
    assert bool(lse[:, :, :Lq].isfinite().all())
    return O[:M, :64 * H], None if Olo is None else Olo[:M, :64 * H], lse


def backward(c, imgs, fw, n, Lp_q, Lp_k, *, poison, ld_dq=LD_DQ, ld_dkv=LD_DKV):
    """one tcdiff_attention_bwd launch into sentinel buffers, fed by a forward()'s buffers -> delta, dQ, dK, dV"""
    dt, T = mode(c["kind"])
    H, Lq, Lk = c["H"], c["Lq"], c["Lk"]
    Q, Kp, Vp, dO = (t.to(DEV).to(T) for t in imgs)
    O, Olo, lse = fw
    Mq, Mk, ldo = n * Lq, n * Lk, O.stride(0)
    delta = torch.full((n, H, Lp_q), math.nan if poison else 0.0, device=DEV)
    dQ = torch.full((Mq + 1, ld_dq), SENT, device=DEV, dtype=T)
    dKV = torch.full((Mk + 1, ld_dkv), SENT, device=DEV, dtype=T)
    thr, sc = K.drop_params(c["p"])
    K.attention_bwd(dt, Q, Kp, Vp, O, dO, lse, delta, dQ, ld_dq, dKV, dKV.view(-1)[512:], ld_dkv, n, H, Lq, Lk, Lp_q, Lp_k, ldo, 0.125,
                    seed_dev(), AR.SITE, thr, sc, O_lo=Olo)
    torch.cuda.synchronize()
    q, kv = dQ.float(), dKV.float()
    assert bool((q[:Mq, 64 * H:] == SENT).all()) and bool((q[Mq:] == SENT).all()), "dQ was written outside its block"
    assert bool((kv[:Mk, 64 * H:512] == SENT).all()) and bool((kv[:Mk, 512 + 64 * H:] == SENT).all()) and bool((kv[Mk:] == SENT).all()), \
        "dK / dV were written outside their blocks"
    if poison:
        assert bool(delta[:, :, Lq:].isnan().all()), "delta was written in its pad slots"
    return {"delta": delta[:, :, :Lq].reshape(n * H, Lq), "dQ": dQ[:Mq, :64 * H], "dK": dKV[:Mk, :64 * H], "dV": dKV[:Mk, 512:512 + 64 * H]}


def check(rows, c, frob):
    """every figure is printed before anything is asserted"""
    AR.report(rows, WORST)
    lim_o, lim_g = AR.FROBENIUS[c["kind"]]
    for out, f in frob.items():
        FROB[(out, c["kind"])] = max(FROB.get((out, c["kind"]), 0.0), f)
        print(f"{out} {c['kind']}: whole-tensor Frobenius ratio against float64 {f:.2e}")
    bad = AR.outside(rows)
    assert not bad, bad
    if c["gain"] == 1:        # (the existing test's bounds are for its unit-gain data)
        assert all(f < (lim_o if out == "O" else lim_g) for out, f in frob.items()), frob


def dev_inputs(c, n, Lp_q, Lp_k, poison):
    return AR.inputs(c, Lp_q, Lp_k, poison=poison, n_cu=n_cu())


@pytest.mark.parametrize("i", range(len(FWD)), ids=[AR.case_id(c) for c in FWD])
def test_forward(i):
    c = FWD[i]
    n, kind, Lq, Lk, H = AR.n_seq(c, n_cu()), c["kind"], c["Lq"], c["Lk"], c["H"]
    Lp_q, Lp_k = AR.pads(c)
    fam = "stream" if not AR.resident_fwd(kind, Lp_q, c["ldo"]) else "res%d" % AR.resident_fwd_ng(Lq, H, n, n_cu())
    if fam != c["want"]:
        skip(c, f"{-(-Lq // 256)} x {H} x {n} workgroups on {n_cu()} CUs take {fam}, the case is meant for {c['want']}")
    imgs = dev_inputs(c, n, Lp_q, Lp_k, True)
    O, Olo, lse = forward(c, imgs, n, Lp_q, Lp_k, poison=True)
    Oz, Oloz, lsez = forward(c, dev_inputs(c, n, Lp_q, Lp_k, False), n, Lp_q, Lp_k, poison=False)
    assert same_bits(O, Oz) and same_bits(lse[:, :, :Lq], lsez[:, :, :Lq]), "finite poison in the padding rows changed O or lse"
    got = {"O": O, "lse": lse[:, :, :Lq].reshape(n * H, Lq)}
    if kind == "bf16":
        assert same_bits(Olo, Oloz), "finite poison in the padding rows changed O_lo"
        O1, _, lse1 = forward(c, imgs, n, Lp_q, Lp_k, poison=True, olo=False)
        assert same_bits(O, O1) and same_bits(lse[:, :, :Lq], lse1[:, :, :Lq]), "O or lse differs with and without O_lo"
        got["O+O_lo"] = O.double() + Olo.double()
    keep = AR.keep_of(c, Lp_k, n_cu())
    Q, Kp, Vp = imgs[:3]
    refs = {a: AR.fwd_outputs(r.fwd(Q[:, :, :Lq], Kp, Vp, keep, Lk), kind) for a, r in (("model", AR.model_of(kind)), ("f64", AR.Ref(False)))}
    check(AR.measure(got, refs, c, n), c, {"O": AR.frobenius(O, refs["f64"]["O"])})
    if (Lq, Lk) == (1, 1) and c["p"] == 0:
        # one key: P = 1 and O = V exactly (bf16: V is a bf16 value already); lse = s log2e to the fp32 evaluation of s (in f32 a sum
        # of 64 rounded products, each step within 2^-24 of the magnitudes summed so far: 65 2^-24 sum |q_d k_d|; exact in bf16) and
        # to the roundings of m = s log2e, of exp2, of log2 and of the sum (2^-22 of max(|lse|, 1))
        assert torch.equal(O.double().cpu(), AR.tok(Vp[:, :, :1].double()))
        qk = Q[:, :, :1].double() * Kp[:, :, :1].double()
        s = qk.sum(-1).reshape(n * H, 1) * AR.LOG2E
        tol = (65 * 2.0 ** -24 * AR.LOG2E * qk.abs().sum(-1).reshape(n * H, 1) if kind == "f32" else 0.0) + 2.0 ** -22 * s.abs().clamp_min(1.0)
        err = (got["lse"].double().cpu() - s).abs()
        print(f"1 x 1 {kind}: |lse - s log2e| / tolerance {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all())


@pytest.mark.parametrize("i", range(len(BWD)), ids=[AR.case_id(c) for c in BWD])
def test_backward(i):
    c = BWD[i]
    n, kind, Lq, Lk, H = AR.n_seq(c, n_cu()), c["kind"], c["Lq"], c["Lk"], c["H"]
    Lp_q, Lp_k = AR.pads(c, True)
    fam = "res" if AR.resident_bwd(kind, Lq, Lk, LD_DQ, LD_DKV) else "stream"
    assert fam == c["want"]                                    # (the backward's predicate does not depend on the CU count)
    imgs = dev_inputs(c, n, Lp_q, Lp_k, True)
    fw = forward(c, imgs, n, Lp_q, Lp_k, poison=True, olo=c["olo"])
    got = backward(c, imgs, fw, n, Lp_q, Lp_k, poison=True)
    again = backward(c, imgs, fw, n, Lp_q, Lp_k, poison=True)
    assert all(same_bits(got[k], again[k]) for k in got), "the backward is not bitwise repeatable"
    imgz = dev_inputs(c, n, Lp_q, Lp_k, False)
    gz = backward(c, imgz, forward(c, imgz, n, Lp_q, Lp_k, poison=False, olo=c["olo"]), n, Lp_q, Lp_k, poison=False)
    assert all(same_bits(got[k], gz[k]) for k in got), \
        "poison in the padding rows or NaN in the delta workspace changed " + str([k for k in got if not same_bits(got[k], gz[k])])
    keep = AR.keep_of(c, Lp_k, n_cu())
    Q, Kp, Vp, dO = imgs
    Oh, lo = AR.heads(fw[0].double().cpu(), n, H), None if fw[1] is None else AR.heads(fw[1].double().cpu(), n, H)
    refs = {a: AR.bwd_outputs(r.bwd(Q[:, :, :Lq], Kp, Vp, dO[:, :, :Lq], Oh, lo, fw[2][:, :, :Lq].cpu(), keep, Lk))
            for a, r in (("model", AR.model_of(kind)), ("f64", AR.Ref(False)))}
    tops = AR.zero_gradient_tops(c, Q, Kp, Vp, dO)
    check(AR.measure(got, refs, c, n, tops), c, {k: AR.frobenius(got[k], refs["f64"][k]) for k in ("dQ", "dK", "dV") if k not in tops})


# ---- mask probes: every regenerated keep bit on its own -----------------------------------------------------------------------------
FAMILIES = {
    # family: kind, ldo of the forward probe, (ld_dq, ld_dkv) of the backward probes
    "res": ("bf16", 520, (1536, 1024)),
    "stream-bf16": ("bf16", 516, (1540, 1028)),       # ldo % 8 != 0 and ld_dq % 8 != 0: the streaming kernels at a resident size
    "stream-f32": ("f32", 520, (1536, 1024)),
}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("Lq,Lk", AR.PROBE_SHAPES)
@pytest.mark.parametrize("which", ["fwd", "dkv", "dq"])
def test_mask_probe(which, Lq, Lk, family):
    kind, ldo_f, (ld_dq, ld_dkv) = FAMILIES[family]
    n, H = 2, 8
    c = AR.case(Lq, Lk, kind, n=n, H=H, p=AR.PROBE_P[which], ldo=ldo_f if which == "fwd" else 520)
    Lp_q, Lp_k = AR.pads(c, True)
    res = family == "res"
    assert AR.resident_fwd(kind, Lp_q, c["ldo"]) == (kind == "bf16" and (res or which != "fwd"))
    assert AR.resident_bwd(kind, Lq, Lk, ld_dq, ld_dkv) == res
    keep = AR.keep_of(c, Lp_k)
    model = AR.model_of(kind)
    worst, n_over, where = 0.0, 0, []
    for blk in AR.probe_blocks(which, Lk):
        imgs = AR.probe_inputs(which, Lq, Lk, kind, Lp_q, Lp_k, n, H, block=blk)
        Q, Kp, Vp, dO = imgs
        fw = forward(c, imgs, n, Lp_q, Lp_k, poison=True)
        if which == "fwd":
            got, ref = fw[0], AR.tok(model.fwd(Q[:, :, :Lq], Kp, Vp, keep, Lk)["O"])
        else:
            out = "dV" if which == "dkv" else "dQ"
            got = backward(c, imgs, fw, n, Lp_q, Lp_k, poison=True, ld_dq=ld_dq, ld_dkv=ld_dkv)[out]
            Oh, lo = AR.heads(fw[0].double().cpu(), n, H), None if fw[1] is None else AR.heads(fw[1].double().cpu(), n, H)
            ref = AR.tok(model.bwd(Q[:, :, :Lq], Kp, Vp, dO[:, :, :Lq], Oh, lo, fw[2][:, :, :Lq].cpu(), keep, Lk)[out])
        d = (got.double().cpu() - ref).abs()
        tol = 2 * AR.bf16_ulp(ref) if kind == "bf16" else 1e-5 * ref.abs()
        over = d > tol
        worst, n_over = max(worst, float((d / tol.clamp_min(1e-300)).max())), n_over + int(over.sum())
        where += [(blk, *x) for x in over.nonzero()[:4].tolist()]
        print(f"{which} probe {Lq} x {Lk} {family} block {blk}: worst |kernel - model| / tolerance {float((d / tol.clamp_min(1e-300)).max()):.3f}, "
              f"{int(over.sum())} of {d.numel()} elements over it, magnitudes {float(ref.abs().min()):.3e} .. {float(ref.abs().max()):.3e}")
    assert n_over == 0, (n_over, worst, where[:8])


def test_zz_report_worst():
    """the worst figure per (output, dtype, against, region class) of this run, beside its bound"""
    for key in sorted(WORST):
        print(f"{key[0]:10s} {key[1]:4s} vs {key[2]:5s} bound {AR.BOUNDS[key][0]:.1e}/{AR.BOUNDS[key][1]:.1e}  " +
              " ".join(f"{r}={a:.2e}/{b:.2e}" for r, (a, b) in sorted(WORST[key].items())))
    for key in sorted(FROB):
        print(f"{key[0]:10s} {key[1]:4s} worst whole-tensor Frobenius ratio against float64 {FROB[key]:.2e}")
    print("skipped:", SKIPPED)
    if n_cu() == 256:
        assert not SKIPPED, SKIPPED
