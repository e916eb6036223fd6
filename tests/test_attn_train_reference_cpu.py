"""tests/attn_train_ref.py -- the float64 reference that train-mode attention is held to on the GPU (tests/test_attn_train_f64_gpu.py)
-- pinned before any GPU run: without rounding it is torch autograd in float64 through torch.softmax, a mask multiply and two
matmuls; its forward with p = 0 is bf16_ref's attention model bit for bit; the float32 stand-in of an honest kernel lies inside
every GPU bound at every GPU case; each emulated kernel defect moves the region it touches by at least ten times that region's
bound (max or mean: after a bf16 store the max is single rounding flips and the mean is the sharp statistic); and in the mask
probes' inputs every single keep bit moves its output element by at least four bf16 ulps."""
import math

import pytest
import torch

import attn_train_ref as AR
import bf16_ref as BR

D = torch.float64
N_CU = 256
FWD, BWD = AR.fwd_cases(), AR.bwd_cases()


# ---- without rounding: torch autograd in float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,Lk,p", [(1, 1, 0.0), (33, 31, 0.1), (129, 65, 0.5), (70, 577, 0.1)])
def test_without_rounding_is_torch_autograd(Lq, Lk, p):
    c = AR.case(Lq, Lk, "f32", H=3, p=p)
    Lp_q, Lp_k = AR.pads(c, True)
    Q, Kp, Vp, dO = AR.inputs(c, Lp_q, Lp_k, poison=True)
    keep = AR.keep_of(c, Lp_k)
    r = AR.Ref(False)
    f = r.fwd(Q[:, :, :Lq], Kp, Vp, keep, Lk)
    b = r.bwd(Q[:, :, :Lq], Kp, Vp, dO[:, :, :Lq], f["O"], None, f["lse"], keep, Lk, scale_q=0.125)
    qr = (Q[:, :, :Lq].to(D) * 8).requires_grad_(True)               # the unscaled projection output
    kr, vr = Kp[:, :, :Lk].to(D).requires_grad_(True), Vp[:, :, :Lk].to(D).requires_grad_(True)
    s = (qr * 0.125) @ kr.transpose(2, 3)
    att = torch.softmax(s, -1)
    if p > 0:
        att = att * keep.mask() * keep.scale
    o = att @ vr
    o.backward(dO[:, :, :Lq].to(D))
    # (1e-12 of the reference's top magnitude; at 1 x 1 the gradients of Q' and K are exactly zero -- P = 1, dS = dP - delta = 0 --
    # and the operands' unit scale takes its place)
    near = lambda a, w: float((a - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), 1.0 if Lk == 1 else 0.0)     # noqa: E731
    assert near(f["O"], o.detach()) and torch.equal(f["O"], f["o"]) and float(f["O_lo"].abs().max()) == 0.0
    assert near(f["lse"], torch.logsumexp(s.detach(), -1) / math.log(2.0))
    assert near(b["delta"], (dO[:, :, :Lq].to(D) * o.detach()).sum(-1))
    assert near(b["dQ"], qr.grad) and near(b["dK"], kr.grad) and near(b["dV"], vr.grad)


@pytest.mark.parametrize("Lq,Lk,gain", [(33, 31, 1), (129, 65, 1), (450, 450, 1), (64, 545, 4), (70, 513, 1)])
def test_forward_model_without_dropout_is_the_inference_model(Lq, Lk, gain):
    c = AR.case(Lq, Lk, gain=gain)
    Lp_q, Lp_k = AR.pads(c)
    Q, Kp, Vp, _ = AR.inputs(c, Lp_q, Lp_k, poison=True)
    for defect in (None, "p_trunc", "no_rescale_chunk", "mask_off_by_one"):
        got = AR.Ref(True, defect).fwd(Q[:, :, :Lq], Kp, Vp, AR.keep_of(c, Lp_k), Lk)
        assert torch.equal(AR.tok(got["O"]), BR.Ref(True, defect).attention(Q[:, :, :Lq], Kp, Vp, Lk))
        assert torch.equal(AR.tok(got["o"]), BR.Ref(True, defect).attention(Q[:, :, :Lq], Kp, Vp, Lk, store=False))
    # O + O_lo carries 16 bits of o
    got = AR.Ref(True).fwd(Q[:, :, :Lq], Kp, Vp, AR.keep_of(c, Lp_k), Lk)
    assert float(((got["O+O_lo"] - got["o"]).abs() / got["o"].abs().clamp_min(1e-30)).max()) <= 2.0 ** -16


def test_predicates_and_cases():
    """every kernel and branch of the launchers has a case meant for it on 256 CUs"""
    fam = lambda c: ("stream" if not AR.resident_fwd(c["kind"], AR.pads(c)[0], c["ldo"]) else       # noqa: E731
                     "res%d" % AR.resident_fwd_ng(c["Lq"], c["H"], AR.n_seq(c, N_CU), N_CU))
    assert all(fam(c) == c["want"] for c in FWD)
    assert all(("res" if AR.resident_bwd(c["kind"], c["Lq"], c["Lk"]) else "stream") == c["want"] for c in BWD)
    res = [c for c in FWD if c["want"].startswith("res")]
    assert {AR.last_tile_ns(c["Lk"]) for c in res} == {1, 2}
    assert any(c["Lk"] == 513 for c in res) and any(c["Lk"] > 512 and AR.last_tile_ns(c["Lk"]) == 2 for c in res)
    assert any(c["want"] == "res2" for c in res) and AR.resident_fwd_ng(385, 8, 16, N_CU) == 1
    assert any(c["ldo"] % 8 and AR.pads(c)[0] >= 512 and c["want"] == "stream" for c in FWD)
    assert len({AR.case_id(c) for c in FWD}) == len(FWD) and len({AR.case_id(c) for c in BWD}) == len(BWD)


# ---- every GPU case through a Ref ----------------------------------------------------------------------------------------------------
_MEMO = {}


def run_case(c, backward, who, defect=None):
    """the compared outputs of a case: who = "standin" / "model" / "f64".  A backward case takes O, O_lo and lse from the stand-in's
    forward (on the GPU: from the kernel's own), whoever evaluates the backward."""
    key = (AR.case_id(c), backward, who, defect)
    if key in _MEMO:
        return _MEMO[key]
    Lq, Lk, kind = c["Lq"], c["Lk"], c["kind"]
    Lp_q, Lp_k = AR.pads(c, backward)
    Q, Kp, Vp, dO = AR.inputs(c, Lp_q, Lp_k, poison=True, n_cu=N_CU)
    keep = AR.keep_of(c, Lp_k, N_CU)
    mk = lambda d=None: {"standin": AR.Ref(kind == "bf16", d, dtype=torch.float32), "model": AR.model_of(kind, d),     # noqa: E731
                         "f64": AR.Ref(False, d)}[who]
    if not backward:
        out = AR.fwd_outputs(mk(defect).fwd(Q[:, :, :Lq], Kp, Vp, keep, Lk), kind)
    else:
        f = AR.Ref(kind == "bf16", dtype=torch.float32).fwd(Q[:, :, :Lq], Kp, Vp, keep, Lk)
        lo = f["O_lo"] if c["olo"] and kind == "bf16" else None
        out = AR.bwd_outputs(mk(defect).bwd(Q[:, :, :Lq], Kp, Vp, dO[:, :, :Lq], f["O"], lo, f["lse"], keep, Lk))
    if defect is None:
        _MEMO[key] = out
    return out


def tops_of(c, backward):
    Lp_q, Lp_k = AR.pads(c, backward)
    return AR.zero_gradient_tops(c, *AR.inputs(c, Lp_q, Lp_k, poison=True, n_cu=N_CU)) if backward else {}


def test_every_bound_has_a_case_and_every_case_a_bound():
    keys = set()
    for cases, outs in ((FWD, ("O", "O+O_lo", "lse")), (BWD, ("delta", "dQ", "dK", "dV"))):
        keys |= {(AR.out_name(o, c), c["kind"], a) for c in cases for o in outs for a in ("model", "f64")
                 if not (o == "O+O_lo" and c["kind"] == "f32")}
    assert keys == set(AR.BOUNDS)
    for (out, kind, against), (bmax, bmean) in AR.BOUNDS.items():
        assert 0 <= bmean <= bmax
        if kind == "f32":
            assert bmax <= 1e-5 and AR.BOUNDS[(out, kind, "model")] == AR.BOUNDS[(out, kind, "f64")]
        if kind == "bf16" and against == "model":
            assert bmax <= AR.ONE_ULP


@pytest.mark.parametrize("c", FWD + BWD, ids=[AR.case_id(c) for c in FWD] + ["bwd-" + AR.case_id(c) for c in BWD])
def test_standin_is_within_every_bound(c):
    backward = any(c is b for b in BWD)
    got = run_case(c, backward, "standin")
    refs = {"model": run_case(c, backward, "model"), "f64": run_case(c, backward, "f64")}
    rows = AR.measure(got, refs, c, AR.n_seq(c, N_CU), tops_of(c, backward))
    AR.report(rows)
    assert not AR.outside(rows), AR.outside(rows)


# ---- each emulated defect moves its region by at least 10x the bound ---------------------------------------------------------------
def _find(cases, **kw):
    return [c for c in cases if all(c[k] == v for k, v in kw.items())][0]


DEFECT_TABLE = [
    # defect, backward, case, output, region
    ("mask_off_by_one", False, dict(Lq=450, Lk=450, p=0.1), "O", "all"),
    ("mask_off_by_one", False, dict(Lq=129, Lk=65, p=0.0, kind="f32"), "O", "sh1.2"),
    ("p_trunc", False, dict(Lq=450, Lk=450, p=0.1), "O", "all"),
    ("p_trunc", False, dict(Lq=129, Lk=65, p=0.1, kind="bf16", gain=1), "O", "tail32"),
    ("denom_after_dropout", False, dict(Lq=450, Lk=152, p=0.1, ldo=520), "O", "tail128"),
    ("denom_after_dropout", False, dict(Lq=384, Lk=97, p=0.1, kind="f32"), "lse", "all"),
    ("keep_stride_lpk", False, dict(Lq=450, Lk=545, p=0.1, gain=1), "O", "sh1.7"),
    ("keep_stride_lpk", True, dict(Lq=289, Lk=31, p=0.1, olo=True), "dQ", "tail32"),
    ("keep_stride_lpk", True, dict(Lq=289, Lk=31, p=0.1, olo=True), "dV", "tail32"),
    ("bwd_keep_group_shift", True, dict(Lq=450, Lk=450, p=0.1, olo=True), "dQ", "sh0.0"),
    ("bwd_keep_group_shift", True, dict(Lq=450, Lk=450, p=0.1, olo=True), "dK", "all"),
    ("bwd_keep_group_shift", True, dict(Lq=129, Lk=65, p=0.1, kind="f32"), "dV", "tail32"),
    ("no_rescale_chunk", False, dict(Lq=450, Lk=545, gain=4), "O_big", "all"),
    ("lse_natural", False, dict(Lq=385, Lk=33, p=0.0), "lse", "tail32"),
    ("no_scale_q", True, dict(Lq=257, Lk=33, p=0.0, olo=True), "dQ", "tail32"),
    # (delta is the region it touches: in dQ the same defect is 6 times the mean bound, under the ten that count as caught here)
    ("delta_no_lo", True, dict(Lq=450, Lk=450, vshift=1.5), "delta", "all"),
]


@pytest.mark.parametrize("defect,backward,sel,out,region", DEFECT_TABLE)
def test_each_emulated_defect_exceeds_its_region_bound(defect, backward, sel, out, region):
    c = _find(BWD if backward else FWD, **sel)
    got, ref = run_case(c, backward, "model", defect), run_case(c, backward, "model")
    o = out[:-4] if out.endswith("_big") else out
    mx, mn = AR.region_stats(got[o], ref[o], AR.regions_of(o, c, AR.n_seq(c, N_CU)))[region]
    bmax, bmean = AR.BOUNDS[(out, c["kind"], "model")]
    print(f"{defect} on {AR.case_id(c)} {out}/{region}: moves {mx:.2e} / {mn:.2e} = {mx / bmax:.1f} x / {mn / bmean:.1f} x the bound "
          f"({bmax:.1e}, {bmean:.1e})")
    assert mx >= 10 * bmax or mn >= 10 * bmean, (defect, mx, mn, bmax, bmean)


def test_every_defect_is_in_the_table_and_none_is_the_reference():
    assert {d for d, *_ in DEFECT_TABLE} == set(AR.DEFECTS)
    with pytest.raises(ValueError):
        AR.Ref(True, defect="nonsense")
    # the reference itself masks: the poison in the padding rows does not move it by a bit
    c = AR.case(129, 65, p=0.1)
    Lp_q, Lp_k = AR.pads(c, True)
    outs = []
    for poison in (False, True):
        Q, Kp, Vp, dO = AR.inputs(c, Lp_q, Lp_k, poison=poison)
        f = AR.Ref(True).fwd(Q[:, :, :129], Kp, Vp, AR.keep_of(c, Lp_k), 65)
        outs.append((f, AR.Ref(True).bwd(Q[:, :, :129], Kp, Vp, dO[:, :, :129], f["O"], f["O_lo"], f["lse"], AR.keep_of(c, Lp_k), 65)))
    assert all(torch.equal(outs[0][i][k], outs[1][i][k]) for i in (0, 1) for k in outs[0][i])


# ---- the mask probes' inputs: every keep bit is observable on its own ---------------------------------------------------------------
def _probe_bits(Lq, Lk, n, H):
    """(seq, head, q, k): all bits of the last row, of the last key and of the first row of a second 32-row / 32-key group, and
    1000 random ones"""
    g = torch.Generator().manual_seed(3)
    bits = [(n - 1, H - 1, Lq - 1, k) for k in range(Lk)] + [(n - 1, H - 1, q, Lk - 1) for q in range(Lq)]
    bits += [(0, 0, 32, k) for k in range(Lk)] + [(0, 0, q, min(32, Lk - 1)) for q in range(Lq)]
    r = torch.stack([torch.randint(0, m, (1000,), generator=g) for m in (n, H, Lq, Lk)], 1).tolist()
    return bits + [tuple(x) for x in r]


@pytest.mark.parametrize("Lq,Lk", AR.PROBE_SHAPES)
@pytest.mark.parametrize("which", ["fwd", "dkv", "dq"])
def test_flipping_one_keep_bit_moves_its_element_by_four_ulps(which, Lq, Lk):
    """... and, for the dq probe, no element of its launches is a near-cancellation (attn_train_ref.probe_inputs): each is at least
    an eighth of the magnitudes summed into it"""
    n, H, p = 2, 8, AR.PROBE_P[which]
    mk = lambda nn, hh, lq, lk, fixed=None: AR.Keep(AR.SITE, nn, hh, lq, lk, p, fixed=fixed)      # noqa: E731
    keep = mk(n, H, Lq, Lk).mask()
    r = AR.Ref(True)
    full = {}
    for blk in AR.probe_blocks(which, Lk):
        Q, Kp, Vp, dO = AR.probe_inputs(which, Lq, Lk, "bf16", Lq, Lk, n, H, block=blk)
        f = r.fwd(Q, Kp, Vp, mk(n, H, Lq, Lk), Lk)
        full[blk] = (Q, Kp, Vp, dO, f, f["lse"].to(torch.float32))
        if which == "dq":
            b = r.bwd(Q, Kp, Vp, dO, f["O"], f["O_lo"], f["lse"].to(torch.float32), mk(n, H, Lq, Lk), Lk)
            # |x| against the sum of the magnitudes it is made of: P keep scale dPd and P delta over the keys of the element
            P = torch.exp2((Q.double() @ Kp.double().transpose(-1, -2)) * AR.LOG2E - f["lse"].unsqueeze(-1))
            dPd = dO.double() @ Vp.double().transpose(-1, -2)
            mags = 0.125 * ((P * (keep * mk(n, H, Lq, Lk).scale * dPd + b["delta"].unsqueeze(-1))) @ Kp.double())
            cond = float((b["dQ"].abs() / mags)[mags > 0].min())       # (both live bits of a 2-key last block dropped: delta = 0, x = 0)
            print(f"dq probe at {Lq} x {Lk}, block {blk}: the smallest element is {cond:.3f} of the magnitudes summed into it")
            assert cond >= 0.125
    worst = math.inf
    for s, h, q, k in _probe_bits(Lq, Lk, n, H):
        Q, Kp, Vp, dO, f, lse = full[k // 64 if which == "dq" else None]
        vals = []
        for flip in (False, True):
            if which == "dkv":      # one key column: dV[k][q % 64]
                m = keep[s:s + 1, h:h + 1, :, k:k + 1].clone()
                m[0, 0, q, 0] ^= flip
                b = r.bwd(Q[s:s + 1, h:h + 1], Kp[s:s + 1, h:h + 1, k:k + 1], Vp[s:s + 1, h:h + 1, k:k + 1], dO[s:s + 1, h:h + 1],
                          f["O"][s:s + 1, h:h + 1], f["O_lo"][s:s + 1, h:h + 1], lse[s:s + 1, h:h + 1], mk(1, 1, Lq, 1, m), 1)
                vals.append(b["dV"][0, 0, 0, q % 64])
            else:                   # one query row: O[q][k % 64] or dQ[q][k % 64]
                m = keep[s:s + 1, h:h + 1, q:q + 1].clone()
                m[0, 0, 0, k] ^= flip
                kp = mk(1, 1, 1, Lk, m)
                sl = (slice(s, s + 1), slice(h, h + 1), slice(q, q + 1))
                if which == "fwd":
                    vals.append(r.fwd(Q[sl], Kp[s:s + 1, h:h + 1], Vp[s:s + 1, h:h + 1], kp, Lk)["O"][0, 0, 0, k % 64])
                else:
                    b = r.bwd(Q[sl], Kp[s:s + 1, h:h + 1], Vp[s:s + 1, h:h + 1], dO[sl], f["O"][sl], f["O_lo"][sl], lse[sl], kp, Lk)
                    vals.append(b["dQ"][0, 0, 0, k % 64])
        a, b_ = vals
        worst = min(worst, float((a - b_).abs() / AR.bf16_ulp(torch.maximum(a.abs(), b_.abs()))))
    print(f"{which} probe at {Lq} x {Lk}: the least move of an element by one keep bit is {worst:.1f} bf16 ulps")
    assert worst >= 4.0
