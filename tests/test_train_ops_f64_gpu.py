"""The training step's row-block, weight-gradient and element-wise kernels against float64, region by region (MI355X only):
tcdiff_row_fwd / _bwd / _param_reduce, tcdiff_act_drop(_bwd), tcdiff_cast_transpose(_multi) (csrc/train_ops.hip),
tcdiff_gemm_splitk / _tn / _tn_grouped and the fused activation epilogues of tcdiff_gemm_tile (csrc/gemm.hip) against
tests/train_ops_ref.py, called through tcdiff_amd.kernels only.

Every output of every case, region by region (train_ops_ref.row_regions, vec_regions, film_regions, tile_regions, band_regions;
max-abs and mean-abs scaled by the reference's top magnitude), twice: against the float64 value rounded once to the storage type
("model") and unrounded ("f64").  Rules of every case:

  * every figure is printed before anything is asserted (check());
  * sentinels: every output buffer has one row more than the launch writes, and a leading dimension wider than the block where the
    layout has one; `partials` is exactly chunks x nseq rows plus a sentinel row; the columns of d_film outside the block, the
    sentinel rows and columns must survive, and every input is bit-unchanged after the call;
  * exact items carry no tolerance: cast_transpose's bits and zero pads, the zero pattern of every dropout output, integer-operand
    GEMMs (init + product bit for bit, for every `splits` and every group), the fused epilogues against the separate launches, and
    row_fwd's outputs, d_z and d_xres in two runs;
  * accumulating outputs (d_film, g_*, the row_param_reduce targets, colsum, GEMM outputs) start from non-zero values and are compared
    as start + reference;
  * refusals return before any launch with the documented code and leave the outputs alone.

A grouped case restates the launcher's split (train_ops_ref.grouped_regime) and skips, with the numbers, where this chip's CU count
moves it out of the regime it is meant to reach; on 256 CUs none skips (asserted by the report)."""
import pytest
import torch

import train_ops_ref as TR

pytestmark = pytest.mark.gpu

from tcdiff_amd import _lib as L  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402

DEV = "cuda"
SENT = 7.0
WORST, SKIPPED, REGIMES = {}, [], []
ROWS = TR.row_groups()
ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = "(code -1)", "(code -2)", "(code -4)"


def n_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def mode(kind):
    dt = K.dtype_id(kind)
    return dt, K.TORCH_DT[dt]


def seed_dev():
    return torch.tensor(TR.SEED, dtype=torch.int32, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def sent(rows, cols, dtype=torch.float32):
    return torch.full((rows, cols), SENT, device=DEV, dtype=dtype)


def all_sent(t):
    return bool((t.float() == SENT).all())


def check(rows, frob=(), exact=()):
    """every figure is printed before anything is asserted: the case's worst max / mean per output (the region classes are kept for
    the report), the worst whole-tensor Frobenius ratio per output against its limit, the count of exact items"""
    TR.report(rows, WORST)
    fr = {}
    for what, f, lim in frob:
        k = what.split(" ")[-1]
        fr[k] = max(fr.get(k, (0.0, lim)), (f, lim))
    print("frobenius vs f64: " + (" ".join(f"{k}={f:.1e}(<{lim:.0e})" for k, (f, lim) in fr.items()) or "-") +
          f" | exact items: {sum(bool(ok) for _, ok in exact)} of {len(exact)} hold" + "".join(f"\n  VIOLATED: {w}" for w, ok in exact if not ok))
    bad = TR.outside(rows)
    assert not bad, bad[:10]
    assert all(f < lim for _, f, lim in frob), [x for x in frob if not x[1] < x[2]]
    assert all(ok for _, ok in exact), [w for w, ok in exact if not ok]


def refused(code, fn, *outputs):
    """fn is refused with the documented code and no output buffer is touched"""
    before = [o.clone() for o in outputs]
    with pytest.raises(L.TcdiffError) as e:
        fn()
    torch.cuda.synchronize()
    assert code in str(e.value), str(e.value)
    assert all(same_bits(a, b) for a, b in zip(before, outputs))


# ---- the row block ----------------------------------------------------------------------------------------------------------------
class RowRun:
    """device inputs of one case and its launches into sentinel buffers"""

    def __init__(self, c):
        self.c, self.x = c, TR.row_inputs(c)
        self.dt, self.T = mode(c["kind"])
        self.M, self.nseq = c["nseq"] * c["L"], c["nseq"]
        x = self.x
        self.d = {k: x[k].to(DEV).contiguous() for k in ("z", "xres", "bias", "ln_g", "ln_b", "nln_g", "nln_b", "film", "rope", "d_xn")}
        self.d["d_h"], self.d["d_rot"] = x["d_h"].to(DEV).to(self.T), x["d_rot"].to(DEV).to(self.T)
        self.d["seed"] = seed_dev()
        self.before = {k: v.clone() for k, v in self.d.items()}
        thr, sc = K.drop_params(TR.P_DROP)
        pm, pb = TR.pos_of(c)
        d = self.d
        self.common = dict(flags=c["flags"], M=self.M, L=c["L"], z=d["z"], bias=d["bias"], ln_g=d["ln_g"], ln_b=d["ln_b"], ln_eps=TR.LN_EPS,
                           film=d["film"][:, 1024:], film_ld=2048, xres=d["xres"], nln_g=d["nln_g"], nln_b=d["nln_b"], nln_eps=TR.NLN_EPS,
                           rope=d["rope"], pos_mod=pm, pos_base=pb, seed=d["seed"], drop_thr=thr, drop_scale=sc, site_pre=TR.SITE_PRE,
                           site_post=TR.SITE_POST)

    def inputs_unchanged(self):
        return all(same_bits(self.before[k], v) for k, v in self.d.items())

    def fwd(self, **over):
        M = self.M
        o = dict(xout=sent(M + 1, 512), hout=sent(M + 1, 512, self.T), rout=sent(M + 1, 512, self.T))
        K.row_fwd(self.dt, K.row_args(**{**self.common, **o, **over}))
        torch.cuda.synchronize()
        return o

    def grads(self):
        return {k: self.d[k] for ch, k in (("x", "d_xn"), ("h", "d_h"), ("r", "d_rot")) if ch in self.c["grads"]}

    def bwd(self, *, direct, **over):
        c, M, nseq = self.c, self.M, self.nseq
        nb = c["chunks"] * nseq
        o = dict(d_z=sent(M + 1, 512, torch.float32 if c["dz_f32"] else self.T), d_xres=sent(M + 1, 512))
        film = sent(nseq + 1, 2048)
        film[:nseq] = self.x["start_film"].to(DEV)
        extra = {}
        if direct:
            live = TR.live_outputs(c)
            g = {k: sent(2, 512) for k in TR.ROW_OUT_B[3:]}
            for k in g:
                g[k][0] = self.x["start_" + k].to(DEV)
            extra = {k: (v if k in live else None) for k, v in g.items()}
        else:
            part = sent(nb + 1, 5 * 512)
            extra = dict(partials=part)
        K.row_bwd(self.dt, K.row_args(**{**self.common, **self.grads(), **o, "d_film": film[:, 1024:], "dfilm_ld": 2048, "chunks": c["chunks"],
                                         "dz_f32": int(c["dz_f32"]), **extra, **over}))
        if not direct:
            g = {k: sent(2, 512) for k in TR.ROW_OUT_B[3:]}
            for k in g:
                g[k][0] = self.x["start_" + k].to(DEV)
            K.row_param_reduce(part, nb, *[g[k] for k in TR.ROW_OUT_B[3:]])
        torch.cuda.synchronize()
        o.update(film=film, g=g, part=None if direct else part)
        return o


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[g for g, _ in ROWS])
def test_row_block(i):
    """one case, or a flag set's plain cases at every shape of train_ops_ref.SHAPES (figures printed as the worst over the shapes; a
    violation names its case)"""
    rows, frob, exact = [], [], []
    for c in ROWS[i][1]:
        a, b, e = run_row_case(c)
        cid = TR.row_case_id(c)
        rows += [(key, f"{cid}:{reg}", mx, mn) for key, reg, mx, mn in a]
        frob += [(f"{cid} {w}", f, lim) for w, f, lim in b]
        exact += [(f"{cid} {w}", ok) for w, ok in e]
    check(rows, frob, exact)


def run_row_case(c):
    r = RowRun(c)
    M, nseq, kind = r.M, r.nseq, c["kind"]
    refs = TR.row_refs(c, r.x)
    live = TR.live_outputs(c)
    exact, frob, lim = [], [], TR.FROBENIUS[kind]
    f1, f2 = r.fwd(), r.fwd()
    got = {}
    for k in TR.ROW_OUT_F:
        exact.append((f"{k}: the sentinel row survives", all_sent(f1[k][M:])))
        if k in live:
            got[k] = f1[k][:M]
            exact.append((f"{k}: equal bits in two runs", same_bits(f1[k], f2[k])))
            if not c["variant"]:
                frob.append((k, TR.frobenius(got[k], refs["f64"][k]), lim[k]))
        else:
            exact.append((f"{k}: not stored, untouched", all_sent(f1[k])))
    rows = TR.measure_row(c, got, refs)
    for direct in (False, True):
        b1, b2 = r.bwd(direct=direct), r.bwd(direct=direct)
        tag = "direct" if direct else "partials"
        got = {"d_z": b1["d_z"][:M], "d_xres": b1["d_xres"][:M], "d_film": b1["film"][:nseq, 1024:]}
        got.update({k: v[:1] for k, v in b1["g"].items()})
        exact += [(f"{tag} d_z: equal bits in two runs", same_bits(b1["d_z"], b2["d_z"])),
                  (f"{tag} d_xres: equal bits in two runs", same_bits(b1["d_xres"], b2["d_xres"])),
                  (f"{tag} d_z, d_xres: the sentinel row survives", all_sent(b1["d_z"][M:]) and all_sent(b1["d_xres"][M:])),
                  (f"{tag} d_film: the row after the last sequence and the columns outside the block survive",
                   all_sent(b1["film"][nseq:]) and same_bits(b1["film"][:nseq, :1024], r.x["start_film"][:, :1024].to(DEV))),
                  (f"{tag} g_*: the sentinel rows survive", all(all_sent(v[1:]) for v in b1["g"].values()))]
        if "d_xres" not in live:
            exact.append((f"{tag} d_xres: no residual, untouched", all_sent(b1["d_xres"])))
        if "d_film" not in live:
            exact.append((f"{tag} d_film: no FiLM, untouched", same_bits(b1["film"][:nseq], r.x["start_film"].to(DEV))))
        for k in TR.ROW_OUT_B[3:]:
            if k not in live:
                exact.append((f"{tag} {k}: not live, keeps its start", same_bits(b1["g"][k][0], r.x["start_" + k].to(DEV))))
        if not direct:
            part = b1["part"]
            exact += [("partials: the sentinel row survives", all_sent(part[-1:])),
                      ("partials: every block wrote a finite row", bool(part[:-1].isfinite().all()) and not bool((part[:-1] == SENT).all(1).any()))]
        if not c["variant"]:
            for k in ("d_z", "d_xres", "d_film") + TR.ROW_OUT_B[3:]:
                if k in live:
                    start = r.x["start_film"][:, 1024:] if k == "d_film" else (r.x["start_" + k] if k.startswith("g_") else 0.0)
                    name = "g" if k.startswith("g_") else ("d_z32" if k == "d_z" and c["dz_f32"] else k)
                    frob.append((f"{tag} {k}", TR.frobenius(got[k].double().cpu() - start, refs["f64"][k] - start), lim[name]))
        rows += TR.measure_row(c, got, refs)
    exact.append(("inputs bit-unchanged", r.inputs_unchanged()))
    return rows, frob, exact


@pytest.mark.parametrize("n_blocks", TR.REDUCE_BLOCKS)
def test_row_param_reduce(n_blocks):
    part = sent(n_blocks + 1, 2560)
    part[:n_blocks] = TR.rnd(50 + n_blocks, n_blocks, 2560).to(DEV)
    start = TR.rnd(49, 5, 512)
    tgt = sent(6, 512)
    tgt[:5] = start.to(DEV)
    before = part.clone()
    K.row_param_reduce(part, n_blocks, tgt[0], tgt[1], None, tgt[3], tgt[4])
    torch.cuda.synchronize()
    ref = start.double() + part[:n_blocks].double().cpu().sum(0).reshape(5, 512)
    ref[2] = start[2].double()
    refs = {h: {"reduce": TR.store(ref, "f32", h)} for h in ("model", "f64")}
    rows = TR.measure({"reduce": tgt[:5]}, refs, "f32", lambda o: [("all", None, slice(0, 512)), ("half0", None, slice(0, 256)),
                                                                   ("half1", None, slice(256, 512))])
    check(rows, exact=[("a NULL target is skipped", same_bits(tgt[2], start[2].to(DEV))), ("the sentinel row survives", all_sent(tgt[5:])),
                       ("partials bit-unchanged", same_bits(part, before))])


def test_row_block_refusals():
    c = TR.row_case("dec_self", (2, 7, 1), "bf16")
    r = RowRun(c)
    M = r.M
    o = dict(xout=sent(M + 1, 512), hout=sent(M + 1, 512, r.T), rout=sent(M + 1, 512, r.T))
    b = dict(d_z=sent(M + 1, 512, r.T), d_xres=sent(M + 1, 512), partials=sent(3, 2560), chunks=1, d_film=sent(3, 2048)[:, 1024:], dfilm_ld=2048)
    outs = list(o.values()) + [b["d_z"], b["d_xres"], b["partials"]]
    fwd = lambda **kw: (lambda: K.row_fwd(r.dt, K.row_args(**{**r.common, **o, **kw})))
    bwd = lambda **kw: (lambda: K.row_bwd(r.dt, K.row_args(**{**r.common, **r.grads(), **b, **kw})))
    refused(ERR_ARG, fwd(L=5), *outs)                                      # M % L != 0
    refused(ERR_ARG, bwd(L=5), *outs)
    refused(ERR_ARG, bwd(chunks=0), *outs)
    refused(ERR_ARG, bwd(chunks=-1), *outs)
    refused(ERR_ARG, fwd(film_ld=2046), *outs)
    refused(ERR_ARG, bwd(dfilm_ld=2046), *outs)
    refused(ERR_ARG, fwd(xres=None), *outs)                                # a required pointer missing
    refused(ERR_ARG, fwd(rout=None), *outs)
    refused(ERR_ARG, bwd(d_xres=None), *outs)
    refused(ERR_ALIGN, fwd(z=torch.zeros(M * 512 + 4, device=DEV)[1:]), *outs)       # a pointer off 16-byte alignment
    refused(ERR_ALIGN, bwd(d_z=sent(M + 2, 512, r.T).view(-1)[2:]), *outs)
    x = sent(4, 510)
    refused(ERR_ARG, lambda: K.pos_drop(x, 4, 510, None, 1, seed_dev(), 9, *K.drop_params(0.1)), x)


# ---- activation + dropout ---------------------------------------------------------------------------------------------------------
def flat_view(rows, ld, dtype, off):
    """a [rows, ld] view `off` elements into a sentinel-filled flat buffer that also holds one row after it"""
    flat = torch.full((off + (rows + 1) * ld,), SENT, device=DEV, dtype=dtype)
    return flat, flat[off:off + rows * ld].view(rows, ld)


def act_launch(kind, src, act, shape, p, extreme=False):
    rows_, cols, ld_a, ld_y, off = shape
    dt, T = mode(kind)
    S = torch.float32 if src == "f32" else T
    a, dy = TR.act_inputs(rows_, cols, kind, src, extreme=extreme)
    fa, av = flat_view(rows_, ld_a, S, off)
    fdy, dyv = flat_view(rows_, ld_y, T, off)
    av[:, :cols], dyv[:, :cols] = a.to(DEV).to(S), dy.to(DEV).to(T)
    fa0, fdy0 = fa.clone(), fdy.clone()
    fy, yv = flat_view(rows_, ld_y, T, off)
    fda, dav = flat_view(rows_, ld_a, S, off)
    thr, sc = K.drop_params(p)
    sd = seed_dev()
    K.act_drop(dt, av, ld_a, yv, ld_y, rows_, cols, act, sd, TR.ACT_SITE, thr, sc)
    K.act_drop_bwd(dt, av, ld_a, dyv, ld_y, dav, rows_, cols, act, sd, TR.ACT_SITE, thr, sc)
    torch.cuda.synchronize()
    y64, da64 = TR.Ops().act_drop(a, dy, act, p, TR.ACT_SITE, ld_y)
    ext = "_ext" if extreme else ""
    refs = {h: {"act_y": TR.store(y64, kind, h), "act_da": TR.store(da64, src, h)} for h in ("model", "f64")}
    regs = lambda o: [("all", None, slice(0, cols))]
    rows = TR.measure({"act_y": yv[:, :cols]}, refs, kind, regs, lambda o: o + ext)
    rows += TR.measure({"act_da": dav[:, :cols]}, refs, kind, regs, lambda o: o + ("_f32src" if kind != src else "") + ext)
    keep = TR.keep_mask(TR.ACT_SITE, rows_, cols, p).to(DEV) if p > 0 else torch.ones(rows_, cols, dtype=torch.bool, device=DEV)
    yf, daf = yv[:, :cols].float(), dav[:, :cols].float()
    tag = f"{TR.ACT_NAMES[act]} {shape} p={p}{ext}"
    exact = [(f"{tag}: y, da finite", bool(yf.isfinite().all()) and bool(daf.isfinite().all())),
             (f"{tag}: dropped elements are zero", bool((yf[~keep] == 0).all()) and bool((daf[~keep] == 0).all())),
             # (below the smallest normal the kernels' v_exp / v_rcp flush to zero: silu(-100) = -3.7e-42 is a zero of either sign)
             (f"{tag}: kept elements are zero only where the reference is zero or underflows",
              bool(((yf != 0) | (y64.abs().to(DEV) < 2.0 ** -126) | ~keep).all())),
             (f"{tag}: columns up to the leading dimension are zeros",
              bool((yv[:, cols:].float() == 0).all()) and bool((dav[:, cols:].float() == 0).all())),
             (f"{tag}: nothing written in front of or after the tensors",
              all(all_sent(f[:f.numel() - (rows_ + 1) * l]) and all_sent(f[-l:]) for f, l in ((fy, ld_y), (fda, ld_a)))),
             (f"{tag}: inputs bit-unchanged", same_bits(fa, fa0) and same_bits(fdy, fdy0))]
    frob = []
    if not extreme:
        lim = TR.FROBENIUS[kind]["act"]
        lim_da = TR.FROBENIUS["f32"]["act"] if src == "f32" else lim          # an fp32 da from an fp32 source is held to the f32 limit
        frob = [(f"{tag} y", TR.frobenius(yv[:, :cols], y64), lim), (f"{tag} da", TR.frobenius(dav[:, :cols], da64), lim_da)]
    return rows, frob, exact


@pytest.mark.parametrize("act", list(TR.ACT_NAMES), ids=list(TR.ACT_NAMES.values()))
@pytest.mark.parametrize("kind,src", TR.ACT_TYPES, ids=[f"{k}-src{s}" for k, s in TR.ACT_TYPES])
def test_act_drop(kind, src, act):
    rows, frob, exact = [], [], []
    for shape in TR.ACT_SHAPES:
        for p in (0.1, 0.0):
            a, b, c = act_launch(kind, src, act, shape, p)
            rows, frob, exact = rows + a, frob + b, exact + c
    a, b, c = act_launch(kind, src, act, TR.ACT_SHAPES[0], 0.0, extreme=True)
    check(rows + a, frob + b, exact + c)


# ---- cast / transpose -------------------------------------------------------------------------------------------------------------
def as_T(v, T):
    """float32 CPU values -> T by round-to-nearest-even (train_ops_ref's rounding, not torch's cast)"""
    if T == torch.float32:
        return v.to(torch.float32)
    return torch.from_numpy(TR.bf16_rne(v.to(torch.float32)).reshape(tuple(v.shape))).to(torch.bfloat16)


def ct_buffers(rows_, cols, kt, T):
    cp, rp = K.round_up(cols, kt), K.round_up(rows_, kt)
    return cp, rp, sent(rows_ + 1, cp + 8, T), sent(cols + 1, rp + 8, T)


def ct_exact(tag, src_vals, rows_, cols, cp, rp, dst, dstT, T):
    want = as_T(src_vals[:, :cols], T).to(DEV)
    out = []
    if dst is not None:
        out += [(f"{tag} dst: the reference's bits", same_bits(dst[:rows_, :cols], want)),
                (f"{tag} dst: pads are zero", bool((dst[:rows_, cols:cp].float() == 0).all())),
                (f"{tag} dst: sentinel row and columns survive", all_sent(dst[rows_:]) and all_sent(dst[:, cp:]))]
    if dstT is not None:
        out += [(f"{tag} dstT: the reference's bits", same_bits(dstT[:cols, :rows_], want.t().contiguous())),
                (f"{tag} dstT: pads are zero", bool((dstT[:cols, rows_:rp].float() == 0).all())),
                (f"{tag} dstT: sentinel row and columns survive", all_sent(dstT[cols:]) and all_sent(dstT[:, rp:]))]
    return out


@pytest.mark.parametrize("src_f32", [True, False], ids=["src-f32", "src-T"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_cast_transpose(kind, src_f32):
    dt, T = mode(kind)
    kt = K.k_tile(dt)
    rows, exact = [], []
    for n, (rows_, cols, ld) in enumerate(TR.CAST_SHAPES):
        src = TR.rnd(60 + n, rows_, ld)
        srcd = src.to(DEV) if src_f32 else as_T(src, T).to(DEV)
        vals = srcd.float().cpu()
        cp, rp, dst, dstT = ct_buffers(rows_, cols, kt, T)
        start = TR.rnd(70 + n, cols)
        cs = sent(2, cols)
        cs[0] = start.to(DEV)
        before = srcd.clone()
        K.cast_transpose(dt, srcd, rows_, cols, ld, dst=dst, ld_dst=cp + 8, cols_pad=cp, dstT=dstT, ld_dstT=rp + 8, rows_pad=rp, colsum=cs[0])
        torch.cuda.synchronize()
        tag = f"{rows_}x{cols} ld {ld}"
        exact += ct_exact(tag, vals, rows_, cols, cp, rp, dst, dstT, T)
        exact += [(f"{tag}: source bit-unchanged", same_bits(srcd, before)), (f"{tag} colsum: the sentinel row survives", all_sent(cs[1:]))]
        ref = TR.Ops().colsum(vals[:, :cols], start).reshape(1, cols)
        refs = {h: {"colsum": TR.store(ref, "f32", h)} for h in ("model", "f64")}
        rows += TR.measure({"colsum": cs[:1]}, refs, kind, lambda o: TR.band_regions(1, cols))
    # the colsum-only call (the bias gradient on the TN path) over 1000 rows on top of a non-zero start
    rows_, cols, ld = TR.CAST_SHAPES[2]
    cs2 = sent(2, cols)
    cs2[0] = start.to(DEV)
    K.cast_transpose(dt, srcd, rows_, cols, ld, colsum=cs2[0])
    torch.cuda.synchronize()
    rows += TR.measure({"colsum": cs2[:1]}, refs, kind, lambda o: TR.band_regions(1, cols))
    exact.append(("colsum-only: the sentinel row survives", all_sent(cs2[1:])))
    # the dst-only cast with cols_pad == cols < ld_dst: nothing past the columns is written
    d3 = sent(rows_ + 1, 96, T)
    K.cast_transpose(dt, srcd, rows_, cols, ld, dst=d3, ld_dst=96, cols_pad=cols)
    torch.cuda.synchronize()
    exact += [("dst-only: the reference's bits", same_bits(d3[:rows_, :cols], as_T(vals[:, :cols], T).to(DEV))),
              ("dst-only: columns cols .. ld_dst and the sentinel row survive", all_sent(d3[:, cols:]) and all_sent(d3[rows_:]))]
    check(rows, exact=exact)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_cast_transpose_multi_over_the_same_table(kind):
    dt, T = mode(kind)
    kt = K.k_tile(dt)
    ents, keep, exact = [], [], []
    for n, (rows_, cols, ld) in enumerate(TR.CAST_SHAPES):
        srcd = TR.rnd(60 + n, rows_, ld).to(DEV)
        cp, rp, dst, dstT = ct_buffers(rows_, cols, kt, T)
        ents.append(dict(src=srcd, rows=rows_, cols=cols, ld_src=ld, dst=dst, ld_dst=cp + 8, cols_pad=cp, dstT=dstT, ld_dstT=rp + 8, rows_pad=rp))
        keep.append((srcd, rows_, cols, cp, rp, dst, dstT))
    rows_, cols, ld = TR.CAST_SHAPES[2]                                          # and one dst-only entry
    d3 = sent(rows_ + 1, 96, T)
    ents.append(dict(src=keep[2][0], rows=rows_, cols=cols, ld_src=ld, dst=d3, ld_dst=96, cols_pad=cols))
    K.cast_transpose_multi(dt, K.ct_table(dt, ents, DEV))
    torch.cuda.synchronize()
    for srcd, r_, c_, cp, rp, dst, dstT in keep:
        exact += ct_exact(f"multi {r_}x{c_}", srcd.cpu(), r_, c_, cp, rp, dst, dstT, T)
    exact += [("multi dst-only: the reference's bits", same_bits(d3[:rows_, :cols], as_T(keep[2][0].cpu()[:, :cols], T).to(DEV))),
              ("multi dst-only: columns cols .. ld_dst and the sentinel row survive", all_sent(d3[:, cols:]) and all_sent(d3[rows_:]))]
    check([], exact=exact)


# ---- weight gradients -------------------------------------------------------------------------------------------------------------
def tn_problem(shape, kind, data, seed):
    """one weight gradient's device operands (token-major, read in place from wider buffers) and its sentinel output"""
    _, T = mode(kind)
    n_out, n_in, rows_ = shape
    dY, X, init = TR.gemm_operands(shape, kind, data, seed)
    dYd, Xd = dY.to(DEV).to(T), X.to(DEV).to(T)
    out = sent(n_out + 1, n_in + 8)
    out[:n_out, :n_in] = init.to(DEV)
    return dict(dY=dYd, X=Xd, out=out, before=(dYd.clone(), Xd.clone()), shape=shape,
                args=(dYd.view(-1)[64:], Xd, n_out, n_in, rows_, n_out + 128, n_in + 8, out, n_in + 8))


def gemm_check(name, kind, data, seed, pr, rows, frob, exact):
    n_out, n_in, _ = pr["shape"]
    ref = TR.gemm_ref(pr["shape"], kind, data, seed)
    got = pr["out"][:n_out, :n_in]
    exact += [(f"{name}: sentinel row and columns survive", all_sent(pr["out"][n_out:]) and all_sent(pr["out"][:, n_in:])),
              (f"{name}: operands bit-unchanged", same_bits(pr["dY"], pr["before"][0]) and same_bits(pr["X"], pr["before"][1]))]
    if data == "int":
        exact.append((f"{name}: init + product bit for bit", same_bits(got, ref.to(torch.float32).to(DEV))))
    else:
        refs = {h: {name.split(" ")[0]: TR.store(ref, "f32", h)} for h in ("model", "f64")}
        rows += TR.measure({name.split(" ")[0]: got}, refs, kind, lambda o: TR.tile_regions(n_out, n_in))
        frob.append((name + " out", TR.frobenius(got, ref), TR.FROBENIUS[kind]["gemm"]))


@pytest.mark.parametrize("data", TR.DATA)
@pytest.mark.parametrize("kind", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(TR.GROUPED))
def test_gemm_tn_grouped(name, kind, data):
    dt, _ = mode(kind)
    ok, txt = TR.grouped_regime(name, kind, n_cu())
    print(txt)
    if not ok:
        SKIPPED.append((f"{name}-{kind}-{data}", txt))
        pytest.skip(txt)
    REGIMES.append(txt)
    shapes = TR.grouped_shapes(name, kind)
    probs = [tn_problem(sh, kind, data, 20 + i) for i, sh in enumerate(shapes)]
    K.gemm_tn_grouped(dt, [p["args"] for p in probs])
    torch.cuda.synchronize()
    rows, frob, exact = [], [], []
    for i, p in enumerate(probs):
        gemm_check(f"tn_grouped {name} problem {i} {p['shape']}", kind, data, 20 + i, p, rows, frob, exact)
    check(rows, frob, exact)


def test_gemm_refusals():
    dt, _ = mode("bf16")
    p = tn_problem((128, 128, 64), "bf16", "int", 20)
    a = p["args"]
    refused(ERR_ARG, lambda: K.gemm_tn_grouped(dt, [a] * (TR.TN_MAX_PROB + 1)), p["out"])
    assert L.TN_MAX_PROB == TR.TN_MAX_PROB
    for M, N, Kd in ((100, 128, 64), (128, 100, 64), (128, 128, 32)):                     # off the 128 / k-tile grid
        bad = (a[0], a[1], M, N, Kd) + a[5:]
        refused(ERR_UNSUPPORTED, lambda: K.gemm_tn_grouped(dt, [bad]), p["out"])
        refused(ERR_UNSUPPORTED, lambda: K.gemm_tn(dt, a[0], a[1], M, N, Kd, a[5], a[6], a[7], a[8], 1), p["out"])
        assert not K.gemm_tn_ok(dt, M, N, Kd)


@pytest.mark.parametrize("data", TR.DATA)
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_gemm_tn(kind, data):
    dt, _ = mode(kind)
    rows, frob, exact = [], [], []
    for sh, splits in TR.tn_cases(kind):
        deep = TR.tn_deep(*sh, K.k_tile(dt), splits, n_cu())
        print(f"gemm_tn {sh} splits {splits} on {n_cu()} CUs: {'four' if deep else 'two'}-stage kernel")
        p = tn_problem(sh, kind, data, 30)
        K.gemm_tn(dt, *p["args"], splits)
        torch.cuda.synchronize()
        gemm_check(f"tn {sh} splits {splits}", kind, data, 30, p, rows, frob, exact)
    check(rows, frob, exact)


@pytest.mark.parametrize("data", TR.DATA)
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_gemm_splitk(kind, data):
    """the same sums from k-major operands (what cast_transpose leaves): shapes off the 128 grid, splits that do not divide the
    k-tiles, and more splits than k-tiles (clamped by the launcher)"""
    dt, T = mode(kind)
    rows, frob, exact = [], [], []
    for sh, splits in TR.splitk_cases(kind):
        n_out, n_in, rows_ = sh
        dY, X, init = TR.gemm_operands(sh, kind, data, 30)
        At = dY[:, 64:64 + n_out].t().contiguous().to(DEV).to(T)
        Wt = X[:, :n_in].t().contiguous().to(DEV).to(T)
        out = sent(n_out + 1, n_in + 9)
        out[:n_out, :n_in] = init.to(DEV)
        p = dict(dY=At, X=Wt, out=out, before=(At.clone(), Wt.clone()), shape=sh)
        K.gemm_splitk(dt, At, Wt, n_out, n_in, rows_, rows_, rows_, out, n_in + 9, splits)
        torch.cuda.synchronize()
        gemm_check(f"splitk {sh} splits {splits}", kind, data, 30, p, rows, frob, exact)
    check(rows, frob, exact)


# ---- the fused activation epilogues of gemm_tile, inside wider buffers --------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("act,p", [(TR.ACT_GELU, 0.1), (TR.ACT_RELU, 0.0), (TR.ACT_RELU, 0.1), (TR.ACT_MISH, 0.0), (TR.ACT_SILU, 0.1)])
def test_fused_epilogues_inside_wider_buffers(kind, act, p):
    """N = 512 inside 640-wide out, out2 and act_src buffers: bit-identical to gemm_tile followed by act_drop(_bwd) with cols = 512,
    ld = 640 (the separate launches zero columns 512 .. 639; the fused ones leave them alone)"""
    dt, T = mode(kind)
    M, N, Kd, ld = 300, 512, 512, 640
    A, W = TR.rnd(80, M, Kd).to(DEV).to(T), (0.05 * TR.rnd(81, N, Kd)).to(DEV).to(T)
    bias = TR.rnd(82, N).to(DEV)
    thr, sc = K.drop_params(p)
    sd, site = seed_dev(), 22
    a1, y1, a2, y2 = (sent(M + 1, ld, T) for _ in range(4))
    K.gemm_tile(dt, A, W, M, N, Kd, bias=bias, out=a1, ldc=ld)
    K.act_drop(dt, a1, ld, y1, ld, M, N, act, sd, site, thr, sc)
    K.gemm_tile(dt, A, W, M, N, Kd, bias=bias, out=a2, ldc=ld, out2=y2, ldc2=ld, act2=act, seed=sd, site=site, thr=thr, drop_scale=sc)
    dY, W2T = TR.rnd(83, M, Kd).to(DEV).to(T), (0.05 * TR.rnd(84, N, Kd)).to(DEV).to(T)
    d1, da1, da2 = (sent(M + 1, ld, T) for _ in range(3))
    K.gemm_tile(dt, dY, W2T, M, N, Kd, out=d1, ldc=ld)
    K.act_drop_bwd(dt, a1, ld, d1, ld, da1, M, N, act, sd, site, thr, sc)
    K.gemm_tile(dt, dY, W2T, M, N, Kd, out=da2, ldc=ld, act_src=a1, ld_src=ld, act2=act, seed=sd, site=site, thr=thr, drop_scale=sc)
    torch.cuda.synchronize()
    for name, s_, f_ in (("out", a1, a2), ("out2", y1, y2), ("act_src", da1, da2)):
        ne = bits(s_[:M, :N]) != bits(f_[:M, :N])
        print(f"{name}: {int(ne.sum())} of {M * N} elements differ in bits, {int((ne & (s_[:M, :N] == f_[:M, :N])).sum())} of them equal in value")
    exact = [("out: equal bits", same_bits(a1[:M, :N], a2[:M, :N])), ("out2: equal bits", same_bits(y1[:M, :N], y2[:M, :N])),
             ("act_src: equal bits", same_bits(da1[:M, :N], da2[:M, :N])),
             ("fused launches leave columns 512 .. 639 and the sentinel row alone",
              all(all_sent(t[:, N:]) and all_sent(t[M:]) for t in (a2, y2, da2))),
             ("separate launches zero columns 512 .. 639 and leave the sentinel row alone",
              all(bool((t[:M, N:].float() == 0).all()) and all_sent(t[M:]) for t in (y1, da1)))]
    if p > 0:
        frac = float((y2[:M, :N] == 0).float().mean())
        exact.append((f"the mask is live ({frac:.3f} zeros)", 0.05 < frac < 0.6))
    check([], exact=exact)


# ---- report -----------------------------------------------------------------------------------------------------------------------
def test_zz_report_worst():
    print()
    for key in sorted(WORST):
        mx, mn = max(v[0] for v in WORST[key].values()), max(v[1] for v in WORST[key].values())
        lim = TR.BOUNDS.get(key)
        print(f"WORST {key}: {mx:.2e} / {mn:.2e}" + (f"   bound {lim[0]:.2e} / {lim[1]:.2e}" if lim else "   (no bound)") + "   by region: " +
              " ".join(f"{r}={a:.1e}/{b:.1e}" for r, (a, b) in WORST[key].items()))
    for txt in sorted(set(REGIMES)):
        print("REGIME", txt)
    for name, why in SKIPPED:
        print("SKIPPED", name, why)
    print(f"CUs: {n_cu()}")
    if n_cu() == 256:
        assert not SKIPPED, SKIPPED
