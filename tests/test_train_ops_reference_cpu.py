"""The float64 reference of the training step's row-block, element-wise and weight-gradient kernels (tests/train_ops_ref.py), without
a GPU: its explicit formulas equal torch autograd in float64; the float32 stand-in of the kernels' arithmetic is inside BOUNDS in
every case and region (so the bounds are reachable before any GPU run); every DEFECT injected alone falls outside BOUNDS somewhere
(so the bounds are not loose); the restated split of the grouped weight-gradient launch covers every (problem, tile, k-tile) exactly
once and reaches, on 256 CUs, the regime each case names."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as TR

D = torch.float64
ROWS = TR.row_cases()


def close(a, b, tol=1e-12):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


# ---- explicit formulas against autograd -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grads", list(TR.GRAD_SETS))
@pytest.mark.parametrize("fs", list(TR.FLAG_SETS))
def test_row_block_formulas_equal_autograd(fs, grads):
    c = TR.row_case(fs, (3, 50, 3), "f32", grads="".join(k[2] for k in TR.GRAD_SETS[grads]))
    x = TR.row_inputs(c)
    f, nseq, L = c["flags"], c["nseq"], c["L"]
    M = nseq * L
    leaf = {k: x[k].to(D).requires_grad_(True) for k in ("z", "xres", "bias", "ln_g", "ln_b", "nln_g", "nln_b", "film")}
    sc = TR.drop_scale()
    v = leaf["z"]
    if f & TR.BIAS:
        v = v + leaf["bias"]
    if f & TR.DROP_PRE:
        v = v * TR.keep_mask(TR.SITE_PRE, M, 512) * sc
    if f & TR.LN_POST:
        v = F.layer_norm(v, (512,), leaf["ln_g"], leaf["ln_b"], TR.LN_EPS)
    if f & TR.DROP_POST:
        v = v * TR.keep_mask(TR.SITE_POST, M, 512) * sc
    if f & TR.FILM:
        s_, sh_ = leaf["film"][:, 1024:1536], leaf["film"][:, 1536:2048]
        v = ((s_ + 1)[:, None, :] * v.view(nseq, L, 512) + sh_[:, None, :]).reshape(M, 512)
    if f & TR.RES:
        v = leaf["xres"] + v
    xn = v
    u = F.layer_norm(xn, (512,), leaf["nln_g"], leaf["nln_b"], TR.NLN_EPS) if f & TR.NEXT_LN else xn
    cs = x["rope"].to(D)[3 + torch.arange(M) % L]
    rot = TR.Ops.rot(u, cs)
    loss = (xn * 0).sum()
    for k, t in (("d_xn", xn), ("d_h", u), ("d_rot", rot)):
        if k in TR.GRAD_SETS[grads]:
            loss = loss + (t * x[k].to(D)).sum()
    loss.backward()
    raw = TR.Ops().row(c, x)
    g = lambda k: leaf[k].grad if leaf[k].grad is not None else torch.zeros_like(leaf[k])
    assert close(raw["xout"], xn) and close(raw["hout"], u) and close(raw["rout"], rot)
    assert close(raw["d_z"], g("z"))
    if f & TR.RES:
        assert close(raw["d_xres"], g("xres"))
    if f & TR.BIAS:
        assert close(raw["g_bias"], g("bias"))
    assert close(raw["g_bias"], g("z").sum(0))                  # always the column sums of d_z
    if f & TR.LN_POST:
        assert close(raw["g_ln_g"], g("ln_g")) and close(raw["g_ln_b"], g("ln_b"))
    if f & TR.NEXT_LN:
        assert close(raw["g_nln_g"], g("nln_g")) and close(raw["g_nln_b"], g("nln_b"))
    if f & TR.FILM:
        assert close(raw["d_film"], g("film")[:, 1024:])


@pytest.mark.parametrize("act", list(TR.ACT_NAMES))
def test_act_drop_formulas_equal_autograd(act):
    fn = {TR.ACT_RELU: F.relu, TR.ACT_GELU: F.gelu, TR.ACT_MISH: F.mish, TR.ACT_SILU: F.silu}[act]
    a, dy = TR.act_inputs(37, 438, "f32", "f32")
    ar = a.to(D).requires_grad_(True)
    yr = fn(ar) * TR.keep_mask(TR.ACT_SITE, 37, 438) * TR.drop_scale()
    yr.backward(dy.to(D))
    y, da = TR.Ops().act_drop(a, dy, act, TR.P_DROP, TR.ACT_SITE, 448)
    assert close(y, yr) and close(da, ar.grad)
    # the extreme arguments: finite in float64, the saturated values where they are known
    e = torch.tensor(TR.EXTREME, dtype=D)
    ye, ge = TR.Ops().act(e, act), TR.Ops().act_grad(e, act)
    assert bool(ye.isfinite().all()) and bool(ge.isfinite().all())
    assert close(ye[-2:], torch.tensor([100.0, 0.0], dtype=D), 1e-30 if act == TR.ACT_RELU else 1e-12)


# ---- the stand-in inside the bounds, every defect outside -------------------------------------------------------------------------
def standin_rows_row(c, defect=None):
    x = TR.row_inputs(c)
    refs = TR.row_refs(c, x)
    s = TR.standin(defect)
    got = s.finish_row(c, x, s.row(c, x), None)
    return TR.measure_row(c, got, refs)


def act_rows(kind, src, act, shape, p, defect=None, extreme=False):
    rows_, cols, ld_a, ld_y, _ = shape
    a, dy = TR.act_inputs(rows_, cols, kind, src, extreme=extreme)
    y64, da64 = TR.Ops().act_drop(a, dy, act, p, TR.ACT_SITE, ld_y)
    refs = {h: {"act_y": TR.store(y64, kind, h), "act_da": TR.store(da64, src, h)} for h in ("model", "f64")}
    ys, das = TR.standin(defect).act_drop(a, dy, act, p, TR.ACT_SITE, ld_y)
    got = {"act_y": TR.store(ys, kind, "standin"), "act_da": TR.store(das, src, "standin")}
    regs = lambda o: [("all", None, slice(0, cols))]
    ext = "_ext" if extreme else ""
    rows = TR.measure({"act_y": got["act_y"]}, refs, kind, regs, lambda o: o + ext)
    return rows + TR.measure({"act_da": got["act_da"]}, refs, kind, regs, lambda o: o + ("_f32src" if kind != src else "") + ext)


def misc_rows():
    """the column sums of cast_transpose and row_param_reduce's folds, summed in float32"""
    rows, s = [], TR.standin()
    for kind in ("f32", "bf16"):
        for n, (rows_, cols, ld) in enumerate(TR.CAST_SHAPES):
            src = TR.rnd(60 + n, rows_, ld)[:, :cols]
            src, start = (TR.bf(src) if kind == "bf16" else src), TR.rnd(70 + n, cols)
            refs = {h: {"colsum": TR.store(TR.Ops().colsum(src, start).reshape(1, cols), "f32", h)} for h in ("model", "f64")}
            rows += TR.measure({"colsum": s.colsum(src, start).reshape(1, cols).double()}, refs, kind, lambda o: TR.band_regions(1, cols))
    for nb in TR.REDUCE_BLOCKS:
        part, start = TR.rnd(50 + nb, nb, 2560), TR.rnd(49, 5, 512)
        refs = {h: {"reduce": TR.store(start.double() + part.double().sum(0).reshape(5, 512), "f32", h)} for h in ("model", "f64")}
        rows += TR.measure({"reduce": (start + part.sum(0).reshape(5, 512)).double()}, refs, "f32", lambda o: TR.vec_regions())
    return rows


def gemm_rows(which, kind, defect=None, n_cu=256, names=("short-k", "long", "mixed", "one-unit")):
    kt, rows, s = TR.kt_of(kind), [], TR.standin(defect)
    if which == "tn_grouped":
        for name in names:
            shapes = TR.grouped_shapes(name, kind)
            ops = [TR.gemm_operands(sh, kind, "normal", 20 + i) for i, sh in enumerate(shapes)]
            outs = s.gemm_grouped([(init, dY[:, 64:64 + sh[0]], X[:, :sh[1]]) for (dY, X, init), sh in zip(ops, shapes)], kt, n_cu)
            for i, (sh, o) in enumerate(zip(shapes, outs)):
                ref = TR.gemm_ref(sh, kind, "normal", 20 + i)
                refs = {h: {"tn_grouped": TR.store(ref, "f32", h)} for h in ("model", "f64")}
                rows += [(k, f"{name}.p{i}.{reg}", a, b) for k, reg, a, b in
                         TR.measure({"tn_grouped": o.double()}, refs, kind, lambda o_: TR.tile_regions(sh[0], sh[1]))]
    else:
        for sh, splits in (TR.tn_cases(kind) if which == "tn" else TR.splitk_cases(kind)):
            dY, X, init = TR.gemm_operands(sh, kind, "normal", 30)
            o = s.gemm_split(init, dY[:, 64:64 + sh[0]], X[:, :sh[1]], kt, splits)
            ref = TR.gemm_ref(sh, kind, "normal", 30)
            refs = {h: {which: TR.store(ref, "f32", h)} for h in ("model", "f64")}
            rows += [(k, f"{sh}s{splits}.{reg}", a, b) for k, reg, a, b in
                     TR.measure({which: o.double()}, refs, kind, lambda o_: TR.tile_regions(sh[0], sh[1]))]
    return rows


ACT_SWEEP = [(kind, src, act, shape, p) for kind, src in TR.ACT_TYPES for act in TR.ACT_NAMES for shape in TR.ACT_SHAPES for p in (0.1, 0.0)]


def standin_everywhere():
    """the float32 stand-in over every case of the GPU module: [(case, rows)]"""
    out = [(TR.row_case_id(c), standin_rows_row(c)) for c in ROWS]
    out += [(f"act_drop {kind} src {src} {TR.ACT_NAMES[act]} {shape} p={p}", act_rows(kind, src, act, shape, p))
            for kind, src, act, shape, p in ACT_SWEEP]
    out += [(f"act_drop {kind} src {src} {TR.ACT_NAMES[act]} extreme", act_rows(kind, src, act, TR.ACT_SHAPES[0], 0.0, extreme=True))
            for kind, src in TR.ACT_TYPES for act in TR.ACT_NAMES]
    out.append(("colsum, reduce", misc_rows()))
    out += [(f"{which} {kind}", gemm_rows(which, kind)) for kind in ("f32", "bf16") for which in ("tn_grouped", "tn", "splitk")]
    return out


def test_standin_is_inside_the_bounds_everywhere():
    worst, bad = {}, []
    for case, rows in standin_everywhere():
        for key, reg, mx, mn in rows:
            w = worst.get(key, (0.0, 0.0))
            worst[key] = (max(w[0], mx), max(w[1], mn))
        bad += [(case,) + b for b in TR.outside(rows)]
    for key in sorted(worst):
        print(f"STANDIN {key}: {worst[key][0]:.2e} / {worst[key][1]:.2e}   bound {TR.BOUNDS[key][0]:.2e} / {TR.BOUNDS[key][1]:.2e}")
    assert sorted(worst) == sorted(TR.BOUNDS), "every BOUNDS key is exercised, and nothing else"
    assert not bad, bad[:20]


def test_bounds_keep_the_figures_that_are_not_measurements():
    for (out, kind, against), (mx, mn) in TR.BOUNDS.items():
        if not TR.bf16_store(out, kind):
            assert mx < 1e-5 and mn < 1e-5, (out, kind, against)          # an fp32 store, against the model and against float64
        elif against == "model":
            assert mx == TR.ONE_ULP and mn < 1e-5, (out, kind)
        else:
            assert mx <= 4 * TR.ONE_ULP and mn <= TR.ONE_ULP, (out, kind)


ROW_DEFECT_CASES = {
    "film_row_of_next_sequence": ("dec_self", (3, 50, 3), {}),
    "rotary_pos_without_mod": ("norm_rot", (3, 50, 3), {}),
    "ln_eps_swapped": ("dec_self", (3, 50, 3), dict(variant="_lowvar")),
    "drop_post_uses_site_pre": ("dec_self", (3, 50, 3), {}),
    "bias_grad_before_pre_dropout": ("enc_attn", (3, 50, 3), {}),
    "dz_f32_ignored": ("norm_rot", (2, 152, 8), dict(grads="hr", dz_f32=True)),
    "film_grad_stored_not_added": ("dec_ffn", (3, 50, 3), {}),
    "upper_waves_not_folded": ("dec_self", (2, 150, 8), {}),
    "last_chunk_one_row_short": ("dec_self", (2, 150, 8), {}),
}


@pytest.mark.parametrize("defect", TR.DEFECTS)
def test_every_defect_falls_outside_the_bounds(defect):
    if defect in ROW_DEFECT_CASES:
        fs, shape, kw = ROW_DEFECT_CASES[defect]
        c = TR.row_case(fs, shape, "bf16", **kw)
        bad, where = TR.outside(standin_rows_row(c, defect)), TR.row_case_id(c)
    elif defect in ("act_bwd_scale_twice", "drop_index_with_ld"):
        bad, where = TR.outside(act_rows("bf16", "f32", TR.ACT_GELU, TR.ACT_SHAPES[0], 0.1, defect)), "act_drop 37x438 bf16 / f32 source gelu"
    elif defect == "splitk_ranges_overlap":
        bad, where = TR.outside(gemm_rows("tn", "bf16", defect)), "gemm_tn bf16"
    else:
        name = "mixed" if defect == "unit_at_problem_boundary" else "long"
        bad, where = TR.outside(gemm_rows("tn_grouped", "bf16", defect, names=(name,))), f"gemm_tn_grouped {name} bf16"
    assert bad, f"{defect}: inside the bounds in every region of {where}"
    key, reg, mx, mn, lim = max(bad, key=lambda b: b[2] / b[4][0])
    print(f"{defect}: caught in {where}, {len(bad)} regions; worst {key} region {reg}: {mx:.2e}/{mn:.2e} against {lim[0]:.2e}/{lim[1]:.2e}")


# ---- the grouped split ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cu", [64, 256, 304])
@pytest.mark.parametrize("kind", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(TR.GROUPED))
def test_grouped_split_covers_every_unit_exactly_once(name, kind, n_cu):
    shapes = TR.grouped_shapes(name, kind)
    for pi, cnt in enumerate(TR.coverage(shapes, TR.kt_of(kind), n_cu)):
        assert np.array_equal(cnt, np.ones_like(cnt)), (pi, np.argwhere(cnt != 1)[:5])
    sp = TR.grouped_split(shapes, TR.kt_of(kind), n_cu)
    assert sp["grid"] <= max(n_cu, -(-sp["units"] // 4)) and all(nk > 0 for *_, nk in sp["segments"])


@pytest.mark.parametrize("kind", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(TR.GROUPED))
def test_grouped_cases_reach_their_regime_on_256_cus(name, kind):
    ok, txt = TR.grouped_regime(name, kind, 256)
    print(txt)
    assert ok, txt


def test_tn_cases_sit_on_both_sides_of_the_stage_choice():
    for kind in ("bf16", "f32"):
        deep = [TR.tn_deep(*sh, TR.kt_of(kind), s, 256) for sh, s in TR.tn_cases(kind)]
        print(kind, [(sh, s, "four-stage" if d else "two-stage") for (sh, s), d in zip(TR.tn_cases(kind), deep)])
        assert any(deep) and not all(deep)
