"""The sampler's per-step kernels (csrc/ops.hip: tcdiff_sampler_update, tcdiff_sampler_constrain, tcdiff_window_couple_step; and
tcdiff_add_rows) against tests/sampler_ref.py (MI355X only).  Everything is launched through tcdiff_amd.kernels; the reference only checks.

  * the in-kernel Philox4x32-10 + Box-Muller normals against the reference's, element by element, to 8 x what a float32 numpy
    evaluation of the same expression loses against float64 on the same counters (sampler_ref.normals_bound) -- a wrong bit anywhere in
    the generator or its keying moves a normal by order 1;
  * the update and the kind-2 constraint on injected noise, every form the engine can launch, element by element to
    (r + 1) 2^-24 S: r the fp32 roundings on the expression's longest path, S the sum of the absolute values of the terms it adds
    (both from the reference, counted at its expressions);
  * copies (kind 1, the trajectory channels, the window coupling, disabled steps, add_rows) bit for bit; nothing written outside the
    addressed block; refused arguments leave the outputs alone.

Shapes (sampler_ref): nfeat 151 / 5 / 4 / 1, three clips of 6 rows (684 threads at nfeat 151: a ragged third block), output rows of
nfeat, 152 and 160 elements, three different rows of step scalars and timesteps with counter[0] = 0 or 2."""
import numpy as np
import pytest
import torch

import sampler_ref as SR

pytestmark = pytest.mark.gpu

from tcdiff_amd import _lib as L  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402

DEV = "cuda"
ROWS, LS, CLIPS = SR.ROWS, SR.L_SEQ, SR.CLIPS
F64 = np.float64
SENT = 7.0                                  # sentinel of the rows past an output
CSENT = (77, 91, 92, 93, 94)                # counter[3..7] before a launch
WORST = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def padded(a):
    """a [rows][n] fp32 array on the device with one sentinel row behind it"""
    t = torch.full((a.shape[0] + 1, a.shape[1]), SENT, device=DEV)
    t[:-1] = dev(a)
    return t


def host(t):
    """the device buffer's rows, after checking that the row behind them still holds the sentinel"""
    h = t.cpu().numpy()
    assert (h[-1] == SENT).all(), "wrote past its rows"
    return h[:-1]


def counter_of(step, words=(0, 0)):
    return torch.tensor([step, words[0], words[1]] + list(CSENT), dtype=torch.int32, device=DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def note(key, got, ref, bound):
    """max |got - ref| / bound over the elements (bound > 0), recorded per check for the report"""
    d = np.abs(got.astype(F64) - ref)
    m = bound > 0
    ratio = float((d[m] / bound[m]).max()) if m.any() else 0.0
    w = WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], float(d.max())), max(w[1], ratio)
    return d


TSEQ_T = None


def tseq():
    global TSEQ_T
    if TSEQ_T is None:
        TSEQ_T = torch.tensor(SR.TSEQ, dtype=torch.int32, device=DEV)
    return TSEQ_T


# ---- Philox normals ----------------------------------------------------------------------------------------------------------------
def step_noise(nfeat, step, clip0, seed, words, rows=ROWS, ldo=152):
    """the kernel's step noise: DDPM with params (., 0, 0, 1) on x = 0"""
    x = padded(np.zeros((rows, nfeat), np.float32))
    out = torch.zeros(rows, ldo, device=DEV)
    K.sampler_update(L.SAMPLER_DDPM, None, out, ldo, x, None, None, None, rows, nfeat, LS, counter_of(step, words),
                     dev(SR.noise_params()), tseq(), seed=seed, clip0=clip0)
    return host(x)


def constraint_noise(nfeat, step, clip0, seed, words, rows=ROWS):
    """the kernel's constraint noise: kind 2 without q_eps, mask 1, value 0, params[5] = 1"""
    x = padded(np.zeros((rows, nfeat), np.float32))
    K.sampler_constrain(2, x, torch.ones(rows, nfeat, device=DEV), rows, torch.zeros(rows, nfeat, device=DEV), None, rows, nfeat, LS,
                        counter_of(step, words), dev(SR.noise_params()), tseq(), seed=seed, clip0=clip0)
    return host(x)


@pytest.mark.parametrize("nfeat", SR.NFEATS)
def test_philox_normals_are_the_references(nfeat):
    floor, top, n = SR.normals_floor()
    zb = SR.normals_bound()
    ref = SR.Ref()
    worst = 0.0
    for c in [c for c in SR.philox_cases() if c["nfeat"] == nfeat]:
        noise = SR.noise_of(c)
        zs = step_noise(nfeat, c["step"], c["clip0"], c["seed"], c["dev"])
        zc = constraint_noise(nfeat, c["step"], c["clip0"], c["seed"], c["dev"])
        ds = note(("normals", "step"), zs, ref.normals((ROWS, nfeat), noise, False), np.full(zs.shape, zb))
        dc = note(("normals", "constraint"), zc, ref.normals((ROWS, nfeat), noise, True), np.full(zc.shape, zb))
        worst = max(worst, float(ds.max()), float(dc.max()))
        assert ds.max() <= zb, ("step noise", c, float(ds.max()), zb)
        assert dc.max() <= zb, ("constraint noise (stream word 1)", c, float(dc.max()), zb)
        assert not np.isclose(zs, zc, atol=1e-3).all(axis=None) and np.abs(zs - zc).max() > 0.1, "the constraint reuses the step's stream"
    print(f"philox normals nfeat={nfeat}: floor {floor:.2e} ({n} draws, max|z| {top:.2f}), bound {zb:.2e}, observed max {worst:.2e}")


def test_seed_words_and_clip_partition_bit_for_bit():
    nfeat, s = 151, SR.SEED
    lo, hi = s & 0xFFFFFFFF, s >> 32
    as_i32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v        # noqa: E731
    # seed s with zero device words == seed 0 with the device words carrying s
    a = step_noise(nfeat, 0, 3, s, (0, 0))
    b = step_noise(nfeat, 0, 3, 0, (as_i32(lo), as_i32(hi)))
    assert same_bits(a, b)
    assert same_bits(constraint_noise(nfeat, 2, 3, s, (0, 0)), constraint_noise(nfeat, 2, 3, 0, (as_i32(lo), as_i32(hi))))
    assert not same_bits(a, step_noise(nfeat, 0, 3, s ^ (1 << 32), (0, 0))) and not same_bits(a, step_noise(nfeat, 0, 3, s ^ 1, (0, 0)))
    # clip k alone at clip0 = k == clip k inside the batch
    for nf in SR.NFEATS:
        whole = step_noise(nf, 2, 10, s, SR.DEV_WORDS)
        wc = constraint_noise(nf, 2, 10, s, SR.DEV_WORDS)
        for k in range(CLIPS):
            assert same_bits(step_noise(nf, 2, 10 + k, s, SR.DEV_WORDS, rows=LS), whole[k * LS:(k + 1) * LS]), (nf, k)
            assert same_bits(constraint_noise(nf, 2, 10 + k, s, SR.DEV_WORDS, rows=LS), wc[k * LS:(k + 1) * LS]), (nf, k)
        # no two clips and no two tokens of a clip share normals
        if nf >= 4:
            rows = whole.reshape(ROWS, -1)[:, :4]
            assert len({r.tobytes() for r in rows}) == ROWS


# ---- the update on injected noise ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfeat", SR.NFEATS)
def test_update_every_launch_form(nfeat):
    ref = SR.Ref()
    for ldo in SR.ldos(nfeat):
        c = SR.cases(nfeat, ldo)
        unc_d, cond_d, eps_d, traj_d = dev(c["unc"]), dev(c["cond"]), dev(c["eps"]), dev(c["traj"])
        for case in SR.update_cases():
            mode, step = case["mode"], case["step"]
            p = SR.params(case["flags"], step, case["last"])
            unc = c["unc"] if case["with_unc"] else None
            want = ref.update(mode, unc, c["cond"], c["x"], p[step], eps=c["eps"])
            # with x0_out, advancing at step 2
            advance = L.SAMPLER_ADVANCE if step == 2 else 0
            x, x0, cnt = padded(c["x"]), padded(np.zeros_like(c["x"])), counter_of(step)
            K.sampler_update(mode | advance, unc_d if case["with_unc"] else None, cond_d, ldo, x, eps_d, None, x0, ROWS, nfeat, LS, cnt,
                             dev(p), tseq())
            got, got0 = host(x), host(x0)
            key = ("update", "ddpm" if mode == SR.DDPM else "ddim")
            d = note(key, got, want["x"], want["bound"])
            d0 = note(("update", "x0_out"), got0, want["x0"], want["bound_x0"])
            assert (d <= want["bound"]).all(), (case, ldo, float((d - want["bound"]).max()), want["r"])
            assert (d0 <= want["bound_x0"]).all(), (case, ldo, float((d0 - want["bound_x0"]).max()), want["r_x0"])
            # without SAMPLER_ADVANCE the whole counter is untouched; with it counter[3] = counter[0] + 1 and nothing else changes
            cn = cnt.cpu().tolist()
            assert cn == [step, 0, 0] + ([step + 1] if advance else [CSENT[0]]) + list(CSENT[1:]), (case, cn)
            if case["flags"] & 8 == 0:
                assert np.abs(got0).max() <= 1.0, "x0 not clamped"
                if not (mode == SR.DDPM and case["flags"] & 4):
                    g = want["x0"]                                  # the guided output was exactly +-1 (or beyond) where the inputs are
                    assert (got0[g == 1.0] == 1.0).all() and (got0[g == -1.0] == -1.0).all() and (g == 1.0).sum() >= 3
            # with the trajectory and without x0_out: channels 4 and 5 hold traj bit for bit, everything else is the run above
            xt = padded(c["x"])
            K.sampler_update(mode, unc_d if case["with_unc"] else None, cond_d, ldo, xt, eps_d, traj_d, None, ROWS, nfeat, LS,
                             counter_of(step), dev(p), tseq())
            gt = host(xt)
            keep = np.ones(nfeat, bool)
            keep[4:6] = False
            assert same_bits(gt[:, keep], got[:, keep]), (case, ldo)
            assert same_bits(gt[:, 4:6], c["traj"][:, :max(0, min(nfeat, 6) - 4)]), (case, ldo)
            if case["last"]:
                assert same_bits(gt[:, keep], got0[:, keep])        # DDIM's last step returns x0 itself


# ---- the constraints ---------------------------------------------------------------------------------------------------------------
def cparams(step, on_selected, on_others):
    p = SR.params(0, step)
    p[:, 7] = 2.0 * on_others + 1.0                                 # bit 0 (the coupling's) is not the constraint's business
    p[step, 7] = 2.0 * on_selected + (4.0 if step == 2 else 0.0)
    return p


@pytest.mark.parametrize("nfeat", SR.NFEATS)
def test_constrain_kind1_bit_exact_and_gated(nfeat):
    c = SR.cases(nfeat)
    ref = SR.Ref()
    val = dev(c["value"])
    for step in (0, 2):
        for mask, mask_rows in ((c["mask"], ROWS), (c["mask_L"], LS)):
            p = cparams(step, True, False)
            x = padded(c["x"])
            K.sampler_constrain(1, x, dev(mask), mask_rows, val, None, ROWS, nfeat, LS, counter_of(step), dev(p), tseq())
            got = host(x)
            assert same_bits(got, ref.constrain(1, c["x"], mask, c["value"], p[step])["x"]), (step, mask_rows)
            assert not same_bits(got, c["x"])
            # bit 1 set in the other rows only: nothing happens
            for kind, qe in ((1, None), (2, dev(c["q_eps"])), (2, None)):
                x = padded(c["x"])
                K.sampler_constrain(kind, x, dev(mask), mask_rows, val, qe, ROWS, nfeat, LS, counter_of(step),
                                    dev(cparams(step, False, True)), tseq())
                assert same_bits(host(x), c["x"]), (kind, step, mask_rows)


@pytest.mark.parametrize("nfeat", SR.NFEATS)
def test_constrain_kind2_injected_noise(nfeat):
    c = SR.cases(nfeat)
    ref = SR.Ref()
    val, qe = dev(c["value"]), dev(c["q_eps"])
    for step in (0, 2):
        for mask, mask_rows in ((c["mask"], ROWS), (c["mask_L"], LS)):
            p = cparams(step, True, False)
            cnt = counter_of(step)
            x = padded(c["x"])
            K.sampler_constrain(2, x, dev(mask), mask_rows, val, qe, ROWS, nfeat, LS, cnt, dev(p), tseq())
            got = host(x)
            want = ref.constrain(2, c["x"], mask, c["value"], p[step], q_eps=c["q_eps"])
            d = note(("constrain", "kind2"), got, want["x"], want["bound"])
            assert (d <= want["bound"]).all(), (step, mask_rows, float((d - want["bound"]).max()))
            m = np.asarray(mask)[np.arange(ROWS) % mask_rows]
            assert same_bits(got[m == 0], c["x"][m == 0]) and (m == 0).any() and (m == 1).any() and (m == 0.25).any()
            assert cnt.cpu().tolist() == [step, 0, 0] + list(CSENT)


# ---- the window coupling -------------------------------------------------------------------------------------------------------------
def test_window_couple_step():
    b, S, re_ = 3, 6, 151                                            # 2 x 453 = 906 moved elements: a ragged last block
    g = np.random.default_rng(5)
    x0 = g.standard_normal((b * S, re_)).astype(np.float32)
    ref = SR.Ref()
    for step in (0, 2):
        p = SR.params(0, step)
        p[:, 7] = 2.0                                                # the others: bit 0 clear
        p[step, 7] = 1.0 + (6.0 if step == 2 else 0.0)
        cnt = counter_of(step)
        x = padded(x0)
        K.window_couple_step(x, b, S, re_, cnt, dev(p))
        got = host(x)
        assert same_bits(got, ref.couple(x0, b, S, p[step]))
        v, o = got.reshape(b, S, re_), x0.reshape(b, S, re_)
        assert same_bits(v[1:, :S // 2], o[:-1, S // 2:]) and same_bits(v[:, S // 2:], o[:, S // 2:]) and same_bits(v[0], o[0])
        assert same_bits(v[2, :S // 2], o[1, S // 2:])              # clip 1's ORIGINAL second half, not what clip 1 received
        y = padded(x0)
        K.window_couple(y, b, S, re_)
        assert same_bits(host(y), got)
        assert cnt.cpu().tolist() == [step, 0, 0] + list(CSENT)
        # bit 0 clear in the selected row (set in the others): untouched
        q = p.copy()
        q[:, 7] = 1.0
        q[step, 7] = 14.0
        x = padded(x0)
        K.window_couple_step(x, b, S, re_, counter_of(step), dev(q))
        assert same_bits(host(x), x0)
    x = padded(x0)
    K.window_couple_step(x, 1, b * S, re_, counter_of(2), dev(p))   # one clip (bit 0 set in row 2): nothing to couple
    assert same_bits(host(x), x0)
    with pytest.raises(L.TcdiffError):
        K.window_couple_step(x, b, 5, re_, counter_of(0), dev(p))   # an odd seq_len has no halves
    assert same_bits(host(x), x0)


# ---- three steps in the engine's order -----------------------------------------------------------------------------------------------
def test_three_steps_update_constraint_coupling_step_end():
    """DDPM with both branches, the kernel's own Philox noise in the update and in the kind-2 constraint, then the coupling and
    step_end; each launch's reference starts from the kernel's own previous fp32 state, so the per-launch bound does not compound"""
    nfeat, ldo, clip0 = 151, 152, 2 ** 20 + 3
    c = SR.cases(nfeat, ldo)
    ref = SR.Ref()
    zb = SR.normals_bound()
    p = SR.params(0, 0)
    p[:, 7] = (3.0, 2.0, 1.0)                                        # couple + constrain, constrain only, couple only
    cp = SR.params(0, 0)[:, ::-1].copy()                             # the constraint's own table: other q_sample scalars
    cp[:, 7] = p[:, 7]
    unc_d, cond_d, mask_d, val_d, p_d, cp_d = dev(c["unc"]), dev(c["cond"]), dev(c["mask_L"]), dev(c["value"]), dev(p), dev(cp)

    def run(check):
        cnt = counter_of(0, SR.DEV_WORDS)
        x = padded(c["x"])
        for step in range(3):
            noise = dict(L=LS, t=SR.TSEQ[step], seed=SR.SEED, dev=SR.DEV_WORDS, clip0=clip0)
            prev = host(x).copy() if check else None
            K.sampler_update(L.SAMPLER_DDPM, unc_d, cond_d, ldo, x, None, None, None, ROWS, nfeat, LS, cnt, p_d, tseq(),
                             seed=SR.SEED, clip0=clip0)
            if check:
                got = host(x).copy()
                w = ref.update(SR.DDPM, c["unc"], c["cond"], prev, p[step], noise=noise)
                bound = w["bound"] + w["noise_coef"] * zb
                d = note(("three steps", "update"), got, w["x"], bound)
                assert (d <= bound).all(), (step, float((d - bound).max()))
                prev = got
            K.sampler_constrain(2, x, mask_d, LS, val_d, None, ROWS, nfeat, LS, cnt, cp_d, tseq(), seed=SR.SEED, clip0=clip0)
            if check:
                got = host(x).copy()
                w = ref.constrain(2, prev, c["mask_L"], c["value"], cp[step], noise=noise)
                bound = w["bound"] + w["noise_coef"] * zb
                d = note(("three steps", "constrain"), got, w["x"], bound)
                assert (d <= bound).all(), (step, float((d - bound).max()))
                if step == 2:
                    assert same_bits(got, prev)                       # bit 1 clear
                prev = got
            K.window_couple_step(x, CLIPS, LS, nfeat, cnt, p_d)
            if check:
                assert same_bits(host(x), ref.couple(prev, CLIPS, LS, p[step])), step
                assert same_bits(host(x), prev) == (step == 1)
            K.step_end(cnt)
            assert not check or cnt.cpu().tolist() == [step + 1, SR.DEV_WORDS[0], SR.DEV_WORDS[1]] + list(CSENT)
        return host(x)

    checked = run(True)
    assert same_bits(run(False), checked)                             # the same launches back to back, no host read between them


# ---- refused arguments ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    nfeat = 5
    c = SR.cases(nfeat, 8)
    x, x0, cnt = padded(c["x"]), padded(np.zeros_like(c["x"])), counter_of(0)
    cond, eps, p = dev(c["cond"]), dev(c["eps"]), dev(SR.params(0, 0))
    mask, val = dev(c["mask"]), dev(c["value"])
    with pytest.raises(L.TcdiffError):                               # ldo < nfeat
        K.sampler_update(L.SAMPLER_DDPM, None, cond, nfeat - 1, x, eps, None, x0, ROWS, nfeat, LS, cnt, p, tseq())
    for mode in (2, 7, 2 | L.SAMPLER_ADVANCE, -1):                   # an unknown mode
        with pytest.raises(L.TcdiffError):
            K.sampler_update(mode, None, cond, 8, x, eps, None, x0, ROWS, nfeat, LS, cnt, p, tseq())
    for kind in (3, 0):
        with pytest.raises(L.TcdiffError):
            K.sampler_constrain(kind, x, mask, ROWS, val, None, ROWS, nfeat, LS, cnt, p, tseq())
    with pytest.raises(L.TcdiffError):                               # mask_rows = 0
        K.sampler_constrain(1, x, mask, 0, val, None, ROWS, nfeat, LS, cnt, p, tseq())
    torch.cuda.synchronize()
    assert same_bits(host(x), c["x"]) and (host(x0) == 0).all() and cnt.cpu().tolist() == [0, 0, 0] + list(CSENT)


# ---- add_rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [512, 151])
def test_add_rows_in_place_with_unequal_leading_dimensions(cols):
    rows, ld_a, ld_b = 5, 1536, 512
    g = np.random.default_rng(cols)
    a0 = g.standard_normal((rows, ld_a)).astype(np.float32)
    b0 = g.standard_normal((rows, ld_b)).astype(np.float32)
    a, b = padded(a0), dev(b0)
    K.add_rows(a, ld_a, b, ld_b, a, ld_a, rows, cols)                # out aliases a
    got = host(a)
    assert same_bits(got[:, :cols], a0[:, :cols] + b0[:, :cols])    # one fp32 addition: the same rounding on the host
    assert same_bits(got[:, cols:], a0[:, cols:]) and same_bits(b.cpu().numpy(), b0)
    out = padded(np.zeros((rows, cols), np.float32))                 # and into a dense third buffer
    K.add_rows(a, ld_a, b, ld_b, out, cols, rows, cols)
    assert same_bits(host(out), got[:, :cols] + b0[:, :cols])
    for lds in ((cols - 1, ld_b, ld_a), (ld_a, cols - 1, ld_a), (ld_a, ld_b, cols - 1)):
        with pytest.raises(L.TcdiffError):
            K.add_rows(a, lds[0], b, lds[1], a, lds[2], rows, cols)
    assert same_bits(host(a), got)


def test_zz_report_worst():
    """the largest |kernel - reference| and its ratio to the bound, per check, over this module's run"""
    floor, top, n = SR.normals_floor()
    print(f"WORST normals floor {floor:.2e} ({n} draws, max|z| {top:.2f}) bound {SR.normals_bound():.2e}")
    for key, (mx, ratio) in sorted(WORST.items()):
        print(f"WORST {key[0]:12s} {key[1]:10s} max|d|={mx:.2e} max d/bound={ratio:.3f}")
