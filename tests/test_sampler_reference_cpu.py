"""tests/sampler_ref.py -- the numpy reference the sampler's per-step kernels are held to on the GPU
(tests/test_sampler_kernels_f64_gpu.py) -- pinned before any GPU run: its Philox4x32-10 gives the Random123 known answers, its normals
have the moments of N(0, 1), its DDPM update and its kind-2 constraint are the oracle's arithmetic in float64, and each emulated kernel
defect moves some element of the GPU test's own inputs by at least 100 times that element's GPU bound."""
import numpy as np
import pytest
import torch

import sampler_ref as SR
from oracle import tcdiff_oracle as O

F64 = np.float64


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


# ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """the Random123 known-answer vectors of philox4x32 with 10 rounds"""
    assert _hex(philox_words(counter, key)) == want


def philox_words(counter, key):
    return [int(w) for w in SR.philox4x32_10(counter, key)]


def _philox_scalar(counter, key):
    """the same generator once more with Python integers, one counter at a time (nothing shared with the vectorised one)"""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_philox_vectorised_equals_scalar_and_other_round_counts_differ():
    g = np.random.default_rng(0)
    cs = g.integers(0, 2 ** 32, (64, 4), dtype=np.uint64)
    ks = g.integers(0, 2 ** 32, (64, 2), dtype=np.uint64)
    got = np.stack(SR.philox4x32_10(tuple(cs[:, i] for i in range(4)), tuple(ks[:, i] for i in range(2))), axis=1)
    for i in range(64):
        assert got[i].tolist() == _philox_scalar([int(v) for v in cs[i]], [int(v) for v in ks[i]])
    assert philox_words((0, 0, 0, 0), (0, 0)) != [int(w) for w in SR.philox4x32_10((0, 0, 0, 0), (0, 0), rounds=9)]


def test_philox_normals_keying():
    """counter = (tok * quads + quad, t, clip0 + row // L, stream), key = (seed_lo ^ dev0, seed_hi ^ dev1), one quad -> four normals"""
    nfeat, L, t, seed, dev, clip0 = 7, 3, 999, SR.SEED, SR.DEV_WORDS, 2 ** 20 + 3
    z = SR.philox_normals(7, nfeat, L, t, seed, dev, clip0, stream=1)
    k = ((seed & 0xFFFFFFFF) ^ (dev[0] & 0xFFFFFFFF), (seed >> 32) ^ (dev[1] & 0xFFFFFFFF))
    for row, col in ((0, 0), (2, 6), (3, 1), (6, 4), (5, 3)):
        w = _philox_scalar([(row % L) * 2 + col // 4, t, clip0 + row // L, 1], list(k))
        want = SR.normals_of_words([np.array([v], np.uint32) for v in w])[col % 4][0]
        assert z[row, col] == want
    # the seed only enters through the XOR with the device words; a negative int32 word is its two's complement
    assert np.array_equal(z, SR.philox_normals(7, nfeat, L, t, 0, (k[0], k[1] - 2 ** 32), clip0, stream=1))


# ---- the normals -----------------------------------------------------------------------------------------------------------------------
def test_normals_have_the_moments_of_the_standard_normal():
    rows, nfeat = 1325, 151                                        # 200 075 draws
    z = SR.philox_normals(rows, nfeat, 25, 417, seed=SR.SEED, dev=SR.DEV_WORDS, clip0=11).ravel()
    n = z.size
    assert n >= 200000
    # standard errors of the sample mean, second and fourth moment of N(0, 1): sqrt(1 / n), sqrt(2 / n), sqrt((105 - 9) / n)
    m1, m2, m4 = z.mean(), (z ** 2).mean(), (z ** 4).mean()
    print(f"normals: n={n} mean={m1:+.2e} var={m2:.5f} m4={m4:.4f} max|z|={np.abs(z).max():.2f}")
    assert abs(m1) <= 4 * np.sqrt(1 / n)
    assert abs(m2 - 1) <= 4 * np.sqrt(2 / n)
    assert abs(m4 - 3) <= 4 * np.sqrt(96 / n)


def test_stream_words_give_different_normals():
    a = SR.philox_normals(18, 151, 6, 999, seed=5, stream=0)
    b = SR.philox_normals(18, 151, 6, 999, seed=5, stream=1)
    assert not np.isclose(a, b, atol=1e-3).any()
    assert abs(np.corrcoef(a.ravel(), b.ravel())[0, 1]) < 4 / np.sqrt(a.size)


def test_u01_edges():
    """u is the kernel's float32 value: never 0, exactly 1.0 at the top (the sum rounds from 2^23 on), and u = 1 gives a finite normal"""
    w = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0x800001FF, 0xFFFFFE00, 0xFFFFFFFF], np.uint32)
    u = SR.u01(w)
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -25) and u[1] == u[0] and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32(8388607.5 * 2.0 ** -24)               # 2^23 - 1 + 0.5: still exact
    assert u[4] == np.float32(0.5)                                  # 2^23 + 0.5: a tie, to even (down)
    assert u[5] == np.float32((2 ** 23 + 2) * 2.0 ** -24)           # 2^23 + 1 + 0.5: a tie, to even (up)
    assert u[6] == np.float32((2 ** 24 - 2) * 2.0 ** -24) and u[7] == np.float32(1.0)
    assert (u > 0).all() and (u <= 1).all()
    top = np.array([0xFFFFFFFF], np.uint32)
    for dt in (np.float64, np.float32):
        z = SR.normals_of_words([top, top, top, top], dt)
        assert all(np.isfinite(v).all() for v in z) and float(z[0][0]) == 0.0


def test_normals_floor_is_what_the_design_records():
    floor, top, n = SR.normals_floor()
    print(f"normals floor (float32 numpy vs float64, the GPU test's counters): {floor:.2e} over {n} draws, max|z| = {top:.2f}; "
          f"GPU bound = {SR.normals_bound():.2e}")
    assert 5e-8 < floor < 2e-6 and top > 3.5


# ---- the update formulas against the oracle ---------------------------------------------------------------------------------------------
def _tab64():
    return {k: v.to(torch.float64) for k, v in O.make_tables(1000).items()}


@pytest.mark.parametrize("i", [0, 1, 50, 500, 999])
def test_ddpm_update_is_the_oracles_p_sample(monkeypatch, i):
    c = SR.cases(151)
    tab = _tab64()
    unc, cond, x, eps = (torch.from_numpy(c[k]).double() for k in ("unc", "cond", "x", "eps"))
    w = O.ddpm_guidance_weight(i, 1000, 2.0)
    monkeypatch.setattr(O, "guided_forward", lambda sd, x_, cond_, t, w_: unc + (cond - unc) * w_)
    want, want_x0 = O.p_sample(None, tab, x, None, i, 1000, 2.0, eps)
    sigma = 0.0 if i == 0 else float((0.5 * tab["posterior_log_variance_clipped"][i]).exp())
    pr = [w, float(tab["posterior_mean_coef1"][i]), float(tab["posterior_mean_coef2"][i]), sigma, 0, 0, 0, 0]
    got = SR.Ref().update(SR.DDPM, c["unc"], c["cond"], c["x"], pr, eps=c["eps"])
    assert np.abs(got["x"] - want.numpy()).max() <= 1e-12 and np.abs(got["x0"] - want_x0.numpy()).max() <= 1e-12
    assert got["r"] == 6 and (got["S"] >= np.abs(got["x"]) - 1e-12).all()


def test_predict_epsilon_ddim_and_trajectory_forms():
    """the remaining forms, restated here in one line each from the same reference lines"""
    c = SR.cases(151)
    unc, cond, x, eps, traj = (c[k].astype(F64) for k in ("unc", "cond", "x", "eps", "traj"))
    pr = SR.params(4, 1).astype(F64)[1]
    g = unc + (cond - unc) * pr[0]
    got = SR.Ref().update(SR.DDPM, c["unc"], c["cond"], c["x"], pr, eps=c["eps"])
    x0 = np.clip(pr[4] * x - pr[5] * g, -1, 1)
    assert np.abs(got["x"] - (pr[1] * x0 + pr[2] * x + pr[3] * eps)).max() <= 1e-12 and got["r"] == 8
    # DDIM takes the output as x_0 whatever bit 2 says; bit 3: no clamp
    pr = SR.params(12, 1).astype(F64)[1]
    got = SR.Ref().update(SR.DDIM, None, c["cond"], c["x"], pr, eps=c["eps"], traj=c["traj"])
    pn = (pr[1] * x - cond) / pr[2]
    want = cond * pr[3] + pr[4] * pn + pr[5] * eps
    want[:, 4:6] = traj[:, :2]
    assert np.abs(got["x"] - want).max() <= 1e-12 and got["r"] == 5 and (got["bound"][:, 4:6] == 0).all()
    assert np.array_equal(got["x"][:, 4:6], traj[:, :2]) and np.array_equal(got["x0"], cond)
    last = SR.Ref().update(SR.DDIM, None, c["cond"], c["x"], SR.params(0, 1, last=True)[1], eps=c["eps"])
    assert np.array_equal(last["x"], np.clip(cond, -1, 1)) and last["r"] == 0
    # a 5-wide row has channel 4 only, narrower rows no trajectory channel
    for nf, cols in ((5, 1), (4, 0), (1, 0)):
        cn = SR.cases(nf)
        a = SR.Ref().update(SR.DDIM, None, cn["cond"], cn["x"], pr, eps=cn["eps"], traj=cn["traj"])
        b = SR.Ref().update(SR.DDIM, None, cn["cond"], cn["x"], pr, eps=cn["eps"])
        assert np.array_equal(a["x"][:, :4], b["x"][:, :4])
        if cols:
            assert np.array_equal(a["x"][:, 4], cn["traj"][:, 0].astype(F64))


@pytest.mark.parametrize("t", [1, 40, 999])
def test_kind2_constraint_is_the_oracles_q_sample_mixed_by_the_mask(t):
    c = SR.cases(151)
    tab = _tab64()
    value, noise, x, mask = (torch.from_numpy(c[k]).double() for k in ("value", "q_eps", "x", "mask"))
    v3 = value.reshape(SR.CLIPS, SR.L_SEQ, 151)
    qs = O.q_sample(tab, v3, torch.full((SR.CLIPS,), t - 1), noise.reshape(v3.shape)).reshape(value.shape)
    want = qs * mask + (1.0 - mask) * x                            # oracle.inpaint_loop
    pr = [0, 0, 0, 0, float(tab["sqrt_alphas_cumprod"][t - 1]), float(tab["sqrt_one_minus_alphas_cumprod"][t - 1]), 0, 2]
    got = SR.Ref().constrain(2, c["x"], c["mask"], c["value"], pr, q_eps=c["q_eps"])
    assert np.abs(got["x"] - want.numpy()).max() <= 1e-12
    # the [L][nfeat] mask serves every clip; a step without bit 1 leaves x alone
    gl = SR.Ref().constrain(2, c["x"], c["mask_L"], c["value"], pr, q_eps=c["q_eps"])
    ml = mask[SR.L_SEQ:2 * SR.L_SEQ].repeat(SR.CLIPS, 1)
    assert np.abs(gl["x"] - (qs * ml + (1.0 - ml) * x).numpy()).max() <= 1e-12
    pr[7] = 5
    assert np.array_equal(SR.Ref().constrain(2, c["x"], c["mask"], c["value"], pr, q_eps=c["q_eps"])["x"], c["x"].astype(F64))


def test_kind1_and_coupling():
    c = SR.cases(5)
    pr = [0] * 7 + [2]
    got = SR.Ref().constrain(1, c["x"], c["mask"], c["value"], pr)["x"]
    assert np.array_equal(got, np.where(c["mask"] != 0, c["value"], c["x"]).astype(F64))
    x = np.arange(3 * 6 * 5, dtype=np.float32).reshape(18, 5)
    out = SR.Ref().couple(x, 3, 6, [0] * 7 + [1]).reshape(3, 6, 5)
    xv = x.reshape(3, 6, 5)
    assert np.array_equal(out[1:, :3], xv[:-1, 3:]) and np.array_equal(out[:, 3:], xv[:, 3:]) and np.array_equal(out[0], xv[0])
    assert np.array_equal(SR.Ref().couple(x, 3, 6, [0] * 7 + [2]), x) and np.array_equal(SR.Ref().couple(x, 1, 18, [0] * 7 + [1]), x)


# ---- teeth: every emulated defect exceeds the GPU bound 100 times on the GPU test's inputs ----------------------------------------------
def _update_ratio(mutant, nfeat, case):
    c = SR.cases(nfeat)
    pr = SR.params(case["flags"], case["step"], case["last"])[case["step"]]
    kw = dict(eps=c["eps"])
    unc = c["unc"] if case["with_unc"] else None
    ref = SR.Ref().update(case["mode"], unc, c["cond"], c["x"], pr, **kw)
    mut = mutant().update(case["mode"], unc, c["cond"], c["x"], pr, **kw)
    d = np.abs(mut["x"] - ref["x"])
    return float((d[ref["bound"] > 0] / ref["bound"][ref["bound"] > 0]).max())


@pytest.mark.parametrize("nfeat", SR.NFEATS)
@pytest.mark.parametrize("name,relevant", [
    ("swap_params_1_2", lambda k: not k["last"]),
    ("no_clamp", lambda k: not k["flags"] & 8),
    ("ignore_bit2", lambda k: k["mode"] == SR.DDPM and k["flags"] & 4),
])
def test_arithmetic_mutants_exceed_the_bound_100_times(name, relevant, nfeat):
    worst = {}
    for case in SR.update_cases():
        ratio = _update_ratio(SR.MUTANTS[name], nfeat, case)
        if relevant(case):
            worst[tuple(case.values())] = ratio
        else:
            assert ratio == 0.0, (name, case, ratio)                  # the mutation is not reachable there
    print(f"{name} nfeat={nfeat}: smallest max |mutant - reference| / bound over {len(worst)} cases = {min(worst.values()):.3g}")
    assert worst and min(worst.values()) >= 100.0, (name, nfeat, min(worst, key=worst.get), min(worst.values()))


@pytest.mark.parametrize("name", ["constraint_stream0", "keyed_by_row"])
def test_keying_mutants_exceed_the_normals_bound_100_times(name):
    zb = SR.normals_bound()
    pr = SR.noise_params()
    smallest = np.inf
    for case in SR.philox_cases():
        nf, noise, row = case["nfeat"], SR.noise_of(case), pr[case["step"]]
        zero, one = np.zeros((SR.ROWS, nf), np.float32), np.ones((SR.ROWS, nf), np.float32)
        for M in (SR.Ref, SR.MUTANTS[name]):
            # what the GPU test launches: x = 0, params (., 0, 0, 1): the update's output is its noise; kind 2 with value 0, mask 1,
            # params[5] = 1: the constraint's output is its noise
            step = M().update(SR.DDPM, None, zero, zero, row, noise=noise)["x"]
            con = M().constrain(2, zero, one, zero, row, noise=noise)["x"]
            if M is SR.Ref:
                ref_step, ref_con = step, con
        d = np.abs(con - ref_con).max() if name == "constraint_stream0" else min(np.abs(step - ref_step).max(),
                                                                                 np.abs(con - ref_con).max())
        if name == "constraint_stream0":
            assert np.array_equal(step, ref_step) and np.array_equal(con, ref_step)
        smallest = min(smallest, d / zb)
    print(f"{name}: smallest max |mutant - reference| / normals bound over the launches = {smallest:.3g} (bound {zb:.2e})")
    assert smallest >= 100.0
