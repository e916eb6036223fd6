"""A float64 evaluation of the training loss head (reference model/diffusion.py:660-741) -- the reference the HIP kernels of
tcdiff_amd.diffusion._LossFn are held to, kernel by kernel (tests/test_loss_head_f64_gpu.py):

    forward   ax_from_6v -> smpl_fk -> loss_terms -> loss_total
    backward  loss_terms_bwd (d_out: recon + velocity; d_joints: FK + foot-skate) -> fk_bwd (d_joints -> d_out, accumulated)

Written from the loss's definition, not from the kernels: the four terms are vectorised torch expressions in float64, their gradients
are derived by hand here (tests/test_loss_reference_cpu.py pins them to float64 autograd of the same total), and the
ax_from_6v / smpl_fk Jacobian is float64 autograd through the oracle's restatement.  Two things follow the kernels on purpose:

  * the foot mask is `contact > 0.95` on the float32 contacts, compared with float32(0.95): no float32 lies strictly between
    float32(0.95) and 0.95, so this is the kernels' `> 0.95f`;
  * with `f32_signs` (the default) an l1 gradient takes its sign from the difference the kernel forms -- rounded to float32 at each
    subtraction, in the kernel's association order, e.g. (m_s - m_{s-1}) - (t_s - t_{s-1}) -- so that an ordinary near-zero
    difference cannot flip sign between float32 and float64.  Joint differences use `sign_joints` (the kernel's float32 joints)
    when given, else the float32 images of the reference's joints.

`defects` emulates plausible kernel defects in the gradients (the terms are left alone), to show that the GPU bounds catch them."""
import numpy as np
import torch

from oracle import tcdiff_oracle as O

D = torch.float64
COEF = (0.636, 2.964, 0.646, 10.942)
FOOT = list(O.FOOT_IDX)                 # [7, 8, 10, 11]
F95 = np.float32(0.95)
T_STEPS = 100

DEFECTS = (
    "foot_drop",            # the foot-skate gradient is dropped
    "foot_one_side",        # only the outgoing neighbour's (frame s -> s + 1) foot-skate contribution is kept
    "foot_contact_s",       # the incoming foot term reads the contact of frame s instead of s - 1
    "foot_ge",              # the contact threshold is >= 0.95f instead of > 0.95f
    "p2_clip0",             # clip 0's p2 weight is used for every clip
    "p2_foot",              # the p2 weight is applied to the foot term
    "vel_first",            # the first frame gets no velocity gradient
    "vel_last",             # the last frame gets no velocity gradient
    "row_swap",             # dancer and frame of a token row swapped (row = d * S + s)
    "l1_sign0",             # l1 with sign(0) = +1
    "gscale_ignored",       # the incoming gradient scale is not applied
    "fk_root_drop",         # the root-joint (j = 0) term of the FK gradient is dropped
)


def joints(rows):
    """rows (n, C) float64 -> (n, 24, 3) SMPL joint positions: oracle ax_from_6v of channels 7.., smpl_fk with root 4..6"""
    n = rows.shape[0]
    aa = O.ax_from_6v(rows[:, 7:7 + 144].reshape(1, n, 24, 6))
    return O.smpl_fk(aa, rows[:, 4:7].reshape(1, n, 3))[0]


def fk_vjp(rows, cot):
    """the vector-Jacobian product of rows -> joints(rows) for the joint cotangent cot (n, 24, 3): (n, C), channels 0..3 zero"""
    r = rows.detach().to(D).clone().requires_grad_(True)
    (joints(r) * cot.to(D)).sum().backward()
    return r.grad


def _rows_to_tokens(x, S, dn):
    """(b, S, dn, ...) -> (b, S * dn, ...): token row r = s * dn + d"""
    return x.reshape(x.shape[0], S * dn, *x.shape[3:])


def _lf(x, l1):
    return x.abs() if l1 else x * x


def terms_of(mo, tg, wt, l1, mask):
    """the four weighted per-batch means and the total, differentiable in mo: mo (b, S, dn, C) and tg (b, S, dn, C) float64,
    wt (b,) the p2 weights, mask (b, S, dn, 4) the foot contacts"""
    b, S, dn, C = mo.shape
    recon = _lf(mo - tg, l1).reshape(b, -1).mean(1) * wt
    e = (mo[:, 1:, :, 4:] - mo[:, :-1, :, 4:]) - (tg[:, 1:, :, 4:] - tg[:, :-1, :, 4:])
    vel = _lf(e, l1).reshape(b, -1).mean(1) * wt
    jm = joints(mo.reshape(-1, C)).reshape(b, S, dn, 24, 3)
    jt = joints(tg.reshape(-1, C)).reshape(b, S, dn, 24, 3)
    ef = (jm[..., 1:, :] - jm[..., :1, :]) - (jt[..., 1:, :] - jt[..., :1, :])
    fk = _lf(ef, l1).reshape(b, -1).mean(1) * wt
    feet = jm[..., FOOT, :]
    v = (feet[:, 1:] - feet[:, :-1]) * mask[:, :-1, ..., None]
    foot = _lf(v, l1).reshape(b, -1).sum(1) / (S * dn * 12)            # the last frame's zero velocity counts
    terms = torch.stack([COEF[0] * recon.mean(), COEF[1] * vel.mean(), COEF[2] * fk.mean(), COEF[3] * foot.mean()])
    return terms, terms.sum(), jm, jt


def loss_head(model_out, target, t, w, l1, gscale=1.0, *, f32_signs=True, sign_joints=None, defects=(), with_vjp=True):
    """model_out (b, S * dn, C) token layout, target (b, dn, S, C) dataset layout (x_start, or the noise when predict_epsilon),
    t (b,), w the p2 weight table [T], l1, gscale the incoming gradient of the total.  Returns a dict of float64 tensors:
    terms (4,), total, d_out_direct (b, S * dn, C) -- recon + velocity, what loss_terms_bwd writes to d_out --, d_joints
    (b * S * dn, 24, 3) -- FK + foot, what loss_terms_bwd writes to d_joints --, vjp (b, S * dn, C) -- fk_vjp of d_joints -- and
    d_out = d_out_direct + vjp; jm / jt the joints (b * S * dn, 24, 3)."""
    bad = set(defects)
    assert bad <= set(DEFECTS), bad - set(DEFECTS)
    mo32 = model_out.detach().cpu().float()
    tg32 = target.detach().cpu().float()
    b, dn, S, C = tg32.shape
    m32 = mo32.reshape(b, S, dn, C)
    t32 = tg32.permute(0, 2, 1, 3).contiguous()                       # (b, S, dn, C)
    mo, tg = m32.to(D), t32.to(D)
    wt = w.detach().cpu().to(D)[t.detach().cpu().long()]               # (a float32 table, or a float64 one)
    cont = m32[..., :4]
    mask = cont > torch.tensor(F95)
    terms, total, jm, jt = terms_of(mo, tg, wt, l1, mask.to(D))

    def dl(x64, x32):
        """d loss / d x: 2 x (l2) or the sign of the kernel's float32 difference (l1)"""
        if not l1:
            return 2.0 * x64
        s = torch.sign(x32.to(D)) if f32_signs else torch.sign(x64)
        return torch.where(s == 0, torch.ones_like(s), s) if "l1_sign0" in bad else s

    gs = 1.0 if "gscale_ignored" in bad else float(gscale)
    wb = (wt[:1].expand(b) if "p2_clip0" in bad else wt) / b           # (b,)
    col = lambda x, k=4: x.reshape(b, *([1] * (k - 1)))          # (b,) against (b, S, dn, ...) of k dimensions

    # ---- d_out: reconstruction + velocity (channels 4..), in (b, S, dn, C) ----
    g = col(COEF[0] * wb / (S * dn * C)) * dl(mo - tg, m32 - t32)
    e32 = (m32[:, 1:, :, 4:] - m32[:, :-1, :, 4:]) - (t32[:, 1:, :, 4:] - t32[:, :-1, :, 4:])
    e64 = (mo[:, 1:, :, 4:] - mo[:, :-1, :, 4:]) - (tg[:, 1:, :, 4:] - tg[:, :-1, :, 4:])
    kv = col(COEF[1] * wb / ((S - 1) * dn * (C - 4))) * dl(e64, e32)   # pair (s, s + 1), s < S - 1
    inc, out = kv.clone(), kv.clone()                                  # the incoming term of frame s + 1, the outgoing one of s
    if "vel_last" in bad:
        inc[:, -1] = 0
    if "vel_first" in bad:
        out[:, 0] = 0
    g[:, 1:, :, 4:] += inc
    g[:, :-1, :, 4:] -= out

    # ---- d_joints: FK + foot-skate, in (b, S, dn, 24, 3) ----
    if sign_joints is None:
        sjm, sjt = jm.float(), jt.float()
    else:
        sjm, sjt = (x.detach().cpu().float().reshape(b, S, dn, 24, 3) for x in sign_joints)
    ef64 = (jm[..., 1:, :] - jm[..., :1, :]) - (jt[..., 1:, :] - jt[..., :1, :])
    ef32 = (sjm[..., 1:, :] - sjm[..., :1, :]) - (sjt[..., 1:, :] - sjt[..., :1, :])
    df = col(COEF[2] * wb / (S * dn * 69), 5) * dl(ef64, ef32)
    gj = torch.zeros(b, S, dn, 24, 3, dtype=D)
    gj[..., 1:, :] = df
    if "fk_root_drop" not in bad:
        gj[..., 0, :] = -df.sum(-2)
    if "foot_drop" not in bad:
        cfo = COEF[3] / b / (S * dn * 12) * (col(wt, 5) if "p2_foot" in bad else torch.ones(b, 1, 1, 1, 1, dtype=D))
        mk = (cont >= torch.tensor(F95)) if "foot_ge" in bad else mask
        feet = jm[..., FOOT, :]
        dv = cfo * dl(feet[:, 1:] - feet[:, :-1], sjm[..., FOOT, :][:, 1:] - sjm[..., FOOT, :][:, :-1])   # pair (s, s + 1)
        inc = dv * (mk[:, 1:] if "foot_contact_s" in bad else mk[:, :-1])[..., None]
        out = dv * mk[:, :-1, ..., None]
        if "foot_one_side" not in bad:
            gj[:, 1:, :, FOOT] += inc
        gj[:, :-1, :, FOOT] -= out

    g, gj = gs * g, gs * gj
    g, gj = _rows_to_tokens(g, S, dn), _rows_to_tokens(gj, S, dn)
    if "row_swap" in bad:                    # the kernel decodes token row r as s = r % S, d = r // S
        r = torch.arange(S * dn)
        src = (r % S) * dn + r // S
        g, gj = g[:, src], gj[:, src]
    res = dict(terms=terms.detach(), total=total.detach(), d_out_direct=g.contiguous(), d_joints=gj.reshape(-1, 24, 3).contiguous(),
               jm=jm.reshape(-1, 24, 3).detach().contiguous(), jt=jt.reshape(-1, 24, 3).detach().contiguous())
    if with_vjp:
        res["vjp"] = fk_vjp(mo32.reshape(-1, C), res["d_joints"]).reshape(b, S * dn, C)
        res["d_out"] = g + res["vjp"]
    return res


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------
def p2_table(use_p2, T=T_STEPS):
    """the p2 weight table GaussianDiffusion registers (float32): (1 + ac / (1 - ac)) ** -0.5 with use_p2, else all ones"""
    ac = O.make_tables(T)["alphas_cumprod"]
    return ((1 + ac / (1 - ac)) ** -0.5).float() if use_p2 else torch.ones(T)


def timesteps(b, seed, T=T_STEPS):
    """distinct t per clip: 0 and T - 1 first, then a draw without replacement"""
    g = torch.Generator().manual_seed(seed)
    rest = (torch.randperm(T - 2, generator=g) + 1).tolist()
    return torch.tensor(([0, T - 1] + rest)[:b], dtype=torch.long)


def contacts(kind, shape, g):
    """foot contacts: "none" (all <= 0.9), "some" (~20 % above 0.95), "all" (all above), "edge" (float32(0.95) and its two
    float32 neighbours, mixed with the rest)"""
    u = torch.rand(shape, generator=g)
    if kind == "none":
        return u * 0.9
    if kind == "some":
        return u * 1.2
    if kind == "all":
        return 0.951 + 0.04 * u
    f = F95
    vals = torch.tensor([np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(2))], dtype=torch.float32)
    c = u * 1.2
    pick = torch.randint(0, 3, shape, generator=g)
    sel = torch.rand(shape, generator=g) < 0.5
    return torch.where(sel, vals[pick], c)


def make_case(b, dn, S, l1, p2, cont, seed, ties=None):
    """(model_out (b, S * dn, 151) token layout, target (b, dn, S, 151), t, w) float32 on the CPU; the rotation channels uniform in
    [-1, 1] (random rotations).  ties (default: l1): ~5 % of the entries and two consecutive whole frames of clip 0 (one frame when
    S < 4; every dancer, every channel but the contacts) with model_out == target exactly."""
    g = torch.Generator().manual_seed(seed)
    C = 151
    target = torch.rand(b, dn, S, C, generator=g) * 2 - 1
    mo = torch.rand(b, S, dn, C, generator=g) * 2 - 1
    tgt = target.permute(0, 2, 1, 3)
    if l1 if ties is None else ties:
        eq = torch.rand(b, S, dn, C, generator=g) < 0.05
        mo = torch.where(eq, tgt, mo)
        s0, k = (S // 2 - 1, 2) if S > 3 else (0, 1)                    # (one frame of a 2- or 3-frame clip)
        mo[0, s0:s0 + k] = tgt[0, s0:s0 + k]
    mo[..., :4] = contacts(cont, (b, S, dn, 4), g)
    return mo.reshape(b, S * dn, C).contiguous(), target.contiguous(), timesteps(b, seed), p2_table(p2)


def _rodrigues(axis, ang):
    a = axis / np.linalg.norm(axis)
    K_ = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K_ + (1 - np.cos(ang)) * K_ @ K_


def near_pi_6d(cand, rng):
    """a 6-D rotation within 1e-3 of pi about an axis near e_{cand - 1} (matrix_to_quaternion then selects candidate `cand`), its
    rows scaled and a1 mixed into a2 (Gram-Schmidt removes both)"""
    axis = np.eye(3)[cand - 1] + rng.uniform(-0.2, 0.2, 3)
    R = _rodrigues(axis, np.pi - rng.uniform(1e-4, 9e-4))
    s1, s2, c = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(-0.5, 0.5)
    return np.concatenate([s1 * R[0], s2 * R[1] + c * R[0]])


FK_KINDS = ("near_pi", "random", "identity", "random")          # row kind = i % 4


def fk_rows(n, seed, C=151):
    """(n, C) float32 rows for fk_bwd: channels 4..6 a root, 7.. 24 6-D rotations by row kind (FK_KINDS[i % 4]): near pi
    (candidates 1, 2, 3 in turn), uniform in [-1, 1], exact identity (1, 0, 0, 0, 1, 0: the small-angle branch)"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (n, C))
    for i in range(0, n, 4):
        for j in range(24):
            rows[i, 7 + 6 * j:13 + 6 * j] = near_pi_6d(1 + (i // 4 + j) % 3, rng)
    rows[2::4, 7:151] = np.tile([1.0, 0, 0, 0, 1.0, 0], 24)
    return torch.from_numpy(rows).float()


def degenerate_rows(n, seed, C=151):
    """rows whose 6-D rotations are nearly (or exactly, every other row) degenerate: a2 parallel to a1"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (n, C))
    for i in range(n):
        for j in range(24):
            a1 = rng.uniform(-1, 1, 3)
            eps = 0.0 if i % 2 else 1e-7
            rows[i, 7 + 6 * j:13 + 6 * j] = np.concatenate([a1, rng.uniform(-2, 2) * a1 + eps * rng.uniform(-1, 1, 3)])
    return torch.from_numpy(rows).float()


FK_SEED = 77


def fk_cotangent(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 24, 3, generator=g)


def fk_errors(got, want):
    """fk_bwd regions: rows 7..150 ("rot") and 4..6 ("root"), max-abs error relative to the region's max |want|"""
    got, want = got.detach().cpu().to(D), want.detach().cpu().to(D)
    res = {}
    for name, cs in (("rot", slice(7, 151)), ("root", slice(4, 7))):
        res[name] = float((got[:, cs] - want[:, cs]).abs().max() / want[:, cs].abs().max())
    return res


def case_seed(case):
    """a fixed seed per GPU case (b, dn, S, l1, p2, contacts, gscale): the CPU and GPU tests build the same inputs"""
    b, dn, S, l1, p2, cont, gs = case
    return 1000 * b + 100 * dn + S + 7 * int(l1) + 13 * int(p2) + 17 * "none some all edge".split().index(cont)


def quat_candidate(rows):
    """(n, 24) the matrix_to_quaternion candidate float64 selects for each rotation of rows"""
    m = O.rotation_6d_to_matrix(rows[:, 7:151].to(D).reshape(-1, 24, 6))
    tr = torch.stack([1 + m[..., 0, 0] + m[..., 1, 1] + m[..., 2, 2], 1 + m[..., 0, 0] - m[..., 1, 1] - m[..., 2, 2],
                      1 - m[..., 0, 0] + m[..., 1, 1] - m[..., 2, 2], 1 - m[..., 0, 0] - m[..., 1, 1] + m[..., 2, 2]], -1)
    return tr.argmax(-1)


# ---- regions -------------------------------------------------------------------------------------------------------------
CHANNELS = {"c0-3": slice(0, 4), "c4-5": slice(4, 6), "c6": slice(6, 7), "c7-150": slice(7, 151)}
JOINT_SETS = {"j0": [0], "feet": FOOT, "other": [j for j in range(1, 24) if j not in FOOT]}


def out_regions(S, dn):
    """d_out (b, S * dn, C) regions: channel group x first / last / interior frame -> (row index, channel slice)"""
    frames = {"first": [0], "last": [S - 1], "interior": list(range(1, S - 1))}
    res = {}
    for fn, fr in frames.items():
        rows = [s * dn + d for s in fr for d in range(dn)]
        if rows:
            for cn, cs in CHANNELS.items():
                res[f"{cn}/{fn}"] = (torch.tensor(rows), cs)
    return res


def region_errors(got, ref, regions, kind):
    """{region: (max-abs error / max |ref| of the region, max |ref|)}; `kind` "out" (b, S * dn, C) or "joints" (n, 24, 3)"""
    got, ref = got.detach().cpu().to(D), ref.detach().cpu().to(D)
    res = {}
    for name, sel in regions.items():
        if kind == "out":
            a, r = got[:, sel[0], sel[1]], ref[:, sel[0], sel[1]]
        else:
            a, r = got[:, sel], ref[:, sel]
        den = float(r.abs().max())
        scale = den if den > 0 else float(ref.abs().max())
        res[name] = (float((a - r).abs().max()) / scale, den)
    return res


# the case grid of the GPU tests (a, c, d): (b, dn, S, l1, p2, contacts, gscale) -- every shape, both losses, both weightings, gscale
# 1 and not, each kind of contacts; l1 cases carry exact ties (make_case)
GPU_CASES = [
    (1, 1, 2, False, False, "none", 1.0),
    (1, 1, 2, True, False, "all", 0.37),
    (1, 1, 2, True, True, "edge", 2.5),
    (2, 3, 20, False, True, "some", 1.0),
    (2, 3, 20, False, False, "none", 2.5),
    (2, 3, 20, True, False, "edge", 0.37),
    (2, 3, 20, True, True, "edge", 1.0),
    (3, 2, 61, True, True, "some", 1.0),
    (3, 2, 61, False, False, "all", 0.37),
    (3, 2, 61, False, True, "edge", 2.5),
    (32, 3, 150, False, True, "some", 1.0),
    (32, 3, 150, True, True, "some", 0.37),
]


def case_id(case):
    b, dn, S, l1, p2, cont, gs = case
    return f"{b}x{dn}x{S}-{'l1' if l1 else 'l2'}-{'p2' if p2 else 'w1'}-{cont}-g{gs}"


# Bounds, relative max-abs per region (max |got - ref| / max |ref| over the region).  u = 2^-24 = 6.0e-8.
#  loss_terms_bwd (a): an element of d_out is at most three float32 products of a coefficient (4 roundings each: w / b, times the
#   constant, over the count, times dloss) and two differences of differences (3 roundings, operands up to twice the result's
#   region maximum), summed in 2 roundings: <= ~20 u * 2 = 2.4e-6 of the region maximum.  d_joints: the FK difference of differences
#   of float32 joints (|j| <= ~4 against differences ~1: 4 roundings of operands 4x larger) and, for joint 0, a sum of 23 such terms
#   whose magnitude may cancel to ~1/5 of its absolute sum: 23 * 4 * 5 u = 2.8e-5; the feet add two foot terms (3 roundings).
#  loss_terms + loss_total (c): per element 2-3 roundings (l2: the difference(s), the square), a float64 sum, the mean and the p2
#   product rounded (2), then the batch sum (b roundings of same-sign terms) and the coefficient (2): <= (b + 8) u = 2.4e-6 at b = 32.
#  fk_bwd (b): from the host build of the same fk_math.h (test_loss_reference_cpu.py::test_fk_bwd_host_error_estimate) on the rows
#   of the n = 14400 case: worst float32-vs-float64 error 1.5e-5 on rows 7..150 (random rows with a short a1 or a2: 1 / |a|
#   amplifies), 1.2e-7 on rows 4..6, 9.7e-6 on the joint positions; bounds ~5x, 16x and 5x of these.
#  composite (d): fk_bwd's bound plus the cotangent's own error (l2: the kernel's joints are float32 FK, 1e-5 relative): 1e-4.
#  The first MI355X run, worst over the grid (bound, margin): loss_terms_bwd d_out 1.8e-7 (4e-6, 22x), d_joints j0 2.1e-7 (4e-5),
#   feet 2.1e-7 / other 2.0e-7 (4e-6, 19x); terms 1.6e-7 (4e-6, 25x); fk_bwd rows 7..150 1.3e-5 (8e-5, 6x), rows 4..6 1.2e-7
#   (2e-6, 16x), positions 1.0e-5 (5e-5, 5x); _LossFn d_out 1.7e-5 (1e-4, 6x); p_losses d_out 2.6e-6 (1e-4 + the p2 slack).
BOUNDS = {
    "out": 4e-6,                 # loss_terms_bwd -> d_out, every region
    "joints": {"j0": 4e-5, "feet": 4e-6, "other": 4e-6},
    "terms": 4e-6,               # loss_terms + loss_total, relative per term
    "fk_rot": 8e-5,              # fk_bwd, rows 7..150 (6-D rotations)
    "fk_root": 2e-6,             # fk_bwd, rows 4..6 (root)
    "fk_pos": 5e-5,              # ax_from_6v + smpl_fk joint positions, relative to max |position|
    "composite": 1e-4,           # _LossFn backward, full d_out, every region
    "composite_terms": 2e-5,     # _LossFn forward terms (the FK and foot terms of float32 joints)
}
