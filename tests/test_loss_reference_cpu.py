"""tests/loss_ref.py -- the float64 loss head every kernel of the training loss is held to on the GPU (tests/test_loss_head_f64_gpu.py)
-- pinned to the oracle's p_losses (terms) and to float64 autograd of its own total (gradients), and shown to have power: each
plausible kernel defect it can emulate moves the region it touches by more than that region's GPU bound, on the GPU tests' inputs.
The fk_bwd bounds are estimated here from the host build of the same fk_math.h the kernel compiles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import loss_ref as R
from oracle import tcdiff_oracle as O

D = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("p2,cont", [(False, "some"), (True, "all"), (True, "edge")])
def test_reference_terms_equal_the_oracle_p_losses(l1, p2, cont):
    """target = x_start: the reference's four terms and total are the oracle's p_losses(model_out=...) in float64"""
    b, dn, S = 3, 2, 21
    mo, tg, t, w = R.make_case(b, dn, S, l1, p2, cont, 5)
    tab = O.make_tables(R.T_STEPS)
    tab["p2_loss_weight"] = w
    total, want = O.p_losses({}, tab, tg.to(D), None, t, torch.zeros(b, S, dn, 151, dtype=D), None,
                             loss_type="l1" if l1 else "l2", model_out=mo.to(D))
    got = R.loss_head(mo, tg, t, w, l1, with_vjp=False)
    assert float(want[3]) > 0 or cont == "none"
    for a, o in zip(got["terms"], want):
        assert abs(float(a) - float(o)) <= 1e-12, (float(a), float(o))
    assert abs(float(got["total"]) - float(total)) <= 1e-12


@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("shape,p2,cont", [((2, 3, 7), True, "some"), ((1, 1, 2), False, "all"), ((3, 2, 5), True, "edge")])
def test_reference_gradient_decomposition_equals_float64_autograd(l1, shape, p2, cont):
    """d_out_direct + VJP(d_joints) is float64 autograd of the reference total (l1 signs from the float64 differences, as autograd
    takes them), and autograd of k * total scales it by k (gscale)"""
    b, dn, S = shape
    mo, tg, t, w = R.make_case(b, dn, S, l1, p2, cont, 9)
    k = 2.75
    got = R.loss_head(mo, tg, t, w, l1, gscale=k, f32_signs=False)
    m = mo.to(D).reshape(b, S, dn, 151).clone().requires_grad_(True)
    mask = (mo.reshape(b, S, dn, 151)[..., :4] > torch.tensor(R.F95)).to(D)
    _, total, _, _ = R.terms_of(m, tg.to(D).permute(0, 2, 1, 3), w.to(D)[t], l1, mask)
    (k * total).backward()
    want = m.grad.reshape(b, S * dn, 151)
    assert float((got["d_out"] - want).abs().max()) <= 1e-12
    assert float(want.abs().max()) > 1e-6
    one = R.loss_head(mo, tg, t, w, l1, gscale=1.0, f32_signs=False)
    assert float((k * one["d_out"] - got["d_out"]).abs().max()) <= 1e-12 and float(one["d_out"].abs().max()) > 1e-6
    # with f32_signs the l1 signs may differ only where the float64 difference is within float32 rounding of zero; l2 is unaffected
    if not l1:
        assert torch.equal(R.loss_head(mo, tg, t, w, l1, gscale=k)["d_out"], got["d_out"])


# (defect, GPU case (b, dn, S, l1, p2, contacts, gscale), tensor, region it must move past its GPU bound)
DEFECT_CASES = [
    ("foot_drop", (2, 3, 20, False, True, "some", 1.0), "d_joints", "feet"),
    ("foot_drop", (1, 1, 2, True, False, "all", 0.37), "d_joints", "feet"),
    ("foot_one_side", (2, 3, 20, False, True, "some", 1.0), "d_joints", "feet"),
    ("foot_contact_s", (3, 2, 61, True, True, "some", 1.0), "d_joints", "feet"),
    ("foot_ge", (2, 3, 20, True, False, "edge", 0.37), "d_joints", "feet"),
    ("foot_ge", (3, 2, 61, False, True, "edge", 2.5), "d_joints", "feet"),
    ("p2_clip0", (2, 3, 20, False, True, "some", 1.0), "d_out_direct", "c7-150/interior"),
    ("p2_clip0", (32, 3, 150, True, True, "some", 0.37), "d_joints", "other"),
    ("p2_foot", (3, 2, 61, True, True, "some", 1.0), "d_joints", "feet"),
    ("vel_first", (3, 2, 61, False, False, "all", 0.37), "d_out_direct", "c7-150/first"),
    ("vel_first", (1, 1, 2, True, False, "all", 0.37), "d_out_direct", "c4-5/first"),
    ("vel_last", (3, 2, 61, True, True, "some", 1.0), "d_out_direct", "c6/last"),
    ("row_swap", (2, 3, 20, False, True, "some", 1.0), "d_out_direct", "c7-150/interior"),
    ("row_swap", (32, 3, 150, False, True, "some", 1.0), "d_joints", "feet"),
    ("l1_sign0", (3, 2, 61, True, True, "some", 1.0), "d_out_direct", "c4-5/interior"),
    ("l1_sign0", (2, 3, 20, True, False, "edge", 0.37), "d_out_direct", "c7-150/interior"),
    ("gscale_ignored", (2, 3, 20, True, False, "edge", 0.37), "d_out_direct", "c0-3/first"),
    ("gscale_ignored", (3, 2, 61, False, True, "edge", 2.5), "d_joints", "j0"),
    ("fk_root_drop", (2, 3, 20, False, True, "some", 1.0), "d_joints", "j0"),
    ("fk_root_drop", (1, 1, 2, True, False, "all", 0.37), "d_joints", "j0"),
]


def _bound(tensor, region):
    return R.BOUNDS["out"] if tensor == "d_out_direct" else R.BOUNDS["joints"][region]


@pytest.mark.parametrize("defect,case,tensor,region", DEFECT_CASES,
                         ids=[f"{d}-{c[0]}x{c[1]}x{c[2]}-{'l1' if c[3] else 'l2'}-{r}" for d, c, _, r in DEFECT_CASES])
def test_each_emulated_defect_exceeds_its_region_bound(defect, case, tensor, region):
    b, dn, S, l1, p2, cont, gs = case
    mo, tg, t, w = R.make_case(b, dn, S, l1, p2, cont, R.case_seed(case))
    good = R.loss_head(mo, tg, t, w, l1, gs, with_vjp=False)
    bad = R.loss_head(mo, tg, t, w, l1, gs, defects=(defect,), with_vjp=False)
    regions = R.out_regions(S, dn) if tensor == "d_out_direct" else R.JOINT_SETS
    st = R.region_errors(bad[tensor], good[tensor], regions, "out" if tensor == "d_out_direct" else "joints")
    print(f"{defect} at {case}: {tensor} moves by " + ", ".join(f"{k} {v[0]:.1e}" for k, v in st.items()))
    assert st[region][0] > 10 * _bound(tensor, region), (region, st[region])


def test_every_defect_is_emulated_on_a_gpu_case():
    assert {d for d, *_ in DEFECT_CASES} == set(R.DEFECTS)
    assert all(c in R.GPU_CASES for _, c, _, _ in DEFECT_CASES)


def test_no_defect_is_the_reference():
    """every switch off: the reference is deterministic and unchanged (the defect runs compare against it)"""
    case = (2, 3, 20, True, True, "edge", 0.37)
    mo, tg, t, w = R.make_case(*case[:6], R.case_seed(case))
    a, b = R.loss_head(mo, tg, t, w, True, 0.37), R.loss_head(mo, tg, t, w, True, 0.37, defects=())
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_the_gpu_cases_exercise_what_they_claim():
    """the inputs of the GPU grid: contacts exactly at float32(0.95) and its neighbours, exact l1 ties of entries and whole frames,
    distinct t per clip with 0 and T - 1, non-trivial p2 weights"""
    case = (2, 3, 20, True, True, "edge", 1.0)
    mo, tg, t, w = R.make_case(*case[:6], R.case_seed(case))
    c = mo[..., :4].numpy()
    f = R.F95
    assert (c == f).any() and (c == np.nextafter(f, np.float32(0))).any() and (c == np.nextafter(f, np.float32(2))).any()
    tok = tg.permute(0, 2, 1, 3).reshape(mo.shape)
    eq = mo[..., 4:] == tok[..., 4:]
    assert eq.any() and not eq.all()
    assert eq[0].reshape(20, 3, -1).all(-1).all(-1).sum() == 2          # two whole frames of clip 0
    assert len(set(t.tolist())) == 2 and set(t.tolist()) == {0, R.T_STEPS - 1}
    assert float(w.max() / w.min()) > 10 and len(set(R.timesteps(32, 1).tolist())) == 32


# ---- fk_bwd: the float32 error of the host build of fk_math.h, before any GPU run ---------------------------------------------
def _fk_host(tmp_path):
    so = str(tmp_path / "fk_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "host", "fk_host.cpp")])
    return C.CDLL(so)


def host_fk_bwd(lib, rows, cot):
    """fk_bwd_kernel's arithmetic on the host (fk_math.h under g++): (n, 151) rows, (n, 24, 3) cotangent -> (n, 151), rows 0..3 zero"""
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    n = rows.shape[0]
    d6 = np.ascontiguousarray(rows[:, 7:151].numpy().reshape(n * 24, 6))
    aa = np.zeros((n * 24, 3), np.float32)
    lib.host_ax_from_6v(fp(d6), C.c_long(n * 24), fp(aa))
    par = (C.c_int * 24)(*O.SMPL_PARENTS)
    off = np.array(O.SMPL_OFFSETS, np.float32)
    g = np.ascontiguousarray(cot.numpy().astype(np.float32))
    gaa, groot = np.zeros((n, 24, 3), np.float32), np.zeros((n, 3), np.float32)
    lib.host_fk_bwd(fp(aa), fp(g), C.c_long(n), par, fp(off), fp(gaa), fp(groot))
    g6 = np.zeros((n * 24, 6), np.float32)
    lib.host_ax_from_6v_bwd(fp(d6), fp(gaa), C.c_long(n * 24), fp(g6))
    out = np.zeros((n, 151), np.float32)
    out[:, 4:7], out[:, 7:151] = groot, g6.reshape(n, 144)
    joints = np.zeros((n, 24, 3), np.float32)
    root = np.ascontiguousarray(rows[:, 4:7].numpy())
    lib.host_fk(fp(aa), fp(root), C.c_long(n), par, fp(off), fp(joints))
    return torch.from_numpy(out), torch.from_numpy(joints)


def test_fk_bwd_host_error_estimate(tmp_path):
    """the float32-vs-float64 error of fk_bwd on the GPU test's rows (random, exact identity, within 1e-3 of pi with every quaternion
    candidate selected), from the host build: below a quarter of the GPU bounds R.BOUNDS["fk_rot"] / ["fk_root"] / ["fk_pos"]
    (host worst: rot 1.5e-5, root 1.2e-7, positions 9.7e-6; the first MI355X run measured 1.3e-5, 1.2e-7 and 1.0e-5)"""
    lib = _fk_host(tmp_path)
    n = 14400                                        # the largest GPU case's rows (test_fk_bwd_alone_vs_float64_vjp_and_accumulates)
    rows = R.fk_rows(n + 64, R.FK_SEED + n)[:n]
    cot = R.fk_cotangent(n + 64, R.FK_SEED + n)[:n]
    assert set(R.quat_candidate(rows).reshape(-1).tolist()) == {0, 1, 2, 3}
    got, pos = host_fk_bwd(lib, rows, cot)
    want = R.fk_vjp(rows, cot)
    pw = R.joints(rows.to(D))
    st = R.fk_errors(got, want)
    pe = float((pos.to(D) - pw).abs().max() / pw.abs().max())
    print("host fk_bwd vs float64: " + ", ".join(f"{k} {v:.1e}" for k, v in st.items()) + f"; positions {pe:.1e}")
    assert st["rot"] < R.BOUNDS["fk_rot"] / 4 and st["root"] < R.BOUNDS["fk_root"] / 4 and pe < R.BOUNDS["fk_pos"] / 4
    for kind in set(R.FK_KINDS):                     # each row kind on its own, too
        sel = [i for i in range(n) if R.FK_KINDS[i % 4] == kind]
        e = R.fk_errors(got[sel], want[sel])["rot"]
        print(f"   {kind}: rot {e:.1e}, positions {float((pos[sel].to(D) - pw[sel]).abs().max() / pw.abs().max()):.1e}")
        assert e < R.BOUNDS["fk_rot"] / 4, kind
    deg = R.degenerate_rows(64, 3)
    g_deg, _ = host_fk_bwd(lib, deg, R.fk_cotangent(64, 4))
    assert torch.isfinite(g_deg).all()
