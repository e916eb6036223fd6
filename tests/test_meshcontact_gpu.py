"""tcm_mesh_contact (csrc/meshcontact.hip) and tcdiff_amd/mesh_contact.py on an MI355X against the numpy float64 restatement
tests/meshcontact_ref.py.

Equality on every integer output: the counts of inside vertices, the episodes, the frame, dancer and vertex of the deepest one.  On
the float64 outputs -- the rate, the mean, the deepest depth and the depth plane -- the bound FLOAT_BOUND below: a hundred times the
largest difference measured (profiles/meshcontact.txt), and never looser than 1e-9 m.  The difference measured is 0 in every case, so
the bound is equality: kernel and restatement do the same correctly rounded float64 operations (+, -, *, /, sqrt) in the same order,
contraction off; minima and maxima round nothing and the counts are integers.  No case is excluded: the restatement first shows
(here again, and in tests/test_meshcontact_cpu.py for every seeded scene) that no decision is a near-tie.

The shapes are chosen against the header's constants: 72 vertices and 140 faces are less than one chunk of 256 and one tile of 512;
301 vertices are two chunks with a ragged second, 598 faces two tiles with a ragged second; 1149 vertices that are all inside overflow
one batch of 1024 candidates."""
import importlib

import numpy as np
import pytest
import torch

import meshcontact_ref as R
import skin_ref
from tcdiff_amd import _lib as L
from tcdiff_amd import body as B
from tcdiff_amd import export as E
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd import metrics as MT

M = importlib.import_module("tcdiff_amd.mesh_contact")          # the module: the package's attribute `mesh_contact` is the function
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = 0.0            # metres: the largest difference of a float64 output from the restatement over every case here (profiles/meshcontact.txt)
FLOAT_BOUND = min(100 * MEASURED, 1e-9)
FLOATS = ("mesh_contact_rate", "mesh_depth_max", "mesh_inside_mean", "depth")
INTS = (("mesh_contact_episodes", torch.int64), ("mesh_deepest", torch.int64), ("inside", torch.int32))
_worst = {"f64": 0.0}


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # a copy: the shared inputs are read-only


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), k


def _compare(got, want, what):
    assert list(got) == list(M.METRICS) + ["inside", "depth"], what
    for k, dtype in INTS:
        g = got[k]
        assert g.dtype == dtype and g.is_cuda and np.array_equal(g.cpu().numpy(), want[k]), (what, k, g.cpu().numpy(), want[k])
    worst = 0.0
    for k in FLOATS:
        g = got[k].cpu().numpy()
        assert g.dtype == np.float64 and g.shape == want[k].shape and np.array_equal(np.isnan(g), np.isnan(want[k])), (what, k)
        err = np.abs(g - want[k])[~np.isnan(want[k])]
        worst = max(worst, float(err.max()) if err.size else 0.0)
    _worst["f64"] = max(_worst["f64"], worst)
    print(f"[meshcontact] {what}: float64 outputs within {worst:.3e} of the restatement (bound {FLOAT_BOUND:.3e}); inside vertices "
          f"{int(np.maximum(want['inside'], 0).sum())}, deepest {float(want['mesh_depth_max'].max()) if want['mesh_depth_max'].size else 0.0:.4f} m; "
          f"so far {_worst['f64']:.3e}")
    assert worst <= FLOAT_BOUND, (what, worst)


def _clear(ref, what):
    ok, why = R.decisions_clear(ref)
    assert ok, f"a decision of the reference is a near-tie on {what}: {why}"
    return ref


@pytest.mark.parametrize("name", R.CASES)
def test_mesh_contact_equals_the_restatement_on_the_seeded_scenes(name):
    v, f, dn = R.scene(name)
    want = _clear(R.reference(name), name)
    got = M.mesh_contact(f, _dev(v), dn, return_frames=True)
    b, T, P = v.shape[0], v.shape[1] // dn, dn * (dn - 1) // 2
    assert tuple(got["inside"].shape) == (b, P, T, 2) and tuple(got["mesh_deepest"].shape) == (b, P, 3)
    _compare(got, want, f"{name} {tuple(v.shape)} dn {dn}")
    plain = M.mesh_contact(f, _dev(v), dn)
    assert list(plain) == list(M.METRICS)
    _same_bits(plain, {k: got[k] for k in M.METRICS})


@pytest.mark.parametrize("up", [0, 1])
def test_another_axis_up(up):
    v, f, dn = R.scene("motion")
    moved = np.ascontiguousarray(v[..., {0: [2, 0, 1], 1: [0, 2, 1]}[up]])
    _compare(M.mesh_contact(f, _dev(moved), dn, up=up, return_frames=True), R.reference("motion"), f"motion with up = {up}")


def test_a_body_folded_through_itself():
    one = R.closed_lattice(10, 7)[1]
    faces = np.concatenate([one, one + 72]).astype(np.int32)
    b = np.concatenate([R.closed_lattice(10, 7, 11, (0.0, 0.0, 1.0))[0], R.closed_lattice(10, 7, 12, (0.5, 0.0, 1.0))[0]])
    a = np.concatenate([R.closed_lattice(10, 7, 13, (0.25, 0.0, 0.95), 0.08)[0], R.closed_lattice(10, 7, 14, (0.25, 0.05, 1.1), 0.08)[0]])
    v = np.stack([a, b])[None]
    want = _clear(R.mesh_contact(v, faces, 2), "the folded body")
    assert want["inside"][0, 0, 0].tolist() == [144, 0]
    _compare(M.mesh_contact(faces, _dev(v), 2, return_frames=True), want, "folded body, V = 144")
    # an open mesh: refused, and with check_closed=False the signed count of the definition all the same
    want = _clear(R.mesh_contact(v, faces[:-3], 2), "the folded body with a hole")
    with pytest.raises(L.TcdiffError, match="not closed"):
        M.mesh_contact(faces[:-3], _dev(v), 2)
    _compare(M.mesh_contact(faces[:-3], _dev(v), 2, return_frames=True, check_closed=False), want, "folded body with a hole")


def test_a_strided_or_permuted_view_is_read_in_place_and_runs_repeat_their_bits():
    v, f, dn = R.scene("motion")
    b, rows, V = v.shape[:3]
    x = _dev(v)
    base = M.mesh_contact(f, x, dn, return_frames=True)
    _same_bits(M.mesh_contact(f, x, dn, return_frames=True), base)                     # the same input gives the same bits
    wide = torch.full((b, rows + 3, V, 3), float("nan"), device=DEV)                  # a window of a larger buffer: NaN all around it
    wide[:, 1:rows + 1] = x
    view = wide[:, 1:rows + 1]
    assert not view.is_contiguous() and view.data_ptr() != wide.data_ptr()
    _same_bits(M.mesh_contact(f, view, dn, return_frames=True), base)
    twin = torch.full((b, rows, 2, V, 3), float("nan"), device=DEV)                   # every other row
    twin[:, :, 1] = x
    _same_bits(M.mesh_contact(f, twin[:, :, 1], dn, return_frames=True), base)
    major = x.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)                    # stored row-major, clips inside
    assert major.stride(0) == V * 3 and major.stride(1) == b * V * 3
    _same_bits(M.mesh_contact(f, major, dn, return_frames=True), base)
    _compare(base, R.reference("motion"), "motion, the base of the views")


def test_the_outputs_land_where_they_are_told_and_nothing_else_is_written():
    v, f, dn = R.scene("small")
    b, rows, V = v.shape[:3]
    T, P, F, guard = rows // dn, dn * (dn - 1) // 2, f.shape[0], 64
    x, fd = _dev(v), _dev(f)
    want = M.mesh_contact(f, x, dn, return_frames=True)
    need = K.mesh_contact_workspace(b, dn, T, V, F)
    assert need == 32 * b * rows + 16 * b * T * P * 2
    shapes = {"inside": ((b, P, T, 2), torch.int32), "depth": ((b, P, T), torch.float64), "mesh_contact_rate": ((b, P), torch.float64),
              "mesh_contact_episodes": ((b, P), torch.int64), "mesh_depth_max": ((b, P), torch.float64),
              "mesh_deepest": ((b, P, 3), torch.int64), "mesh_inside_mean": ((b, P), torch.float64)}
    bufs, outs = {}, {}
    for k, (shape, dtype) in shapes.items():
        n = int(np.prod(shape))
        bufs[k] = torch.full((n + 2 * guard,), -77, dtype=dtype, device=DEV)
        outs[k] = bufs[k][guard:guard + n].view(shape)
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    vx = torch.full((x.numel() + 2 * guard,), 123.0, device=DEV)
    vx[guard:guard + x.numel()] = x.reshape(-1)
    before = vx.clone()
    K.mesh_contact(vx[guard:guard + x.numel()].view(x.shape), fd, f, dn, 2, ws[guard:guard + need], outs["inside"], outs["depth"],
                   outs["mesh_contact_rate"], outs["mesh_contact_episodes"], outs["mesh_depth_max"], outs["mesh_deepest"], outs["mesh_inside_mean"])
    torch.cuda.synchronize()
    for k in shapes:
        assert torch.equal(_bits(outs[k]), _bits(want[k])), k
        assert bool((bufs[k][:guard] == -77).all()) and bool((bufs[k][-guard:] == -77).all()), k
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[-guard:] == 0xA5).all())
    assert torch.equal(vx, before) and torch.equal(fd, _dev(f))                        # the inputs are read, never written
    # without the frame planes: the same per-pair outputs
    K.mesh_contact(x, fd, f, dn, 2, ws[guard:guard + need], None, None, outs["mesh_contact_rate"], outs["mesh_contact_episodes"],
                   outs["mesh_depth_max"], outs["mesh_deepest"], outs["mesh_inside_mean"])
    for k in M.METRICS:
        assert torch.equal(_bits(outs[k]), _bits(want[k])), k


def test_a_nan_vertex_changes_its_own_frames_pairs_and_nothing_else():
    base = M.mesh_contact(R.scene("motion")[1], _dev(R.scene("motion")[0]), 3, return_frames=True)
    v, f, dn = R.with_nan("motion", clip=1, frame=6, dancer=1)
    want = _clear(R.mesh_contact(v, f, dn), "motion with a NaN")
    got = M.mesh_contact(f, _dev(v), dn, return_frames=True)
    _compare(got, want, "motion with a NaN vertex in clip 1, frame 6, dancer 1")
    assert got["inside"][1, :, 6].cpu().tolist() == [[-1, -1], [0, 0], [-1, -1]]
    keep = torch.arange(12, device=DEV) != 6
    for k in ("inside", "depth"):
        assert torch.equal(_bits(got[k])[0], _bits(base[k])[0]) and torch.equal(_bits(got[k])[1][:, keep], _bits(base[k])[1][:, keep]), k
    for k in M.METRICS:
        assert torch.equal(_bits(got[k])[0], _bits(base[k])[0]) and torch.equal(_bits(got[k])[1, 1], _bits(base[k])[1, 1]), k


def _body(V=72, seed=5):
    model = skin_ref.make_model(V, 3, seed=seed, smpl_tree=True)
    model["f"] = R.closed_lattice(10, 7)[1].astype(np.uint32)          # a closed mesh over the random template: no person, but a surface
    return B.load_body_model(model, device=DEV)


def test_evaluate_mesh_contact_is_export_then_skin_then_mesh_contact():
    body = _body()
    assert body.closed()
    g = torch.Generator().manual_seed(13)
    dn, S = 3, 6
    norm = tio.Normalizer(torch.randn(400, 151, generator=g))
    x = (torch.rand(2, S * dn, 151, generator=g) * 2 - 1).to(DEV)
    got = M.evaluate_mesh_contact(x, norm, dn, body, return_frames=True)
    q, pos, _, _ = E.export_poses(x, norm, "normal", dn)
    vertices = B.skin(body, q, pos)
    assert tuple(vertices.shape) == (2, S * dn, 72, 3) and tuple(got["inside"].shape) == (2, 3, S, 2)
    _same_bits(got, M.mesh_contact(body, vertices, dn, return_frames=True))
    want = _clear(R.mesh_contact(vertices.cpu().numpy(), body.faces, dn), "the skinned synthetic body")
    _compare(got, want, "evaluate_mesh_contact on a synthetic body")
    summary = MT.summarize(M.evaluate_mesh_contact(x, norm, dn, body))
    assert list(summary) == list(M.METRICS) and all(type(s) is float for s in summary.values())
    # long mode: 3 half-overlapping windows of 6 frames are one song of 12
    x3 = (torch.rand(3, S * dn, 151, generator=g) * 2 - 1).to(DEV)
    long = M.evaluate_mesh_contact(x3, norm, dn, body, mode="long", return_frames=True)
    assert tuple(long["inside"].shape) == (1, 3, 12, 2) and tuple(long["mesh_contact_rate"].shape) == (1, 3)


def test_summarize_takes_the_result():
    v, f, dn = R.scene("motion")
    want = R.reference("motion")
    summary = MT.summarize(M.mesh_contact(f, _dev(v), dn))
    assert list(summary) == list(M.METRICS)
    assert abs(summary["mesh_contact_rate"] - float(np.mean(want["mesh_contact_rate"]))) <= 1e-12
    alone = M.mesh_contact(R.scene("alone")[1], _dev(R.scene("alone")[0]), 1, return_frames=True)
    assert tuple(alone["mesh_contact_rate"].shape) == (2, 0) and tuple(alone["inside"].shape) == (2, 0, 3, 2)
    assert tuple(alone["mesh_deepest"].shape) == (2, 0, 3) and all(t.is_cuda for t in alone.values())
