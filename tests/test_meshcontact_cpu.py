"""CPU checks of mesh-level contact (no GPU): the numpy restatement tests/meshcontact_ref.py of include/tcdiff_meshcontact.h on cubes
whose answers the coordinates give exactly and on what the winding number is for, the eleventh header and its binding, the launchers'
and the entry points' refusals, BodyModel.closed, csrc/meshcontact_math.h built for the host as a stand-alone program with the address
and undefined-behaviour sanitizers against the restatement, and the condition the GPU comparison rests on: on the seeded scenes no
decision is a near-tie."""
import ctypes as C
import importlib
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import meshcontact_ref as R
import skin_ref
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd import body as B

M = importlib.import_module("tcdiff_amd.mesh_contact")          # the module: the package's attribute `mesh_contact` is the function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcm_mesh_contact_workspace", "tcm_mesh_contact"]


# ---- cubes: the coordinates give the answer ---------------------------------------------------------------------------------------------------
def cube(n, size, at):
    """box_mesh(n) scaled by `size` (a number or three) and moved to `at`; every number dyadic: exact in float32"""
    v, f = R.box_mesh(n)
    return (v.astype(np.float64) * np.asarray(size, np.float64) + np.asarray(at, np.float64)).astype(np.float32), f


def expected(src, dst):
    """which vertices of the cube src lie strictly inside the cube dst, and how far from its nearest side: from the coordinates"""
    s, d = src.astype(np.float64), dst.astype(np.float64)
    lo, hi = d.min(0), d.max(0)
    inside = ((s > lo) & (s < hi)).all(1)
    depth = np.minimum(s - lo, hi - s).min(1)
    return inside, np.where(inside, depth, np.nan)


def check_pair_of_cubes(a, b, faces):
    out = R.mesh_contact(np.stack([a, b])[None], faces, 2)
    best, arg = 0.0, (-1, -1, -1)
    for direction, (src, dst) in enumerate(((a, b), (b, a))):
        inside, depth = expected(src, dst)
        got_inside, got_depth, _ = R.inside_of(src, dst, faces)
        assert np.array_equal(got_inside, inside)
        assert np.array_equal(got_depth, depth, equal_nan=True)          # equality, not a tolerance
        assert out["inside"][0, 0, 0, direction] == inside.sum()
        for v in np.flatnonzero(inside):
            if depth[v] > best:                               # ascending dancer and vertex: the first of equals stays
                best, arg = depth[v], (0, direction, int(v))
    assert out["mesh_depth_max"][0, 0] == best == out["depth"][0, 0, 0] and tuple(out["mesh_deepest"][0, 0]) == arg
    contact = arg[0] == 0
    assert out["mesh_contact_rate"][0, 0] == float(contact) and out["mesh_contact_episodes"][0, 0] == int(contact)
    assert out["mesh_inside_mean"][0, 0] == float(out["inside"][0, 0, 0].sum())
    return out


def test_two_cubes_at_dyadic_offsets_give_exactly_what_the_coordinates_say():
    a, f = cube(2, 1.0, (0.0, 0.0, 0.0))
    b, _ = cube(2, 1.0, (0.625, 0.375, 0.3125))
    out = check_pair_of_cubes(a, b, f)
    assert out["inside"][0, 0, 0].tolist() == [4, 4] and out["mesh_depth_max"][0, 0] == 0.3125
    a, f = cube(4, 1.0, (0.0, 0.0, 0.0))
    b, _ = cube(4, 0.5, (0.6875, -0.15625, 0.71875))
    out = check_pair_of_cubes(a, b, f)
    assert out["inside"][0, 0, 0].sum() > 0


def test_a_cube_wholly_inside_another():
    a, f = cube(2, 0.25, (0.375, 0.3125, 0.4375))
    b, _ = cube(2, 1.0, (0.0, 0.0, 0.0))
    out = check_pair_of_cubes(a, b, f)
    assert out["inside"][0, 0, 0].tolist() == [26, 0] and out["mesh_depth_max"][0, 0] == 0.4375
    assert out["mesh_deepest"][0, 0, 1] == 0                  # the small cube is dancer 0


def test_disjoint_cubes_and_cubes_that_overlap_with_no_vertex_inside():
    a, f = cube(2, 1.0, (0.0, 0.0, 0.0))
    b, _ = cube(2, 1.0, (1.5, 0.25, 0.125))
    out = check_pair_of_cubes(a, b, f)
    assert out["inside"][0, 0, 0].tolist() == [0, 0] and tuple(out["mesh_deepest"][0, 0]) == (-1, -1, -1)
    a, f = cube(1, (2.0, 0.25, 0.25), (-1.0, 0.0, 0.0))           # two bars that cross: their volumes meet, no corner is inside
    b, _ = cube(1, (0.25, 2.0, 0.25), (0.0625, -0.9375, 0.0625))
    lo, hi = np.maximum(a.min(0), b.min(0)), np.minimum(a.max(0), b.max(0))
    assert (lo < hi).all()                                        # the boxes overlap
    out = check_pair_of_cubes(a, b, f)
    assert out["inside"][0, 0, 0].tolist() == [0, 0] and out["mesh_contact_rate"][0, 0] == 0.0 and out["mesh_depth_max"][0, 0] == 0.0


def test_reversing_every_face_flips_the_sign_of_w_and_changes_no_result():
    v, f, dn = R.scene("small")
    w, _ = R.winding(v[0, 0], v[0, 1], f)
    w_rev, _ = R.winding(v[0, 0], v[0, 1], f[:, ::-1])
    assert (w != 0).any() and np.array_equal(w_rev, -w)
    want, got = R.reference("small"), R.mesh_contact(v, f[:, ::-1], dn)
    for k in ("mesh_contact_rate", "mesh_contact_episodes", "mesh_deepest", "mesh_inside_mean", "inside"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    for k in ("mesh_depth_max", "depth"):                     # a face named C, B, A rounds its distance differently: a few float64 steps
        assert np.abs(got[k] - want[k]).max() <= 1e-15, k


@pytest.mark.parametrize("up", [0, 1])
def test_another_axis_up_gives_the_same_answer_on_the_rotated_scene(up):
    v, f, dn = R.scene("motion")
    moved = np.ascontiguousarray(v[..., {0: [2, 0, 1], 1: [0, 2, 1]}[up]])          # x, y, z of the header land where `up` reads them
    want, got = R.reference("motion"), R.mesh_contact(moved, f, dn, up=up)
    for k in R.METRICS + ("inside", "depth"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert got["margins"] == want["margins"]


def folded_scene():
    """body b: two closed lattices that overlap, as ONE mesh (V = 144); body a: the same topology, two small balls in the doubly
    covered region"""
    one = R.closed_lattice(10, 7)[1]
    faces = np.concatenate([one, one + 72]).astype(np.int32)
    b = np.concatenate([R.closed_lattice(10, 7, 11, (0.0, 0.0, 1.0))[0], R.closed_lattice(10, 7, 12, (0.5, 0.0, 1.0))[0]])
    a = np.concatenate([R.closed_lattice(10, 7, 13, (0.25, 0.0, 0.95), 0.08)[0], R.closed_lattice(10, 7, 14, (0.25, 0.05, 1.1), 0.08)[0]])
    return np.stack([a, b])[None], faces


def test_a_body_folded_through_itself_keeps_its_doubly_covered_region_inside():
    v, faces = folded_scene()
    assert R.closed(faces)
    w, _ = R.winding(v[0, 0], v[0, 1], faces)
    assert (np.abs(w) == 2).all()                             # every vertex of a is covered twice: the parity rule would say outside
    out = R.mesh_contact(v, faces, 2)
    assert out["inside"][0, 0, 0].tolist() == [144, 0] and out["mesh_contact_rate"][0, 0] == 1.0
    assert 0.15 < out["mesh_depth_max"][0, 0] < 0.35
    ok, why = R.decisions_clear(out)
    assert ok, why


def test_an_invalid_frame_leaves_every_rate_and_changes_no_other_frame():
    want = R.reference("motion")
    v, f, dn = R.with_nan("motion", clip=1, frame=6, dancer=1)
    got = R.mesh_contact(v, f, dn)
    pr = R.pairs(dn)
    for k, (a, b) in enumerate(pr):
        hit = 1 in (a, b)
        assert (got["inside"][1, k, 6] == -1).all() == hit and np.isnan(got["depth"][1, k, 6]) == hit
        keep = np.arange(12) != 6
        assert np.array_equal(got["inside"][1, k, keep], want["inside"][1, k, keep])
        assert np.array_equal(got["depth"][1, k, keep], want["depth"][1, k, keep])
        if hit:                                               # frame 6 sat in the middle of a run: the run is cut in two
            n = int((want["inside"][1, k, keep].sum(1) > 0).sum())
            assert got["mesh_contact_rate"][1, k] == n / 11 and got["mesh_contact_episodes"][1, k] == want["mesh_contact_episodes"][1, k] + 1
            assert got["mesh_inside_mean"][1, k] == float(want["inside"][1, k, keep].sum()) / 11
            assert got["mesh_deepest"][1, k, 0] != 6
    for k in R.METRICS:
        assert np.array_equal(got[k][0], want[k][0], equal_nan=True), k          # the other clip
        assert np.array_equal(got[k][1, 1], want[k][1, 1], equal_nan=True), k    # the pair (0, 2)
    v = np.array(v)
    v[1, :, 0, 0] = np.inf                                    # no valid frame in clip 1
    got = R.mesh_contact(v, f, dn)
    assert np.isnan(got["mesh_contact_rate"][1]).all() and np.isnan(got["mesh_inside_mean"][1]).all()
    assert (got["mesh_contact_episodes"][1] == 0).all() and (got["mesh_depth_max"][1] == 0).all() and (got["mesh_deepest"][1] == -1).all()


def test_a_single_frame_and_a_single_dancer():
    out = R.reference("single")
    assert out["inside"].shape == (1, 1, 1, 2) and out["mesh_contact_rate"].tolist() == [[1.0]] and out["mesh_contact_episodes"].tolist() == [[1]]
    assert out["mesh_deepest"][0, 0, 0] == 0 and out["mesh_depth_max"][0, 0] == out["depth"][0, 0, 0]
    out = R.reference("alone")
    assert out["mesh_contact_rate"].shape == (2, 0) and out["mesh_deepest"].shape == (2, 0, 3) and out["inside"].shape == (2, 0, 3, 2)


def test_the_seeded_meshes_are_what_the_tests_say():
    v, f = R.closed_lattice(10, 7, 1)
    assert v.shape == (72, 3) and f.shape == (140, 3) and R.closed(f)
    v, f = R.closed_lattice(23, 13, 1)
    assert v.shape == (301, 3) and f.shape == (598, 3) and R.closed(f)
    assert R.closed_lattice(83, 83)[0].shape == (6891, 3) and R.closed_lattice(83, 83)[1].shape == (13778, 3)
    v, f = R.box_mesh(4)
    assert v.shape == (98, 3) and f.shape == (192, 3) and R.closed(f) and np.array_equal(v * 4, np.round(v * 4))
    # the rule classifies random points against the perturbed sphere: inside below its least radius, outside above its largest
    v, f = R.closed_lattice(10, 7, 3, (0.0, 0.0, 0.0), 1.0)
    pts = np.random.default_rng(0).uniform(-1.2, 1.2, (400, 3)).astype(np.float32)
    w, _ = R.winding(pts, v, f)
    r = np.linalg.norm(pts, axis=1)
    assert set(np.unique(w)) <= {0, 1} and (w[r < 0.85] == 1).all() and (w[r > 1.07] == 0).all() and (r < 0.85).sum() > 30
    a, f = R.closed_lattice(10, 7, None, (0.0, 0.0, 1.0))
    b, _ = R.closed_lattice(10, 7, None, (0.9, 0.0, 1.0))
    inside, depth, _ = R.inside_of(a, b, f)
    assert inside.sum() == 3 and abs(np.nanmax(depth) - 0.187) < 1e-3          # the facetted counterpart of the spheres' 0.2 m


# ---- what the GPU comparison rests on ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_no_decision_is_a_near_tie_on_the_seeded_scenes(name):
    ok, why = R.decisions_clear(R.reference(name))
    assert ok, why


def test_the_seeded_scenes_are_not_trivial():
    motion = R.reference("motion")
    assert sorted(np.unique(motion["mesh_contact_episodes"]).tolist()) == [0, 3] and 0.0 < motion["mesh_contact_rate"].max() < 1.0
    assert R.reference("ontop")["inside"][0, 0, 0].tolist() == [1149, 0]          # more than one batch of candidates, all inside
    assert R.reference("ragged")["inside"].min() > 10
    for name in ("disjoint", "near"):
        assert (R.reference(name)["inside"] == 0).all(), name
    v, _, dn = R.scene("near")                                # its boxes do overlap
    lo, hi = v[0].min(1), v[0].max(1)
    assert (np.maximum(lo[0], lo[1]) < np.minimum(hi[0], hi[1])).all()
    v, _, dn = R.scene("disjoint")
    assert v[0, 1, :, 0].min() > v[0, 0, :, 0].max()


def test_the_guard_sees_a_near_tie():
    body, f = R.closed_lattice(10, 7, 1)
    other = np.array(R.closed_lattice(10, 7, 2, (0.4, 0.0, 1.0))[0])
    assert R.decisions_clear(R.mesh_contact(np.stack([other, body])[None], f, 2))[0]
    tied = np.array(other)
    tied[5, :2] = body[17, :2]                                # straight above or below a vertex of the body: p.x == xe of its edges
    ok, why = R.decisions_clear(R.mesh_contact(np.stack([tied, body])[None], f, 2))
    assert not ok and any("edge" in w for w in why)
    a, f = cube(2, 0.5, (0.125, 0.1875, 0.5))                 # its top side in the plane of the large cube's: z_hit == p.z
    b, _ = cube(2, 1.0, (0.0, 0.0, 0.0))
    ok, why = R.decisions_clear(R.mesh_contact(np.stack([a, b])[None], f, 2))
    assert not ok and any("height" in w for w in why)
    a, f = cube(2, 0.25, (0.375, 0.375, 0.375))               # centred: the eight corners are equally deep
    ok, why = R.decisions_clear(R.mesh_contact(np.stack([a, b])[None], f, 2))
    assert not ok and any("lead" in w for w in why)


# ---- csrc/meshcontact_math.h on the host, under the sanitizers ------------------------------------------------------------------------------------
def run_host(exe, tmp, v, faces, dn, up=2):
    rows, V = v.shape[:2]
    T = rows // dn
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([dn, T, V, faces.shape[0], up], np.int32).tobytes())
        f.write(np.ascontiguousarray(faces, np.int32).tobytes())
        f.write(np.ascontiguousarray(v, np.float32).tobytes())
    said = subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True).stdout.split()
    run_host.skipped, run_host.faces = run_host.skipped + int(said[0]), run_host.faces + int(said[2])
    return np.fromfile(fout, np.float64).reshape(dn * (dn - 1) // 2, T, 5)


run_host.skipped = run_host.faces = 0


def test_meshcontact_math_on_the_host_under_the_sanitizers_equals_the_restatement(tmp_path):
    """the SAME functions the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "meshcontact_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "meshcontact_host.cpp")])
    scenes = [(name,) + R.scene(name) + (R.reference(name),) for name in ("small", "ragged", "ontop", "single", "near", "motion")]
    v, f, dn = R.with_nan("motion", 1, 6, 1)
    scenes.append(("nan", v, f, dn, R.mesh_contact(v, f, dn)))
    v, f = folded_scene()
    scenes.append(("folded", v, f, 2, R.mesh_contact(v, f, 2)))
    a, f = cube(2, 1.0, (0.0, 0.0, 0.0))
    v = np.stack([a, cube(2, 1.0, (0.625, 0.375, 0.3125))[0]])[None]
    scenes.append(("cubes", v, f, 2, R.mesh_contact(v, f, 2)))
    frames = 0
    for name, v, f, dn, ref in scenes:
        for c in range(v.shape[0]):
            out = run_host(exe, tmp_path, v[c], f, dn)
            assert np.array_equal(out[..., :2], ref["inside"][c]), name
            assert np.array_equal(out[..., 2], ref["depth"][c], equal_nan=True), name          # to the bit
            for k in range(out.shape[0]):
                t = int(ref["mesh_deepest"][c, k, 0])
                if t >= 0:
                    assert out[k, t, 3:].tolist() == ref["mesh_deepest"][c, k, 1:].tolist(), (name, c, k)
            frames += out.shape[0] * out.shape[1]
    motion = R.scene("motion")
    moved = np.ascontiguousarray(motion[0][0][..., [2, 0, 1]])
    assert np.array_equal(run_host(exe, tmp_path, moved, motion[1], 3, up=0)[..., 2], R.reference("motion")["depth"][0])
    # the program also ran every distance pass the kernel's way (squared distances, faces skipped by their boxes, one root) and ended
    # with an error had a depth changed; the skipping is not idle
    assert run_host.skipped > run_host.faces // 2
    print(f"[meshcontact] host build equals the restatement on {frames} frames of pairs; {run_host.skipped} of {run_host.faces} faces "
          f"skipped by their boxes in the distance passes")


# ---- BodyModel.closed -----------------------------------------------------------------------------------------------------------------------------
def test_closed_on_closed_open_and_doubly_used_edge_meshes():
    lattice = R.closed_lattice(10, 7)[1]
    assert B.faces_closed(lattice) and B.faces_closed(R.box_mesh(2)[1]) and B.faces_closed(lattice[:, ::-1])
    assert not B.faces_closed(lattice[:-1])                                      # a hole
    assert not B.faces_closed(np.concatenate([lattice, lattice[:1]]))            # a face twice: its edges used twice
    flipped = np.array(lattice)
    flipped[0] = flipped[0, ::-1]                                                # one face wound the other way
    assert not B.faces_closed(flipped)
    assert not B.faces_closed(np.array([[0, 1, 1], [1, 0, 1]]))                  # an edge from a vertex to itself
    import shade_ref
    assert not B.faces_closed(shade_ref.lattice(10, 7)[1])                       # open at the poles
    for faces in (lattice, lattice[:-1], flipped, shade_ref.lattice(10, 7)[1]):
        assert B.faces_closed(faces) == R.closed(faces)
    model = skin_ref.make_model(72, 3, seed=5)
    assert B.load_body_model(model).closed() is False                            # make_model's triangle fan is open
    model["f"] = lattice.astype(np.uint32)
    body = B.load_body_model(model)
    assert body.closed() is True and body._closed is True and body.closed() is True          # cached


# ---- the eleventh header --------------------------------------------------------------------------------------------------------------------------
def test_the_eleventh_header_parses_and_is_bound_beside_the_frozen_sets():
    abi = _abi.load_meshcontact()
    assert list(abi.functions) == NAMES and L.MESH.functions == abi.functions and L.MESH.constants == abi.constants and not abi.structs
    assert abi.constants == dict(TC_MESH_LAUNCHES=3, TC_MESH_THREADS=256, TC_MESH_CANDIDATES=1024, TC_MESH_TILE=512, TC_MESH_WS_POSE=32,
                                 TC_MESH_WS_ORDERED=16)
    I, VP, LONG = C.c_int, C.c_void_p, C.c_long
    assert abi.functions["tcm_mesh_contact_workspace"][:2] == (I, [I] * 5 + [VP])
    assert abi.functions["tcm_mesh_contact"][:2] == (I, [VP] * 4 + [I] * 6 + [VP, LONG] + [VP] * 8)
    assert abi.functions["tcm_mesh_contact"][2][:4] == ["const float*", "const long*", "const int*", "const int*"]
    with open(_abi.HEADER_MESHCONTACT) as f:
        text = f.read()
    flat = " ".join(text.replace("*", " ").split())
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text and "Not built" in text
    assert "winding number, not a parity" in flat and "#define TC_MESH_LAUNCHES 3" in text
    for gone in ("edge-edge crossings between vertices", "contact of a dancer with itself", "the gap between surfaces that do not touch",
                 "using any of this inside keep_apart or ground", "a penetration volume", "a spatial hierarchy"):
        assert gone in flat, gone
    for prefix in ("tcdiff_", "tcx_", "tcs_", "tcr_", "tcj_", "tck_", "tcg_", "tcp_", "tcf_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_meshcontact.h", prefix=prefix)
    for names in (L.ABI.functions, L.EXT.functions, L.GLTF.functions, L.SKIN.functions, L.SHADE.functions, L.MJPEG.functions,
                  L.FOOTLOCK.functions, L.GROUP.functions, L.APART.functions, L.GROUND.functions, L.EXPORTS):
        assert not any(n.startswith("tcm_") for n in names)
    frozen = {**L.ABI.constants, **L.EXT.constants, **L.GLTF.constants, **L.SKIN.constants, **L.SHADE.constants, **L.MJPEG.constants,
              **L.FOOTLOCK.constants, **L.GROUP.constants, **L.APART.constants, **L.GROUND.constants}
    assert not any(k.startswith("TC_MESH_") for k in frozen) and len(L.ABI.functions) == 79 and len(L.GROUND.functions) == 3
    # the candidates (a point, an index, a depth, a bound) and the tile (nine floats, the flags): three workgroups fit a CU's 160 KiB of LDS
    lds = L.MESH.constants["TC_MESH_CANDIDATES"] * (12 + 4 + 8 + 4) + L.MESH.constants["TC_MESH_TILE"] * (36 + 4)
    assert 3 * lds <= 160 * 1024


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    syms = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    assert sorted(s for s in syms if s.startswith("tcm_")) == sorted(NAMES)
    lib = L.load()
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    n = C.c_long(-1)
    want = 32 * 2 * 5 * 3 + 16 * 2 * 5 * 3 * 2                            # boxes per pose, results per (clip, frame, ordered pair)
    assert lib.tcm_mesh_contact_workspace(2, 3, 5, 72, 140, C.addressof(n)) == 0 and n.value == want == 1920
    assert lib.tcm_mesh_contact_workspace(1, 1, 1, 1, 1, C.addressof(n)) == 0 and n.value == 32
    assert lib.tcm_mesh_contact_workspace(2, 3, 5, 72, 140, None) == -1
    for bad in ((0, 3, 5, 72, 140), (2, 0, 5, 72, 140), (2, 3, 0, 72, 140), (2, 3, 5, 0, 140), (2, 3, 5, 72, 0), (2, 3, -1, 72, 140)):
        assert lib.tcm_mesh_contact_workspace(*bad, C.addressof(n)) == -1, bad
    for big in ((2 ** 10, 3, 2 ** 10, 6890, 13776), (1, 2, 1, 2 ** 30, 1), (1, 2, 1, 3, 2 ** 30), (2 ** 12, 2 ** 10, 2 ** 8, 1, 1)):
        assert lib.tcm_mesh_contact_workspace(*big, C.addressof(n)) == -4, big
    faces = np.ascontiguousarray(R.closed_lattice(10, 7)[1])
    strides = (C.c_long * 2)(15 * 216, 216)
    big = 1 << 40

    def call(vertices=p, strides=strides, faces_dev=p, faces_host=faces.ctypes.data, b=2, dn=3, T=5, V=72, F=140, up=2, ws=p,
             ws_bytes=want - 1, inside=p, depth=p, rate=p, episodes=p, depth_max=p, deepest=p, inside_mean=p):
        return lib.tcm_mesh_contact(vertices, strides, faces_dev, faces_host, b, dn, T, V, F, up, ws, ws_bytes, inside, depth, rate, episodes,
                                    depth_max, deepest, inside_mean, None)

    assert call() == -1 and call(inside=None, depth=None) == -1          # good arguments but for one byte of workspace
    assert call(ws=p + 4, ws_bytes=want) == -2 and call(depth=p + 4, ws_bytes=want) == -2 and call(inside=p + 2, ws_bytes=want) == -2
    for kw in (dict(vertices=None), dict(strides=None), dict(faces_dev=None), dict(faces_host=None), dict(ws=None), dict(rate=None),
               dict(episodes=None), dict(depth_max=None), dict(deepest=None), dict(inside_mean=None), dict(b=0), dict(dn=0), dict(T=0),
               dict(T=-3), dict(V=0), dict(F=0), dict(up=-1), dict(up=3), dict(strides=(C.c_long * 2)(-1, 216)),
               dict(strides=(C.c_long * 2)(0, -216)), dict(V=71)):          # V = 71: the faces index vertex 71
        assert call(ws_bytes=big, **kw) == -1, kw
    wrong = np.array(faces)
    wrong[77, 1] = -1
    assert call(ws_bytes=big, faces_host=wrong.ctypes.data) == -1
    wrong[77, 1] = 72
    assert call(ws_bytes=big, faces_host=wrong.ctypes.data) == -1
    assert call(ws_bytes=big, b=2 ** 10, T=2 ** 10, V=6890) == -4 and call(ws_bytes=big, b=2 ** 10, T=2 ** 10, V=6890, up=3) == -1          # the order
    assert call(ws_bytes=big, b=2 ** 10, T=2 ** 10, V=6890, strides=(C.c_long * 2)(-1, 0)) == -4
    # one dancer: no pair, nothing to launch, and the checks still hold
    assert call(dn=1, ws_bytes=big) == 0 and call(dn=1, ws_bytes=big, up=3) == -1 and call(dn=1, ws_bytes=10) == -1


def test_the_eleventh_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.MESH.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_meshcontact.h"', '#include "tcdiff_meshcontact.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "meshcontact.c", tmp_path / "meshcontact"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.MESH.constants[n] for n in names]
    calls = ['#include "tcdiff_meshcontact.h"', '#include "tcdiff_meshcontact.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.MESH.functions.items():
        assert restype is C.c_int and argtypes == [C.c_void_p if c.endswith("*") else _abi.SCALARS[c] for c in ctexts], fname
        calls.append(f"  {{ int (*f)({', '.join(ctexts)}) = {fname}; (void)f; }}")
        zeros = [f"({c})0" if c.endswith("*") or c == "hipStream_t" else f"({c})z" for c in ctexts]
        calls.append(f"  (void){fname}({', '.join(zeros)});")
    calls.append("}")
    tu = tmp_path / "calls.c"
    tu.write_text("\n".join(calls))
    r = subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-c", str(tu), "-o", str(tmp_path / "calls.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the public interface ----------------------------------------------------------------------------------------------------------------------
def test_mesh_contact_and_evaluate_mesh_contact_refuse_before_any_launch():
    import tcdiff_amd
    assert tcdiff_amd.mesh_contact is M.mesh_contact and tcdiff_amd.evaluate_mesh_contact is M.evaluate_mesh_contact
    assert {"mesh_contact", "evaluate_mesh_contact"} <= set(tcdiff_amd.__all__)
    sig = inspect.signature(M.mesh_contact).parameters
    assert list(sig) == ["body_or_faces", "vertices", "dn", "up", "return_frames", "check_closed"]
    assert [sig[k].default for k in list(sig)[3:]] == [2, False, True] and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[3:])
    sig = inspect.signature(M.evaluate_mesh_contact).parameters
    assert list(sig)[:5] == ["samples", "normalizer", "dn", "body", "mode"] and sig["mode"].default == "normal"
    faces = R.closed_lattice(10, 7)[1]
    v = torch.zeros(2, 15, 72, 3)
    model = skin_ref.make_model(72, 3, seed=5)
    model["f"] = faces.astype(np.uint32)
    body = B.load_body_model(model)
    for first in (body, faces, faces.astype(np.int64), torch.from_numpy(faces)):
        with pytest.raises(L.TcdiffError, match="MI355X only"):
            M.mesh_contact(first, v, 3)
    for bad in (dict(vertices=v[0]), dict(vertices=v.double()), dict(vertices=v.numpy()), dict(vertices=v[:, :, :, :2]), dict(vertices=v[:, :0]),
                dict(vertices=v.transpose(-1, -2).contiguous().transpose(-1, -2)), dict(vertices=torch.zeros(2, 15, 71, 3)), dict(dn=0),
                dict(dn=4), dict(dn=3.0), dict(dn=True), dict(up=3), dict(up=-1), dict(up=True), dict(body_or_faces=faces[:, :2]),
                dict(body_or_faces=faces.astype(np.float32)), dict(body_or_faces=-faces), dict(body_or_faces=faces + 1),
                dict(body_or_faces=[[0, 1, 2]]), dict(body_or_faces=torch.from_numpy(faces).float()), dict(body_or_faces=None)):
        kw = dict(body_or_faces=body, vertices=v, dn=3)
        kw.update(bad)
        with pytest.raises(L.TcdiffError, match="mesh_contact"):
            M.mesh_contact(kw.pop("body_or_faces"), kw.pop("vertices"), kw.pop("dn"), check_closed="body_or_faces" not in bad, **kw)
    # a mesh that is not closed raises and says so; with check_closed=False the call goes on to the next check
    open_model = skin_ref.make_model(72, 3, seed=5)
    for first in (B.load_body_model(open_model), faces[:-1]):
        with pytest.raises(L.TcdiffError, match="not closed"):
            M.mesh_contact(first, v, 3)
        with pytest.raises(L.TcdiffError, match="MI355X only"):
            M.mesh_contact(first, v, 3, check_closed=False)
    with pytest.raises(L.TcdiffError, match="the body has 72"):
        M.mesh_contact(body, torch.zeros(2, 15, 80, 3), 3)
    assert "unpinned" in M.__doc__ and "Not built" in M.__doc__ and "winding number" in M.__doc__
    assert M.METRICS == R.METRICS
