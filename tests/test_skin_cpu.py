"""CPU checks of the body skinning (no GPU): the fourth header, include/tcdiff_skin.h, and its binding; the launcher's validation;
csrc/skin_math.h built for the host as a stand-alone program against the numpy restatement tests/skin_ref.py; ``load_body_model``
on seeded synthetic models (no real model file is in the repository); ``build_glb(mesh=...)`` read back by the reader of
tests/gltf_ref.py and its skinned mesh evaluated in float64 against the restatement; no CPU fallback."""
import ctypes as C
import hashlib
import os
import pickle
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import scipy.sparse
import torch

import gltf_ref as G
import skin_ref as S
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd import body as B
from tcdiff_amd import gltf as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tcs_skin_vertices"
I, VP = C.c_int, C.c_void_p
ARGTYPES = [VP, VP, I, VP, VP, VP, VP, VP, VP, VP, I, I, I, I, VP, VP, VP, VP, VP]
CTYPES = ["const float*", "const float*", "int", "const float*", "const float*", "const float*", "const float*", "const int*",
          "const float*", "const int*", "int", "int", "int", "int", "float*", "float*", "float*", "float*", "hipStream_t"]


# ---- the fourth header ------------------------------------------------------------------------------------------------------------------
def test_the_fourth_header_parses_to_the_one_function_and_the_tile_sizes():
    abi = _abi.load_skin()
    assert abi.structs == {} and list(abi.functions) == [NAME] and abi.functions[NAME] == (I, ARGTYPES, CTYPES)
    assert L.SKIN.functions == abi.functions and L.SKIN.constants == abi.constants
    pt, vt = abi.constants["TC_SKIN_POSE_TILE"], abi.constants["TC_SKIN_VERT_TILE"]
    assert pt >= 1 and vt >= 1 and (B.POSE_TILE, B.VERT_TILE) == (pt, vt) and abi.constants["TC_SKIN_FEAT"] == 208
    assert abi.constants["TC_SKIN_ORIGIN_PELVIS"] != abi.constants["TC_SKIN_ORIGIN_SMPL"] and len(abi.constants) == 5
    with open(_abi.HEADER_SKIN) as f:
        text = f.read()
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text
    with pytest.raises(_abi.TcdiffError, match="unknown declaration"):                          # neither tcdiff_ nor tcx_
        _abi.parse(text, "include/tcdiff_skin.h")
    with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
        _abi.parse(text, "include/tcdiff_skin.h", prefix="tcx_")


def test_the_binding_is_in_none_of_the_frozen_sets():
    for names in (L.ABI.functions, L.EXT.functions, L.GLTF.functions, L.EXPORTS):
        assert NAME not in names and not any(n.startswith("tcs_") for n in names)
    assert not any(k.startswith("TC_SKIN") for k in {**L.ABI.constants, **L.EXT.constants, **L.GLTF.constants})
    assert not hasattr(L, "SKIN_POSE_TILE")                               # the constants stay in L.SKIN.constants


def _dynamic_symbols(path):
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split()}
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", path], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    return {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}


def test_the_built_library_defines_the_launcher_and_it_validates_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    syms = _dynamic_symbols(L.LIB_PATH)
    assert [s for s in syms if s.startswith("tcs_")] == [NAME]
    assert not [s for s in syms if "skin" in s.lower() and (s.startswith("tcdiff_") or s.startswith("tcx_"))]
    lib = L.load()
    assert lib.tcs_skin_vertices.argtypes == ARGTYPES and lib.tcs_skin_vertices.restype is I
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # 16-byte aligned, never dereferenced: every call fails a check
    good = (C.c_int * 24)(*S.SMPL_PARENTS)

    def go(P=1, V=1, K=1, pose_blend=1, origin=0, parents=good, feat=p, A=p, joints_out=p, **null):
        ptr = {k: (None if k in null else p) for k in ("poses", "trans", "v_shaped", "blend", "joints", "offsets", "weights", "wj", "out")}
        par = None if parents is None else C.cast(parents, VP)
        return lib.tcs_skin_vertices(ptr["poses"], ptr["trans"], P, ptr["v_shaped"], ptr["blend"], ptr["joints"], ptr["offsets"], par,
                                     ptr["weights"], ptr["wj"], V, K, pose_blend, origin, feat, A, joints_out, ptr["out"], None)
    big = 2 ** 31 - 1
    bad_tail = dict(feat=p + 4, P=big, V=big)                             # what the later checks would object to
    for k in ("poses", "trans", "v_shaped", "blend", "joints", "offsets", "weights", "wj", "out"):
        assert go(**{k: None}, **bad_tail) == -1, k
    assert go(parents=None, **bad_tail) == -1 and go(feat=None, P=big) == -1 and go(A=None, P=big) == -1
    for kw in (dict(P=0), dict(P=-1), dict(V=0), dict(V=-5), dict(K=0), dict(K=9), dict(K=-1)):
        assert go(feat=p + 4, **kw) == -1, kw
    for kw in (dict(pose_blend=2), dict(pose_blend=-1), dict(origin=2), dict(origin=-1)):
        assert go(feat=p + 4, P=big, **kw) == -1, kw
    cycle = list(S.SMPL_PARENTS)
    cycle[4], cycle[1] = 7, 4                                             # 1 -> 4 -> 7 -> 4: joint 4's parent comes after it
    two_roots, no_root, self_parent = [-1, -1] + S.SMPL_PARENTS[2:], [0] + S.SMPL_PARENTS[1:], S.SMPL_PARENTS[:5] + [5] + S.SMPL_PARENTS[6:]
    for bad in (cycle, two_roots, no_root, self_parent, [24] + [24] * 23):
        assert go(parents=(C.c_int * 24)(*bad), feat=p + 4, P=big) == -1, bad
    assert go(feat=p + 4, P=big) == -2 and go(A=p + 8, V=big) == -2 and go(feat=p + 12, A=p + 4) == -2
    assert go(P=big) == -4 and go(V=big) == -4 and go(P=2 ** 16, V=2 ** 16) == -4
    assert go(P=(big // 288) + 1) == -4 and go(P=2, V=big // 6 + 1) == -4 and go(P=big, V=big, K=8, joints_out=None) == -4


def test_the_fourth_header_read_by_the_c_compiler(tmp_path):
    """the pattern of test_the_third_header_read_by_the_c_compiler: the macros' values, and a translation unit that calls the
    launcher with every argument cast to its parsed C type and assigns it to a function pointer of the parsed signature"""
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.SKIN.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_skin.h"', '#include "tcdiff_skin.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "skin.c", tmp_path / "skin"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.SKIN.constants[n] for n in names]
    calls = ['#include "tcdiff_skin.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.SKIN.functions.items():
        assert restype is C.c_int and argtypes == [C.c_void_p if c.endswith("*") else _abi.SCALARS[c] for c in ctexts], fname
        calls.append(f"  {{ int (*f)({', '.join(ctexts)}) = {fname}; (void)f; }}")
        zeros = [f"({c})0" if c.endswith("*") or c == "hipStream_t" else f"({c})z" for c in ctexts]
        calls.append(f"  (void){fname}({', '.join(zeros)});")
    calls.append("}")
    tu = tmp_path / "calls.c"
    tu.write_text("\n".join(calls))
    r = subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-c", str(tu), "-o", str(tmp_path / "calls.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- csrc/skin_math.h on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("skin_host")
    exe = str(d / "skin_host")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "skin_host.cpp")])

    def run(im, poses, trans, origin):
        P = len(poses)
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([P, origin == "smpl"], np.int32).tobytes() + np.array(im["parents"], np.int32).tobytes())
            for a in (im["J"], im["offsets"], poses, trans):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        raw = np.fromfile(d / "out.bin", np.float32)
        assert raw.size == P * (208 + 288 + 72)
        return raw[:208 * P].reshape(P, 208), raw[208 * P:496 * P].reshape(P, 24, 12), raw[496 * P:].reshape(P, 24, 3)
    return run


def _crafted_poses():
    """a special case per joint of pose 0 .. 5 (the rest small seeded rotations), and a chain 23 deep comes with the model:
    the zero vector; theta = 1e-4; theta on both sides of 1e-3 (0.999e-3, 1.001e-3, float32(1e-3)); float32(pi); an unwrapped 4"""
    g = np.random.default_rng(11)
    poses = (0.4 * g.standard_normal((8, 24, 3))).astype(np.float32)
    unit = np.array([2.0, -1.0, 2.0]) / 3
    poses[0] = 0
    poses[1] = (1e-4 * unit).astype(np.float32)
    for j in range(24):
        poses[2, j] = np.float32((0.999e-3, 1.001e-3, 1e-3)[j % 3]) * np.float32([0, 1, 0] if j % 2 else [1, 0, 0])
    poses[3] = np.float32(np.pi) * np.float32([0, 0, 1])
    poses[4] = np.float32(4.0) * np.float32([1, 0, 0])
    poses[5, 1::2] = (np.float32(np.pi) * unit).astype(np.float32)
    trans = g.uniform(-2, 2, (8, 3)).astype(np.float32)
    return poses, trans


def _chain_model(V=5):
    m = S.make_model(V, 2, seed=4)
    m["kintree_table"][0] = [2 ** 32 - 1] + list(range(23))               # joint j hangs on j - 1: a chain 23 deep
    return m


@pytest.mark.parametrize("origin", ["pelvis", "smpl"])
def test_skin_math_on_the_host_reproduces_the_restatement(host, origin):
    """the SAME source the HIP kernel compiles, built with g++ without contraction: feat, A and the joints with error 0"""
    for what, model, (poses, trans) in (("crafted, a chain 23 deep", _chain_model(), _crafted_poses()),
                                        ("crafted, SMPL's tree", S.make_model(7, 3, seed=2, smpl_tree=True), _crafted_poses()),
                                        ("seeded, a random tree", S.make_model(7, 3, seed=3), S.poses_of(33))):
        im = S.images(model)
        feat, A, joints, _ = S.pose_part(im, poses, trans, origin)
        got = host(im, poses, trans, origin)
        for name, g, w in zip(("feat", "A", "joints"), got, (feat, A, joints)):
            err = float(np.abs(g.astype(np.float64) - w.astype(np.float32).astype(np.float64)).max())
            print(f"host, {what}, origin {origin}: {name} largest error {err:.3e}")
            assert g.shape == w.shape and err == 0.0, (what, name, err)
        assert (got[0][:, 207] == 0).all()
    im = S.images(_chain_model())
    poses, trans = _crafted_poses()
    feat, A, joints, shift = S.pose_part(im, poses, trans, origin)
    assert (feat[0] == 0).all() and np.array_equal(A[0].reshape(24, 3, 4)[:, :, :3], np.tile(np.eye(3), (24, 1, 1)))   # the zero vector: rest
    # (offsets and J are each rounded to float32 once, so the chain of offsets meets J to float32's rounding, 23 joints deep)
    assert np.abs(A[0].reshape(24, 3, 4)[:, :, 3]).max() < 2e-6
    assert np.abs(joints[0] - (im["J"].astype(np.float64) + shift[0])).max() < 2e-6
    R = S.rodrigues(poses)                                                # both branches give rotations: R R^T = 1, to 1e-15
    assert np.abs(R @ R.transpose(0, 1, 3, 2) - np.eye(3)).max() < 4e-15
    r = poses[1, 0].astype(np.float64)
    assert abs(R[1, 0, 0, 1] - (0.5 * r[0] * r[1] - r[2])) < 1e-12        # theta = 1e-4: R = 1 + K + K K / 2 to second order
    assert np.abs(R[3, 0] - np.diag([-1.0, -1.0, 1.0])).max() < 2e-7 and np.abs(R[4, 0, 1:, 1:] - [[np.cos(4), -np.sin(4)], [np.sin(4), np.cos(4)]]).max() < 1e-15


# ---- load_body_model ----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert (a.V, a.K, a.parents) == (b.V, b.K, b.parents)
    for k in ("v_shaped", "J", "offsets", "blend", "weights", "weight_values", "weight_joints", "faces", "betas"):
        assert np.array_equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype, k


def test_load_body_model_from_a_mapping_a_npz_and_a_pkl(tmp_path):
    m = S.make_model(37, 5, seed=1)
    one = B.load_body_model(m, device="cpu")
    assert (one.V, one.K) == (37, 5) and one.parents[0] == -1 and one.blend.shape == (207, 111) and one.faces.shape == (35, 3)
    np.savez(tmp_path / "m.npz", **m)
    _same(one, B.load_body_model(str(tmp_path / "m.npz")))
    as_pickled = dict(m, J_regressor=scipy.sparse.csc_matrix(m["J_regressor"]), v_template=m["v_template"].astype(np.float64))
    with open(tmp_path / "m.pkl", "wb") as f:
        pickle.dump(as_pickled, f, protocol=2)
    _same(one, B.load_body_model(tmp_path / "m.pkl"))
    _same(one, B.load_body_model(as_pickled))
    im = S.images(m)                                                      # the prepared arrays are the restatement's
    assert np.array_equal(one.v_shaped, im["v_shaped64"]) and np.array_equal(one.J, im["J64"]) and np.array_equal(one.offsets, im["offsets64"])
    assert np.array_equal(one.blend.astype(np.float32), im["blend"]) and one.blend[5, 3 * 7 + 2] == m["posedirs"][7, 2, 5]
    assert np.array_equal(one.weight_values.astype(np.float32), im["wv"]) and np.array_equal(one.weight_joints, im["wj"])
    assert (np.diff(one.weight_joints, axis=1) > 0).all() and (one.offsets[0] == 0).all() and one.parents == im["parents"]
    betas = [1.5, -2.0]
    moved = B.load_body_model(m, betas=betas)
    assert np.array_equal(moved.J, S.images(m, betas)["J64"]) and np.abs(moved.J - one.J).max() > 1e-3 and moved.betas.tolist() == betas + [0, 0]
    fewer = S.make_model(9, 3, seed=2)
    fewer["weights"][4] = 0
    fewer["weights"][4, 17] = 1.0                                         # one vertex with a single weight: padded with 0 on joint 0
    b = B.load_body_model(fewer)
    assert b.K == 3 and b.weight_values[4].tolist() == [1.0, 0.0, 0.0] and b.weight_joints[4].tolist() == [17, 0, 0]
    with pytest.raises(L.TcdiffError, match="betas"):
        B.load_body_model(m, betas=[0.0] * 5)
    with pytest.raises(L.TcdiffError, match="neither"):
        B.load_body_model(str(tmp_path / "m.fbx"))


def test_every_malformed_model_raises_and_names_the_key():
    m = S.make_model(12, 3, seed=5)

    def bad(key, value, match=None):
        with pytest.raises(L.TcdiffError, match=match or key):
            B.load_body_model(dict(m, **{key: value}))
    for key in S.make_model(1, 1):                                        # a wrong shape, key by key
        bad(key, np.asarray(m[key])[..., :-1] if key not in ("v_template", "shapedirs") else m[key][:, :2])
        bad(key, np.asarray(m[key])[None])
        missing = {k: v for k, v in m.items() if k != key}
        with pytest.raises(L.TcdiffError, match=key):
            B.load_body_model(missing)
    for key in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights"):
        for value in (np.nan, np.inf):
            a = np.array(m[key], np.float64)
            a.reshape(-1)[3] = value
            bad(key, a, f"{key}.*finite")
    f = np.array(m["f"], np.int64)
    f[2, 1] = 12
    bad("f", f, "'f' indexes vertex 12 of 12")
    f[2, 1] = -1
    bad("f", f, "'f'")
    bad("f", np.array(m["f"], np.float64) + 0.5, "'f'.*whole")
    w = np.array(m["weights"])
    w[3] = 0
    w[3, :9] = 1 / 9
    bad("weights", w, "'weights' gives vertex 3 9 nonzero")
    w[3] = 0
    bad("weights", w, "'weights' gives vertex 3 0 nonzero")
    kt = np.array(m["kintree_table"], np.int64)
    kt[0] = [-1] + list(range(23))
    kt[0, 4], kt[0, 7] = 7, 4                                             # 4 -> 7 -> 4
    bad("kintree_table", kt, "'kintree_table' gives joint 4 the parent 7")
    kt[0] = [-1, -1] + list(range(22))
    bad("kintree_table", kt, "'kintree_table'.*root")
    kt[0] = [0] + list(range(23))
    bad("kintree_table", kt, "'kintree_table'")
    bad("J_regressor", "a string", "'J_regressor'")


def test_an_unreadable_pickle_member_raises_the_advice(tmp_path):
    """a member of a class whose package is not installed (the official files hold chumpy objects): the key is named, converting to
    .npz is advised, and nothing by that name is imported"""
    fake = types.ModuleType("chumpy_like_package_that_is_not_installed")

    class Ch:
        def __init__(self, x):
            self.x = np.asarray(x)
    Ch.__module__, Ch.__qualname__ = fake.__name__, "Ch"
    fake.Ch = Ch
    m = S.make_model(6, 2, seed=6)
    sys.modules[fake.__name__] = fake
    try:
        for proto in (2, 4):
            with open(tmp_path / f"c{proto}.pkl", "wb") as f:
                pickle.dump(dict(m, posedirs=Ch(m["posedirs"]), extra=Ch(1.0)), f, protocol=proto)
    finally:
        del sys.modules[fake.__name__]
    for proto in (2, 4):
        with pytest.raises(L.TcdiffError, match=r"'posedirs' is a chumpy_like_package_that_is_not_installed\.Ch object.*\.npz"):
            B.load_body_model(tmp_path / f"c{proto}.pkl")
        assert fake.__name__ not in sys.modules
    with open(tmp_path / "list.pkl", "wb") as f:
        pickle.dump([1, 2], f)
    with pytest.raises(L.TcdiffError, match="mapping"):
        B.load_body_model(tmp_path / "list.pkl")
    with open(tmp_path / "os.pkl", "wb") as f:                            # a pickle that names a callable outside numpy / scipy runs nothing
        f.write(b"cos\nsystem\n(S'true'\ntR.")
    with pytest.raises(L.TcdiffError, match="mapping"):
        B.load_body_model(tmp_path / "os.pkl")


# ---- build_glb(mesh=...) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("V", [1, 37])
@pytest.mark.parametrize("T,dn", [(1, 1), (7, 3)])
def test_build_glb_with_a_mesh_reads_back_and_its_skin_is_the_restatement(T, dn, V, K):
    """the file's skinned mesh, evaluated in float64 as the glTF specification says, is the restatement's pose_blend=False,
    origin="pelvis" vertices turned (x, z, -y), the restatement given the same four weights.  Bound: test_gltf_cpu.py's
    end-to-end bound for joints, 1e-5 m (metre-size inputs, float32 quaternions).  Observed: 6.4e-8 .. 1.9e-7 m at V = 37; 2e-16 at V = 1, whose joints all sit on the one vertex."""
    poses, trans, out, _ = G.seeded(1, T, dn)
    model = S.make_model(V, K, seed=10 * V + K)
    body = B.load_body_model(model)
    data = X.build_glb(out[0], T, dn, 30.0, mesh=body)
    assert data == X.build_glb(out[0].copy(), T, dn, 30.0, mesh=B.load_body_model(model))
    gltf, binary = G.read_glb(data)
    assert binary[:4 * G.floats(T, dn)] == out[0].tobytes()
    kept, dropped = S.top_four(model["weights"])
    im = S.images(model, weights=kept)
    got = S.skinned(gltf, binary)
    assert len(got) == dn == len(gltf["meshes"]) == len(gltf["skins"])
    worst = 0.0
    for d in range(dn):
        want, _ = S.vertices(im, poses[0, :, d], trans[0, :, d], pose_blend=False, origin="pelvis")
        assert got[d].shape == (T, V, 3)
        worst = max(worst, float(np.abs(got[d] - S.to_y_up(want)).max()))
    print(f"T = {T}, dn = {dn}, V = {V}, K = {K}: the file's skinned vertices against the restatement, largest error {worst:.3e} m (bound 1e-5)")
    assert worst <= 1e-5
    # the static data: POSITION = v_shaped, the four largest weights renormalised, the model's skeleton
    prim, = gltf["meshes"][0]["primitives"]
    at = {k: G.accessor(gltf, binary, v) for k, v in prim["attributes"].items()}
    assert gltf["meshes"][0]["name"] == "d0_surface" and all(m["primitives"][0]["attributes"] == prim["attributes"] for m in gltf["meshes"])
    assert np.array_equal(at["POSITION"], body.v_shaped.astype(np.float32)) and at["JOINTS_0"].dtype == np.uint8
    dense = np.zeros((V, 24))
    for i in range(4):
        np.add.at(dense, (np.arange(V), at["JOINTS_0"][:, i]), at["WEIGHTS_0"][:, i].astype(np.float64))
    assert np.abs(dense - kept).max() < 1e-7 and np.abs(at["WEIGHTS_0"].astype(np.float64).sum(1) - 1).max() < 2e-7
    assert (at["JOINTS_0"][at["WEIGHTS_0"] == 0] == 0).all() and (np.diff(at["WEIGHTS_0"], axis=1) <= 0).all()
    if K == 5:                                                            # the mass a core-glTF skin drops, per vertex
        assert dropped.min() > 0 and np.abs(dense * (1 - dropped)[:, None] - np.where(kept > 0, model["weights"], 0)).max() < 1e-7
        assert ((model["weights"] > 0).sum(1) == 5).all() and ((dense > 0).sum(1) == 4).all()
    else:
        assert (dropped == 0).all() and np.abs(dense - model["weights"]).max() < 1e-7
    idx = G.accessor(gltf, binary, prim["indices"])
    assert gltf["accessors"][prim["indices"]]["componentType"] == 5123 and np.array_equal(idx.reshape(-1, 3), model["f"])
    assert np.abs(np.sqrt((at["NORMAL"].astype(np.float64) ** 2).sum(1)) - 1).max() < 1e-6
    ibm = G.accessor(gltf, binary, gltf["skins"][0]["inverseBindMatrices"]).reshape(24, 4, 4)
    assert np.array_equal(ibm[:, 3, :3], (-body.J).astype(np.float32)) and np.array_equal(ibm[:, :3, :3], np.tile(np.eye(3, dtype=np.float32), (24, 1, 1)))
    for j in range(24):
        node = gltf["nodes"][j]
        assert node.get("children", []) == [k for k in range(24) if body.parents[k] == j]
        assert ("translation" not in node) if j == 0 else (node["translation"] == [float(x) for x in body.offsets[j]])


def test_the_rest_normals_and_wide_indices():
    m = S.make_model(4, 1, seed=3)
    m["v_template"] = np.array([[0.0, 0, 0], [1, 0, 0], [0, 0, 1], [5, 5, 5]])
    m["shapedirs"] = np.zeros((4, 3, 4))
    m["f"] = np.array([[0, 2, 1], [3, 3, 3]])                             # one face in the plane y = 0 facing +y; vertex 3 on a face of no area
    pos, nrm, _, _, idx = X._surface(B.load_body_model(m))
    assert np.array_equal(nrm, np.float32([[0, 1, 0]] * 4)) and idx.dtype == np.uint16
    m["f"] = np.array([[0, 1, 2], [3, 3, 3]])
    assert np.array_equal(X._surface(B.load_body_model(m))[1], np.float32([[0, -1, 0]] * 3 + [[0, 1, 0]]))
    m["v_template"] = np.array([[0.0, 0, 0], [2, 0, 0], [0, 0, 1], [0, 1, 0]])      # areas 1 and 1/2: the larger face weighs more
    m["f"] = np.array([[0, 2, 1], [0, 3, 2]])
    n0 = X._surface(B.load_body_model(m))[1][0].astype(np.float64)
    assert np.abs(n0 - np.array([1.0, 2.0, 0.0]) / np.sqrt(5)).max() < 1e-7
    V = 65536                                                             # one vertex more than 16-bit indices reach
    big = {"v_template": np.zeros((V, 3)), "shapedirs": np.zeros((V, 3, 1)), "posedirs": np.zeros((V, 3, 207)),
           "J_regressor": np.full((24, V), 1.0 / V), "weights": np.eye(24)[np.arange(V) % 24], "kintree_table": m["kintree_table"],
           "f": np.array([[0, 1, V - 1]])}
    body = B.load_body_model(big)
    assert X._surface(body)[4].dtype == np.uint32
    gltf, binary = G.read_glb(X.build_glb(G.seeded(1, 1, 1)[2][0], 1, 1, 30.0, mesh=body))
    a = gltf["accessors"][gltf["meshes"][0]["primitives"][0]["indices"]]
    assert a["componentType"] == 5125 and G.accessor(gltf, binary, gltf["meshes"][0]["primitives"][0]["indices"]).tolist() == [0, 1, V - 1]


PARENT_COMMIT = {(7, 3, True): "a5ae865aa859771d61b37da50163a6bb3564d0b9c49f41b2fa7855e35e7118df",
                 (7, 3, False): "46dc0a3a39878db18529cd3d687a0eac4ac750421464c708af42e2984996f22e",
                 (1, 1, True): "8d2ce24b143f4d6c9f068b1b08a630401e2b4eb778d5c1290efcdf4982bbbf82",
                 (1, 1, False): "fe2a92dcb10f0ae9de54145c446958d7ac2f9806f5070fe11bcd4d423eefd5e1"}


def test_without_a_mesh_every_byte_is_what_it_was_and_a_second_skeleton_raises():
    """sha256 of build_glb's files before mesh= existed, on a block made by integer arithmetic alone (no libm in it)"""
    for (T, dn, with_body), digest in PARENT_COMMIT.items():
        blk = ((np.arange(G.floats(T, dn)) * 37 % 101) / 64.0).astype(np.float32)
        plain = X.build_glb(blk, T, dn, 30.0, body=with_body)
        assert hashlib.sha256(plain).hexdigest() == digest and plain == X.build_glb(blk, T, dn, 30.0, body=with_body, mesh=None)
    body = B.load_body_model(S.make_model(5, 2, seed=1))
    _, _, out, _ = G.seeded(1, 7, 3)
    assert X.build_glb(out[0], 7, 3, 30.0, mesh=body) != X.build_glb(out[0], 7, 3, 30.0)
    for kw in (dict(offsets=body.offsets), dict(parents=body.parents), dict(parents=body.parents, offsets=body.offsets), dict(body=False)):
        with pytest.raises(L.TcdiffError, match="mesh="):
            X.build_glb(out[0], 7, 3, 30.0, mesh=body, **kw)
    with pytest.raises(L.TcdiffError, match="load_body_model"):
        X.build_glb(out[0], 7, 3, 30.0, mesh=S.make_model(5, 2))
    for fn in (X.build_glb, X.write_glb, X.write_glb_out, X.convert_fk_out):
        import inspect
        assert inspect.signature(fn).parameters["mesh"].default is None, fn


# ---- the host side ------------------------------------------------------------------------------------------------------------------------
def test_no_cpu_fallback_and_input_checks(tmp_path):
    import tcdiff_amd
    for name in ("load_body_model", "skin", "BodyModel"):
        assert getattr(tcdiff_amd, name) is getattr(B, name) and name in tcdiff_amd.__all__
    body = B.load_body_model(S.make_model(37, 3, seed=1), device="cpu")
    assert body._images == {}                                             # nothing was put on a device
    q, p = torch.zeros(2, 12, 24, 3), torch.zeros(2, 12, 3)
    out = torch.full((2, 12, 37, 3), 5.0)
    for call in (lambda: B.skin(body, q, p), lambda: B.skin(body, q[0].reshape(12, 72), p[0]), lambda: B.skin(body, q, p, out=out),
                 lambda: B.skin(body, q, p, pose_blend=False, origin="smpl", return_joints=True),
                 lambda: X.write_glb([str(tmp_path / "a.glb")], q, p, 3, mesh=body)):
        with pytest.raises(L.TcdiffError, match="MI355X"):
            call()
    assert (out == 5.0).all() and not (tmp_path / "a.glb").exists() and body._images == {}
    with pytest.raises(L.TcdiffError, match="MI355X"):
        body.images("cpu")
    with pytest.raises(L.TcdiffError, match="origin"):
        B.skin(body, q, p, origin="hips")
    with pytest.raises(L.TcdiffError, match="smpl_poses must be"):
        B.skin(body, torch.zeros(2, 12, 72), p)
    with pytest.raises(L.TcdiffError, match="smpl_trans must be"):
        B.skin(body, q, p[:, :11])
    with pytest.raises(L.TcdiffError, match="tensors"):
        B.skin(body, q.numpy(), p.numpy())
    with pytest.raises(L.TcdiffError, match="load_body_model"):
        B.skin(S.make_model(3, 1), q, p)
    # an output above 2^31 - 1 floats: the message names the largest n that fits (views of one pose: no memory behind them)
    lim = 2 ** 31 - 1
    body = B.load_body_model(S.make_model(100, 1, seed=1))                # 300 floats of output per pose, above A's 288
    fits = lim // 300
    for n, clips in ((fits + 1, 1), (fits // 2 + 1, 2)):
        with pytest.raises(L.TcdiffError, match=f"at most n = {lim // (300 * clips)} poses"):
            B.skin(body, torch.zeros(1, 1, 24, 3).expand(clips, n, 24, 3), torch.zeros(1, 1, 3).expand(clips, n, 3))
    with pytest.raises(L.TcdiffError, match="MI355X"):                    # the largest n that fits passes that check
        B.skin(body, torch.zeros(1, 1, 24, 3).expand(1, fits, 24, 3), torch.zeros(1, 1, 3).expand(1, fits, 3))
    one = B.load_body_model(S.make_model(1, 1, seed=1))
    with pytest.raises(L.TcdiffError, match=f"at most n = {lim // 288} poses"):      # one vertex: A's 288 floats per pose decide
        B.skin(one, torch.zeros(1, 1, 24, 3).expand(1, lim // 288 + 1, 24, 3), torch.zeros(1, 1, 3).expand(1, lim // 288 + 1, 3))
