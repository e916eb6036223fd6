"""CPU checks of the glTF export (no GPU): the third header, include/tcdiff_gltf.h, and its binding; the launcher's validation;
csrc/gltf_math.h built for the host against the numpy restatement tests/gltf_ref.py; ``build_glb`` on the restatement's blocks,
read back by the reader of tests/gltf_ref.py and evaluated against float64 forward kinematics; the host side of
tcdiff_amd/gltf.py (names, shapes, no CPU fallback)."""
import ctypes as C
import inspect
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gltf_ref as G
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd import draw as D
from tcdiff_amd import export as E
from tcdiff_amd import gltf as X
from tcdiff_amd.fk import SMPL_OFFSETS, SMPL_PARENTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tcx_gltf_animation"
I, VP = C.c_int, C.c_void_p
ARGTYPES = [VP, VP, I, I, I, C.c_double, VP, VP]
CTYPES = ["const float*", "const float*", "int", "int", "int", "double", "float*", "hipStream_t"]


# ---- the third header ---------------------------------------------------------------------------------------------------------------
def test_the_third_header_parses_to_the_one_function():
    abi = _abi.load_gltf()
    assert abi.structs == {} and abi.constants == {} and list(abi.functions) == [NAME]          # TC_GLTF_FLOATS(T, dn) is skipped
    assert abi.functions[NAME] == (I, ARGTYPES, CTYPES)
    assert L.GLTF.functions == abi.functions
    with open(_abi.HEADER_GLTF) as f:
        text = f.read()
    assert text.count('#include "tcdiff_hip.h"') == 1 and "TC_GLTF_FLOATS(T, dn)" in text and "frozen" in text
    with pytest.raises(_abi.TcdiffError, match="unknown declaration"):                          # the default prefix is tcdiff_
        _abi.parse(text, "include/tcdiff_gltf.h")
    with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
        _abi.parse("int tcdiff_f(int a);", "x.h", prefix="tcx_")
    assert list(_abi.parse("int tcdiff_f(int a);", "x.h").functions) == ["tcdiff_f"]
    assert list(_abi.parse("int tcy_f(void);", "x.h", prefix="tcy_").functions) == ["tcy_f"]
    with pytest.raises(_abi.TcdiffError, match="unknown declaration"):                          # the prefix is text, not a pattern
        _abi.parse("int tcyyf(void);", "x.h", prefix="tc.y")


def test_the_frozen_symbol_sets_are_untouched():
    assert len(L.ABI.functions) == 79 and list(L.EXT.functions) == ["tcdiff_geometric_features"] and len(L.EXPORTS) == 80
    assert L.EXPORTS == sorted(list(L.ABI.functions) + list(L.EXT.functions))
    for names in (L.ABI.functions, L.EXT.functions, L.EXPORTS):
        assert NAME not in names
    assert not any(k.startswith("TC_GLTF") for k in {**L.ABI.constants, **L.EXT.constants})


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
    assert NAME in syms and [s for s in syms if s.startswith("tcx_")] == [NAME]
    lib = L.load()
    assert lib.tcx_gltf_animation.argtypes == ARGTYPES and lib.tcx_gltf_animation.restype is I
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)

    def go(poses=p, trans=p, clips=1, T=1, dn=1, fps=30.0, out=p):
        return lib.tcx_gltf_animation(poses, trans, clips, T, dn, fps, out, None)
    assert go(poses=None) == -1 and go(trans=None) == -1 and go(out=None) == -1
    assert go(clips=0) == -1 and go(T=0) == -1 and go(dn=0) == -1 and go(clips=-3) == -1 and go(T=-1) == -1 and go(dn=-1) == -1
    for fps in (0.0, -30.0, float("nan"), float("inf"), float("-inf")):
        assert go(fps=fps) == -1
    big = 2 ** 31 - 1
    assert go(T=big, dn=big) == -4 and go(clips=big, T=big, dn=big) == -4
    assert go(T=big) == -4 and go(clips=big) == -4 and go(dn=big) == -4                         # F alone is at least 100
    dn = big // 6 // 99 + 1                                       # the first dn with 2 * 3 * (1 + 99 dn) above 2^31 - 1
    assert 2 * G.floats(3, dn - 1) <= big < 2 * G.floats(3, dn) and go(clips=2, T=3, dn=dn) == -4
    assert go(poses=None, T=big, dn=big) == -1                     # the argument checks come first


def test_the_third_header_read_by_the_c_compiler(tmp_path):
    """what tests/test_geometric_cpu.py does for the second header: the macro's value, and a translation unit that calls the
    launcher with every argument cast to its parsed C type and assigns it to a function pointer of the parsed signature"""
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    cases = [(1, 1), (150, 3), (1125, 2), (2 ** 31 - 1, 1), (3, 2 ** 31 - 1)]            # int arguments, a long result
    src = ['#include <stdio.h>', '#include "tcdiff_gltf.h"', "int main(void) {"]
    src += [f'  printf("%ld\\n", TC_GLTF_FLOATS({T}, {dn}));' for T, dn in cases] + ["  return 0;", "}"]
    cfile, exe = tmp_path / "gltf.c", tmp_path / "gltf"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [X.block_floats(T, dn) for T, dn in cases] == [G.floats(T, dn) for T, dn in cases]
    calls = ['#include "tcdiff_gltf.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.GLTF.functions.items():
        assert restype is C.c_int and argtypes == [C.c_void_p if c.endswith("*") else _abi.SCALARS[c] for c in ctexts], fname
        calls.append(f"  {{ int (*f)({', '.join(ctexts)}) = {fname}; (void)f; }}")
        zeros = [f"({c})0" if c.endswith("*") or c == "hipStream_t" else f"({c})z" for c in ctexts]
        calls.append(f"  (void){fname}({', '.join(zeros)});")
    calls.append("}")
    tu = tmp_path / "calls.c"
    tu.write_text("\n".join(calls))
    r = subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-c", str(tu), "-o", str(tmp_path / "calls.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the restatement's own inputs, and csrc/gltf_math.h on the host ------------------------------------------------------------------
def test_the_seeded_dance_flips_and_no_decision_is_a_near_tie():
    poses, trans, out, info = G.seeded(1, 150, 3)
    print(f"T = 150, 3 dancers: {info['flips']} flips, smallest |dot| or |w_0| {info['margin']:.4f}")
    assert info["flips"] >= 72 and info["margin"] > G.MIN_MARGIN          # every channel turns through pi at least once
    _, _, rot = G.split(out[0], 150, 3)
    assert (rot[:, :, 0, 3] < 0).sum() == 0                               # w_0 >= 0 in every channel ...
    q = rot.astype(np.float64)
    assert ((q[:, :, 1:] * q[:, :, :-1]).sum(-1) > 0.99).all()            # ... and neighbours on one side of the sphere
    assert (rot[..., 3] < 0).any()                                        # which a per-frame w >= 0 would not give
    for shape in G.GPU_SHAPES:
        assert G.seeded(*shape)[3]["margin"] > G.MIN_MARGIN


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    so = str(tmp_path_factory.mktemp("gltf_host") / "gltf_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "host", "gltf_host.cpp")])
    lib = C.CDLL(so)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def run(poses, trans, fps=30.0):
        clips, T, dn = poses.shape[:3]
        poses, trans = np.ascontiguousarray(poses, np.float32), np.ascontiguousarray(trans, np.float32)
        out = np.full((clips, G.floats(T, dn)), 7.0, np.float32)
        lib.host_gltf_block(vp(poses), vp(trans), C.c_int(clips), C.c_int(T), C.c_int(dn), C.c_double(fps), vp(out))
        return out

    def flips(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return lib.host_gltf_flips(vp(a), vp(b))
    return run, flips


def test_gltf_math_on_the_host_against_the_restatement(host):
    """the SAME source the HIP kernel compiles, built with g++ without contraction"""
    run, flips = host
    for shape in [(1, 1, 1), (1, 2, 1), (2, 7, 3), (1, 150, 3)]:
        poses, trans, want, _ = G.seeded(*shape)
        G.compare(run(poses, trans), want, shape[1], shape[2], f"host {shape}")
    poses, trans, want, _ = G.seeded(2, 7, 3)
    other, _ = G.block(poses, trans, 29.97)
    assert not np.array_equal(other[:, :7], want[:, :7])
    G.compare(run(poses, trans, 29.97), other, 7, 3, "host 29.97 fps")
    # a dot product of exactly 0 does not flip, nor one of -0, nor a NaN; the rotation vectors cannot reach these
    assert flips([1, 0, 0, 0], [0, 0, 0, 1]) == 0 and flips([0, 1, 0, 0], [0, 0, -1, 0]) == 0 and flips([0, 0, 0, 1], [0, 0, 0, -0.0]) == 0
    assert flips([0, 0, 0, 1], [0, 0, 0, -1]) == 1 and flips([0, 0, 0, 1], [0, 0, 0, 1]) == 0
    assert flips([0.5, 0.5, 0.5, 0.5], [-0.5, -0.5, -0.5, 0.5 + 1e-12]) == 1 and flips([0.5, 0.5, 0.5, 0.5], [-0.5, -0.5, 0.5, 0.5]) == 0
    assert flips([np.nan, 0, 0, 1], [0, 0, 0, -1]) == 0 and flips([0, 0, 0, 1], [0, 0, 0, np.nan]) == 0


def test_the_special_cases_on_the_host(host):
    run, _ = host
    poses, trans, want, _ = G.crafted()
    G.check_crafted(want)
    got = run(poses, trans)
    G.compare(got, want, 130, 1, "host crafted")
    G.check_crafted(got)


# ---- build_glb ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,dn", [(1, 1), (2, 1), (7, 3), (150, 3)])
def test_build_glb_reads_back_and_its_joints_are_forward_kinematics(T, dn):
    poses, trans, out, _ = G.seeded(1, T, dn)
    data = X.build_glb(out[0], T, dn, 30.0)
    assert isinstance(data, bytes) and data == X.build_glb(out[0].copy(), T, dn, 30.0)
    gltf, binary = G.read_glb(data)
    assert binary[:4 * G.floats(T, dn)] == out[0].tobytes()               # the device-made block as it is, at the head
    assert all(v["byteOffset"] % 4 == 0 for v in gltf["bufferViews"]) and all(a["byteOffset"] % 4 == 0 for a in gltf["accessors"])
    anim, = gltf["animations"]
    assert len(anim["channels"]) == len(anim["samplers"]) == 25 * dn and {s["interpolation"] for s in anim["samplers"]} == {"LINEAR"}
    time, = {s["input"] for s in anim["samplers"]}
    a = gltf["accessors"][time]
    assert a["type"] == "SCALAR" and a["componentType"] == 5126 and a["count"] == T
    assert a["min"] == [0.0] and a["max"] == [float(np.float32((T - 1) / 30.0))]
    paths = [(c["target"]["node"], c["target"]["path"]) for c in anim["channels"]]
    assert sorted(paths) == sorted([(24 * d, "translation") for d in range(dn)] + [(24 * d + j, "rotation") for d in range(dn) for j in range(24)])
    for d in range(dn):
        for j in range(24):
            node = gltf["nodes"][24 * d + j]
            assert node["name"] == f"d{d}_{X.JOINT_NAMES[j]}"
            assert node.get("children", []) == [24 * d + k for k in range(24) if SMPL_PARENTS[k] == j]
            assert ("translation" not in node) if j == 0 else (node["translation"] == [float(v) for v in SMPL_OFFSETS[j]])
    world, times = G.evaluate(gltf, binary)
    assert np.array_equal(times, out[0][:T])
    got = G.joints_of(gltf, world, dn, X.JOINT_NAMES)
    want = G.to_y_up(G.fk(poses[0], trans[0], SMPL_OFFSETS))
    err = float(np.abs(got - want).max())
    print(f"T = {T}, {dn} dancer(s): evaluated joints against float64 FK, largest error {err:.3e} m (bound 1e-5)")
    assert got.shape == (dn, T, 24, 3) and err <= 1e-5
    assert float(np.abs(G.joints_of(gltf, world, dn, X.JOINT_NAMES)[:, :, 0] - G.to_y_up(trans[0].transpose(1, 0, 2))).max()) == 0


def test_the_body_is_one_rigidly_skinned_solid_per_bone():
    T, dn = 2, 3
    poses, trans, _, _ = G.seeded(1, T, 1)
    out3, _ = G.block(np.repeat(poses, dn, 2), np.repeat(trans, dn, 2))
    gltf, binary = G.read_glb(X.build_glb(out3[0], T, dn, 30.0))
    assert len(gltf["meshes"]) == len(gltf["skins"]) == len(gltf["materials"]) == dn
    prim0 = gltf["meshes"][0]["primitives"][0]
    rest = np.zeros((24, 3))
    for j in range(1, 24):
        rest[j] = rest[SMPL_PARENTS[j]] + SMPL_OFFSETS[j]
    for d in range(dn):
        prim, = gltf["meshes"][d]["primitives"]
        assert prim["attributes"] == prim0["attributes"] and prim["indices"] == prim0["indices"] and prim["material"] == d   # shared
        skin = gltf["skins"][d]
        assert skin["joints"] == list(range(24 * d, 24 * d + 24))
        ibm = G.accessor(gltf, binary, skin["inverseBindMatrices"]).astype(np.float64)
        assert gltf["accessors"][skin["inverseBindMatrices"]]["type"] == "MAT4" and ibm.shape == (24, 16)
        for j in range(24):
            bind = np.eye(4)
            bind[:3, 3] = rest[j]                                         # the joint's rest transform: translations only
            assert np.abs(ibm[j].reshape(4, 4).T @ bind - np.eye(4)).max() < 1e-6            # column-major
        body = [n for n in gltf["nodes"] if n.get("mesh") == d]
        assert len(body) == 1 and body[0]["skin"] == d and gltf["nodes"].index(body[0]) in gltf["scenes"][0]["nodes"]
        rgb = gltf["materials"][d]["pbrMetallicRoughness"]["baseColorFactor"]
        c = np.asarray(D.PALETTE[d % len(D.PALETTE)]) / 255.0
        lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
        assert rgb[3] == 1.0 and np.abs(np.asarray(rgb[:3]) - lin).max() < 1e-12
    assert gltf["materials"][0]["pbrMetallicRoughness"]["baseColorFactor"][:3] == pytest.approx(
        [((v / 255 + 0.055) / 1.055) ** 2.4 for v in (0xE3, 0xBA, 0x8F)], abs=1e-12)      # the first palette colour, linear
    at = {k: G.accessor(gltf, binary, v) for k, v in prim0["attributes"].items()}
    idx = G.accessor(gltf, binary, prim0["indices"])
    V = len(at["POSITION"])
    assert gltf["accessors"][prim0["indices"]]["componentType"] == 5123 and idx.max() < V and len(idx) % 3 == 0
    assert V == 23 * 8 * 3 and sorted(idx.tolist()) == list(range(V))     # 23 bones, 8 faces, unshared vertices
    assert gltf["accessors"][prim0["attributes"]["JOINTS_0"]]["componentType"] == 5121
    assert at["JOINTS_0"].shape == (V, 4) and at["JOINTS_0"].max() < 24 and np.array_equal(at["WEIGHTS_0"].sum(1), np.ones(V, np.float32))
    assert np.array_equal(at["WEIGHTS_0"][:, 0], np.ones(V, np.float32)) and (at["JOINTS_0"][:, 1:] == 0).all()
    assert np.abs(np.sqrt((at["NORMAL"].astype(np.float64) ** 2).sum(1)) - 1).max() < 1e-6
    P, N = at["POSITION"].astype(np.float64)[idx].reshape(-1, 3, 3), at["NORMAL"].astype(np.float64)[idx].reshape(-1, 3, 3)
    face = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    face /= np.sqrt((face * face).sum(-1, keepdims=True))
    assert np.abs(N - face[:, None]).max() < 1e-5                         # flat shading: the winding's own normal, on all three
    bones = [j for j in range(24) if SMPL_PARENTS[j] >= 0]
    for b, j in enumerate(bones):                                         # bone b: from the parent's rest position to the child's
        p = SMPL_PARENTS[j]
        tri, skinned = P[8 * b:8 * b + 8], at["JOINTS_0"][idx][24 * b:24 * b + 24, 0]
        assert (skinned == p).all()
        assert np.abs(tri[:4, 0] - rest[p]).max() < 1e-6 and np.abs(tri[4:, 0] - rest[j]).max() < 1e-6
        centre = (rest[p] + rest[j]) / 2
        assert ((face[8 * b:8 * b + 8] * (tri.mean(1) - centre)).sum(-1) > 0).all()            # the normals point outwards


def test_without_a_body_there_is_only_the_armature_and_a_bad_block_raises():
    _, _, out, _ = G.seeded(1, 7, 3)
    gltf, binary = G.read_glb(X.build_glb(out[0], 7, 3, 30.0, body=False))
    for key in ("meshes", "skins", "materials"):
        assert key not in gltf
    assert len(gltf["nodes"]) == 72 and gltf["scenes"][0]["nodes"] == [0, 24, 48] and len(binary) == 4 * G.floats(7, 3)
    assert len(gltf["bufferViews"]) == 1 and len(gltf["accessors"]) == 1 + 25 * 3
    world, _ = G.evaluate(gltf, binary)
    with_body, _ = G.evaluate(*G.read_glb(X.build_glb(out[0], 7, 3, 30.0)))
    assert all(np.array_equal(world[n], with_body[n]) for n in world)
    one = X.build_glb(out[0], 7, 3, 30.0, colors=[(255, 0, 0)])
    assert G.read_glb(one)[0]["materials"][2]["pbrMetallicRoughness"]["baseColorFactor"] == [1.0, 0.0, 0.0, 1.0]
    for bad in (np.nan, np.inf, -np.inf):
        for where in (0, 6, 7 + 21, -1):
            blk = out[0].copy()
            blk[where] = bad
            with pytest.raises(L.TcdiffError, match="non-finite"):
                X.build_glb(blk, 7, 3, 30.0)
    with pytest.raises(L.TcdiffError, match="floats"):
        X.build_glb(out[0][:-1], 7, 3, 30.0)
    with pytest.raises(L.TcdiffError, match="floats"):
        X.build_glb(out[0], 7, 2, 30.0)
    with pytest.raises(L.TcdiffError):
        X.build_glb(out[0], 0, 3, 30.0)
    with pytest.raises(L.TcdiffError, match="colors"):
        X.build_glb(out[0], 7, 3, 30.0, colors=[(256, 0, 0)])


def test_a_custom_skeleton_is_written_and_evaluated():
    poses, trans, out, _ = G.seeded(1, 7, 3)
    g = np.random.default_rng(3)
    offsets = np.asarray(SMPL_OFFSETS) * g.uniform(0.5, 1.5, (24, 1))
    gltf, binary = G.read_glb(X.build_glb(out[0], 7, 3, 30.0, parents=SMPL_PARENTS, offsets=offsets))
    got = G.joints_of(gltf, G.evaluate(gltf, binary)[0], 3, X.JOINT_NAMES)
    assert float(np.abs(got - G.to_y_up(G.fk(poses[0], trans[0], offsets))).max()) <= 1e-5


# ---- the host side --------------------------------------------------------------------------------------------------------------------
def test_file_names_render_sample_would_write():
    names = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]
    for mode, epoch, name in (("normal", 7, names), ("ctrl", 7, names[:1]), ("inpaint", "e", names),
                              ("long", 3, ["data/test/features/gLH_sBM_c01_d16_mLH2_ch04_slice0.npy"])):
        pkl = E.fk_out_names(mode, epoch, name)
        assert X.glb_out_names(mode, epoch, name) == [n[:-4] + ".glb" for n in pkl] and all(n.endswith(".pkl") for n in pkl)
    assert X.glb_out_names("normal", 7, names)[0] == "7_0_gBR_sBM_c01_d04_mBR0_ch01_slice3.glb"
    assert X.glb_out_names("long", 3, ["data/test/features/gLH_sBM_c01_d16_mLH2_ch04_slice0.npy"]) == ["3_gLH_sBM_c01_d16_mLH2_ch04.glb"]
    with pytest.raises(L.TcdiffError):
        X.glb_out_names("normal", 1, None)


def test_no_cpu_fallback_and_input_checks(tmp_path):
    q, p = torch.zeros(2, 12, 24, 3), torch.zeros(2, 12, 3)
    for call in (lambda: X.animation_block(q, p, 3), lambda: X.animation_block(q[0].reshape(12, 72), p[0], 3),
                 lambda: X.write_glb([str(tmp_path / "a.glb"), str(tmp_path / "b.glb")], q, p, 3),
                 lambda: X.write_glb_out(str(tmp_path / "out"), "normal", 1, ["a/b.npy", "a/c.npy"], q, p, 3)):
        with pytest.raises(L.TcdiffError, match="MI355X"):
            call()
    assert not (tmp_path / "a.glb").exists() and os.listdir(tmp_path / "out") == []
    with pytest.raises(L.TcdiffError, match="whole number"):
        X.animation_block(q, p, 5)
    with pytest.raises(L.TcdiffError, match="whole number"):
        X.animation_block(q, p, 0)
    with pytest.raises(L.TcdiffError, match="smpl_poses must be"):
        X.animation_block(torch.zeros(2, 12, 72), p, 3)
    with pytest.raises(L.TcdiffError, match="smpl_poses must be"):
        X.animation_block(torch.zeros(12, 24, 3), p[0], 3)
    with pytest.raises(L.TcdiffError, match="smpl_trans must be"):
        X.animation_block(q, p[:, :11], 3)
    with pytest.raises(L.TcdiffError, match="smpl_trans must be"):
        X.animation_block(q[0].reshape(12, 72), p, 3)
    with pytest.raises(L.TcdiffError, match="tensors"):
        X.animation_block(q.numpy(), p.numpy(), 3)
    for fps in (0, -30, float("nan"), float("inf")):
        with pytest.raises(L.TcdiffError, match="fps"):
            X.animation_block(q, p, 3, fps=fps)


def test_convert_fk_out_reads_the_pickles_shapes(tmp_path, monkeypatch):
    """the launch itself needs the GPU (tests/test_gltf_gpu.py); here the pickle's handling, with the GPU taken out of sight"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    poses, trans, _, _ = G.seeded(1, 7, 3)
    q, p = torch.from_numpy(poses.reshape(1, 21, 24, 3).copy()), torch.from_numpy(trans.reshape(1, 21, 3).copy())
    path, = E.write_fk_out(str(tmp_path), "normal", 1, ["a/b.npy"], q, p, torch.zeros(1, 3, 7, 24, 3))
    with pytest.raises(L.TcdiffError, match="MI355X"):                     # the shapes pass; no CPU fallback
        X.convert_fk_out(path)
    assert os.listdir(tmp_path) == [os.path.basename(path)]

    def dump(name, **d):
        with open(tmp_path / name, "wb") as f:
            pickle.dump(d, f)
        return str(tmp_path / name)
    good = dict(smpl_poses=np.zeros((21, 72), np.float32), smpl_trans=np.zeros((21, 3), np.float32), full_pose=np.zeros((3, 7, 24, 3)))
    with pytest.raises(L.TcdiffError, match="MI355X"):
        X.convert_fk_out(dump("good.pkl", **good), str(tmp_path / "x.glb"))
    for bad in (dict(good, full_pose=np.zeros((2, 7, 24, 3))), dict(good, smpl_trans=np.zeros((20, 3))),
                dict(good, smpl_poses=np.zeros((21, 24, 3))), dict(good, smpl_poses=np.zeros((0, 72)), smpl_trans=np.zeros((0, 3)))):
        with pytest.raises(L.TcdiffError, match="are not"):
            X.convert_fk_out(dump("bad.pkl", **bad))
    with pytest.raises(L.TcdiffError, match="holds no"):
        X.convert_fk_out(dump("bad.pkl", smpl_poses=good["smpl_poses"], smpl_trans=good["smpl_trans"]))
    assert not (tmp_path / "x.glb").exists()


def test_render_sample_takes_glb_out_and_the_package_exports_the_names():
    import tcdiff_amd
    sig = inspect.signature(tcdiff_amd.GaussianDiffusion.render_sample)
    names = list(sig.parameters)
    assert sig.parameters["glb_out"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["glb_out"].default is None
    assert names[-2:] == ["glb_out", "draw_out"] and sig.parameters["draw_out"].kind is inspect.Parameter.KEYWORD_ONLY
    assert names[:-2] == ["self", "shape", "cond", "normalizer", "epoch", "render_out", "fk_out", "name", "sound", "mode", "noise",
                          "constraint", "sound_folder", "start_point", "render", "required_dancer_num", "x_0", "render_len"]
    assert all(sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:-2])
    for name in ("animation_block", "build_glb", "write_glb", "write_glb_out", "convert_fk_out"):
        assert getattr(tcdiff_amd, name) is getattr(X, name) and name in tcdiff_amd.__all__
    assert len(X.JOINT_NAMES) == 24 == len(set(X.JOINT_NAMES)) and X.JOINT_NAMES[0] == "m_avg_Pelvis"
