"""CPU checks of the shaded mesh frames (no GPU): the fifth header, include/tcdiff_shade.h, and its binding; the launchers'
validation; ``BodyModel.adjacency`` against a search; the numpy restatement tests/shade_ref.py on its own (outward normals, the
share of pixels it can decide); csrc/shade_math.h built for the host as a stand-alone program with the address and undefined-
behaviour sanitizers against the restatement's bytes; no CPU fallback."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import shade_ref as R
import skin_ref as S
from tcdiff_amd import _abi
from tcdiff_amd import _lib as L
from tcdiff_amd import body as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tcr_mesh_vertices", "tcr_mesh_raster"]
I, VP, LONG = C.c_int, C.c_void_p, C.c_long
VERTICES = (I, [VP, VP, VP, VP, I, I, I, VP, VP, VP, VP],
            ["const float*", "const int*", "const int*", "const int*", "int", "int", "int", "const float*", "float*", "float*", "hipStream_t"])
RASTER = (I, [VP, VP, VP, I, I, I, I, I, I, I, VP, I, VP, VP, VP, LONG, VP, VP],
          ["const float*", "const float*", "const int*", "int", "int", "int", "int", "int", "int", "int", "const unsigned char*", "int",
           "const tcr_shade_style*", "const unsigned char*", "int*", "long", "unsigned char*", "hipStream_t"])
CLEAR_SHARE = 0.98


# ---- the fifth header --------------------------------------------------------------------------------------------------------
def test_the_fifth_header_parses_to_the_two_functions_and_its_constants():
    abi = _abi.load_shade()
    assert list(abi.functions) == NAMES and abi.functions[NAMES[0]] == VERTICES and abi.functions[NAMES[1]] == RASTER
    assert L.SHADE.functions == abi.functions and L.SHADE.constants == abi.constants
    assert abi.constants == dict(TC_SHADE_TILE=32, TC_SHADE_CHUNK=256, TC_SHADE_RASTER_LAUNCHES=2, TC_SHADE_SCRATCH_PER_TRIANGLE=8,
                                 TC_SHADE_MAX_SIDE=32767)
    assert list(abi.structs) == ["tcr_shade_style"]
    fields = [(n, C.sizeof(t)) for n, t in abi.structs["tcr_shade_style"]._fields_]
    assert fields == [("background", 3), ("ambient", 4), ("light", 12)] and L.ShadeStyle is L.SHADE.structs["tcr_shade_style"]
    with open(_abi.HEADER_SHADE) as f:
        text = f.read()
    assert text.count('#include "tcdiff_hip.h"') == 1 and "frozen" in text and "unpinned" in text
    for prefix in ("tcdiff_", "tcx_", "tcs_"):
        with pytest.raises(_abi.TcdiffError, match="unknown declaration"):
            _abi.parse(text, "include/tcdiff_shade.h", prefix=prefix)


def test_the_binding_is_in_none_of_the_frozen_sets():
    for names in (L.ABI.functions, L.EXT.functions, L.GLTF.functions, L.SKIN.functions, L.EXPORTS):
        assert not any(n in names for n in NAMES) and not any(n.startswith("tcr_") for n in names)
    frozen = {**L.ABI.constants, **L.EXT.constants, **L.GLTF.constants, **L.SKIN.constants}
    assert not any(k.startswith("TC_SHADE") for k in frozen) and not any(s.startswith("tcr_") for s in {**L.ABI.structs, **L.EXT.structs})
    assert not hasattr(L, "SHADE_TILE")                                   # the constants stay in L.SHADE.constants


def _dynamic_symbols(path):
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split()}
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--dyn-syms", "-W", path], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    return {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}


def _style(ambient=0.35, light=(0.0, -0.8, 0.6)):
    st = L.ShadeStyle()
    st.background = (C.c_ubyte * 3)(255, 255, 255)
    st.ambient = ambient
    st.light = (C.c_float * 3)(*light)
    return st


def test_the_built_library_defines_the_launchers_and_they_validate_without_gpu():
    from tcdiff_amd import build
    build.build(verbose=False)
    syms = _dynamic_symbols(L.LIB_PATH)
    assert sorted(s for s in syms if s.startswith("tcr_")) == sorted(NAMES)
    assert not [s for s in syms if ("shade" in s.lower() or "mesh" in s.lower()) and s.split("_")[0] in ("tcdiff", "tcx", "tcs")]
    lib = L.load()
    assert lib.tcr_mesh_vertices.argtypes == VERTICES[1] and lib.tcr_mesh_raster.argtypes == RASTER[1]
    buf = C.create_string_buffer(256)
    p = (C.addressof(buf) + 15) & ~15                                     # aligned, never dereferenced: every call fails a check
    view = (C.c_float * 12)()
    big = 2 ** 31 - 1

    def vert(P=big, V=big, F=1, view=view, screen=p, normals=p, **null):
        ptr = {k: (None if k in null else p) for k in ("vertices", "faces", "adj_start", "adj_faces")}
        return lib.tcr_mesh_vertices(ptr["vertices"], ptr["faces"], ptr["adj_start"], ptr["adj_faces"], P, V, F, view, screen, normals, None)
    assert vert() == -4 and vert(P=1, V=1, F=big) == -4 and vert(P=2, V=big // 6 + 1) == -4       # what the good arguments end in
    for k in ("vertices", "faces", "adj_start", "adj_faces"):
        assert vert(**{k: None}) == -1, k
    assert vert(view=None) == -1 and vert(screen=None, normals=None) == -1
    assert vert(normals=None, adj_start=None, adj_faces=None) == -4 and vert(screen=None) == -4   # either output alone is allowed
    for kw in (dict(P=0), dict(P=-1), dict(V=0), dict(V=-3), dict(F=0), dict(F=-1)):
        assert vert(**kw) == -1, kw

    good = _style()

    def rast(b=65536, T=1, dn=1, V=1, F=1, W=1, H=1, n_colors=1, style=good, scratch=p, scratch_bytes=1 << 40, **null):
        ptr = {k: (None if k in null else p) for k in ("screen", "normals", "faces", "colors", "under", "frames")}
        return lib.tcr_mesh_raster(ptr["screen"], ptr["normals"], ptr["faces"], b, T, dn, V, F, W, H, ptr["colors"], n_colors,
                                   None if style is None else C.byref(style), ptr["under"], scratch, scratch_bytes, ptr["frames"], None)
    assert rast() == -4                                                   # good arguments but for the clip count
    for k in ("screen", "normals", "faces", "colors", "frames"):
        assert rast(**{k: None}) == -1, k
    assert rast(under=None) == -4 and rast(style=None) == -1 and rast(scratch=None) == -1
    for k in ("b", "T", "dn", "V", "F", "W", "H", "n_colors"):
        assert rast(**{k: 0}) == -1 and rast(**{k: -2}) == -1, k
    nan, inf = float("nan"), float("inf")
    for st in (_style(ambient=-0.1), _style(ambient=1.5), _style(ambient=nan), _style(light=(0, 0, 0)), _style(light=(1, 1, 0)),
               _style(light=(nan, 0, 1)), _style(light=(inf, 0, 0)), _style(light=(0.0, -0.8, 0.7))):
        assert rast(style=st) == -1
    assert rast(style=_style(ambient=0.0, light=(0, 0, -1))) == -4 and rast(style=_style(ambient=1.0, light=(1, 0, 0))) == -4
    for kw in (dict(b=1, T=65536), dict(b=1, W=32768), dict(b=1, H=32768), dict(b=1, V=big), dict(b=1, F=big, dn=2),
               dict(b=65535, T=65535), dict(b=1, W=32767, H=32767), dict(b=4, T=4, dn=4, V=big // 100), dict(b=3, T=5, dn=7, F=big // 100)):
        assert rast(**kw) == -4, kw
    # a scratch buffer that is too small, or off its boundary; one byte fewer than the formula is refused: 6 frames of 360
    # triangles, which are 2 chunks of 256
    need = 8 * 2 * 3 * (360 + 2)
    assert rast(b=2, T=3, dn=3, F=120, scratch_bytes=need - 1) == -1 and rast(b=2, T=3, dn=3, F=120, scratch_bytes=8 * 2 * 3 * 360) == -1
    assert rast(b=2, T=3, dn=3, F=120, scratch_bytes=0) == -1 and rast(b=1, scratch_bytes=-8) == -1
    assert rast(b=2, T=3, dn=3, F=120, scratch_bytes=need, scratch=p + 4) == -2
    from tcdiff_amd import shade
    assert shade.scratch_bytes(2, 3, 3, 120) == need and shade.scratch_bytes(1, 1, 1, 256) == 8 * 257 == shade.scratch_bytes(1, 1, 2, 128)
    assert shade.scratch_bytes(1, 2, 1, 257) == 8 * 2 * 259 and (shade.TILE, shade.CHUNK) == (32, 256)


def test_the_fifth_header_read_by_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    cc = ["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    names = sorted(L.SHADE.constants)
    src = ['#include <stdio.h>', '#include "tcdiff_shade.h"', '#include "tcdiff_shade.h"', "int main(void) {"]
    src += [f'  printf("%d\\n", {n});' for n in names] + ['  printf("%d\\n", (int)sizeof(tcr_shade_style));', "  return 0;", "}"]
    cfile, exe = tmp_path / "shade.c", tmp_path / "shade"
    cfile.write_text("\n".join(src))
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", str(cfile), "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.SHADE.constants[n] for n in names] + [C.sizeof(L.ShadeStyle)]
    calls = ['#include "tcdiff_shade.h"', "volatile int z;", "void call_every_launcher(void) {"]
    for fname, (restype, argtypes, ctexts) in L.SHADE.functions.items():
        assert restype is C.c_int and argtypes == [C.c_void_p if c.endswith("*") else _abi.SCALARS[c] for c in ctexts], fname
        calls.append(f"  {{ int (*f)({', '.join(ctexts)}) = {fname}; (void)f; }}")
        zeros = [f"({c})0" if c.endswith("*") or c == "hipStream_t" else f"({c})z" for c in ctexts]
        calls.append(f"  (void){fname}({', '.join(zeros)});")
    calls.append("}")
    tu = tmp_path / "calls.c"
    tu.write_text("\n".join(calls))
    r = subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-c", str(tu), "-o", str(tmp_path / "calls.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the adjacency ---------------------------------------------------------------------------------------------------------------
def test_adjacency_equals_a_search_and_is_cached():
    model = S.make_model(9, 2, seed=5)
    model["f"] = np.array([[0, 1, 2], [2, 1, 3], [7, 3, 2], [0, 2, 5], [5, 5, 6], [8, 0, 1]], np.uint32)       # nobody names vertex 4
    body = B.load_body_model(model)
    start, listed = body.adjacency()
    want = R.adjacency(model["f"].astype(np.int64), 9)
    assert start.dtype == np.int32 and listed.dtype == np.int32 and start.shape == (10,) and listed.shape == (18,)
    assert np.array_equal(start, want[0]) and np.array_equal(listed, want[1])
    assert start[4] == start[5] and listed[start[5]:start[6]].tolist() == [3, 4, 4]      # an empty range; a face that names 5 twice
    assert body.adjacency()[0] is start and not start.flags.writeable
    verts, faces = R.lattice(10, 7)
    big = dict(S.make_model(70, 3, seed=1), f=faces.astype(np.uint32))
    got = B.load_body_model(big).adjacency()
    want = R.adjacency(faces, 70)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the restatement on its own ---------------------------------------------------------------------------------------------------
def test_the_restatement_s_normals_point_outward_on_the_exact_lattice():
    """on the unperturbed lattice every vertex lies on a sphere, so its normal is the radial direction up to the lattice's own
    discretisation: neighbouring vertices are 2 pi / 10 and 140 / 6 degrees apart, and the boundary rings see faces on one side only"""
    verts, faces = R.lattice(10, 7, seed=None, cx=0.3)
    n = R.normals(verts[None], faces, R.adjacency(faces, 70))[0]
    radial = verts.astype(np.float64) - np.array([0.3, 0.0, 1.0])
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    cos = (n * radial).sum(1)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-15
    assert cos[10:60].min() > np.cos(np.deg2rad(5.0)) and cos.min() > np.cos(np.deg2rad(36.0)), (cos[10:60].min(), cos.min())
    lone = np.concatenate([verts, np.float32([[9, 9, 9]])])                                     # a vertex that no face names
    assert (R.normals(lone[None], faces, R.adjacency(faces, 71))[0, 70] == 0).all()


@pytest.mark.parametrize("name", R.CASES)
def test_the_restatement_decides_nearly_every_pixel(name):
    """what the GPU test asserts before it touches the GPU: clear pixels are at least 98 % of those inside any triangle's grown box"""
    c = R.case(name)
    if name == "crowded":
        assert len(c["faces"]) == R.CROWD > 2 * L.SHADE.constants["TC_SHADE_CHUNK"]
        xy = c["screen"][0, 0, :, :2]
        assert xy.min() >= 32 and xy.max() < 64                          # every box inside the one tile (1, 1)
    for clip, t, m, d in R.frames_of(name):
        share = R.clear_share(m, d)
        print(f"[shade] {name} clip {clip} frame {t}: deltas {d[0]:.1e} px, {d[1]:.1e} depth, {d[2]:.1e} levels; clear share {share:.4f} "
              f"of {int(m['boxed'].sum())} pixels, {int((m['winner'] >= 0).sum())} covered")
        assert share >= CLEAR_SHARE, (name, clip, t, share)
    if name == "wild":
        m = R.frames_of(name)[0][2]
        assert set(np.unique(m["winner"])) == {0, 10}                     # the oversized triangle and the one in front of it
    if name == "equal-depth":
        m = R.frames_of(name)[0][2]
        assert m["winner"].max() == 1 and (m["zgap"][m["winner"] >= 0] == 0).all()      # dancer 0 shows, dancer 1 ties everywhere


# ---- csrc/shade_math.h on the host, under the sanitizers --------------------------------------------------------------------------
def test_shade_math_on_the_host_under_the_sanitizers_reproduces_the_restatement(tmp_path):
    """the SAME arithmetic the HIP kernels compile, as a stand-alone program built with -fsanitize=address,undefined"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "shade_host")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tcdiff_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "shade_host.cpp")])
    for name in ("33x17", "wild"):
        c = R.case(name)
        st = dict(R.STYLE, **c["style"])
        for clip, t, m, d in R.frames_of(name)[:2]:
            rows = slice(t * c["dn"], (t + 1) * c["dn"])
            with open(tmp_path / "in.bin", "wb") as f:
                f.write(np.array([c["dn"], c["screen"].shape[2], len(c["faces"]), c["W"], c["H"], len(c["colors"]), c["under"] is not None],
                                 np.int32).tobytes())
                f.write(np.array([st["ambient"], *st["light"]], np.float32).tobytes() + bytes(st["background"]) + b"\0")
                f.write(c["screen"][clip, rows].tobytes() + c["normals"][clip, rows].tobytes() + c["faces"].tobytes())
                f.write(np.array(c["colors"], np.uint8).tobytes() + (b"" if c["under"] is None else c["under"][clip, t].tobytes()))
            r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(c["H"], c["W"], 3)
            assert np.array_equal(got, R.to_bytes(m["values"])), (name, clip, t)         # float64 both sides, the same order: equal bytes
            R.check(got, m, d, (name, clip, t))


# ---- no CPU fallback ----------------------------------------------------------------------------------------------------------------
def test_no_cpu_fallback_and_argument_refusals_before_the_gpu():
    from tcdiff_amd import shade
    import tcdiff_amd
    assert tcdiff_amd.draw_bodies is shade.draw_bodies and tcdiff_amd.vertex_normals is shade.vertex_normals
    assert tcdiff_amd.draw_body_samples is shade.draw_body_samples
    body = B.load_body_model(S.make_model(7, 2, seed=1))
    v = torch.zeros(1, 6, 7, 3)
    for fn in (lambda: shade.vertex_normals(body, v), lambda: shade.draw_bodies(body, v, 3)):
        with pytest.raises(L.TcdiffError, match="MI355X only"):
            fn()
    with pytest.raises(L.TcdiffError, match="load_body_model"):
        shade.draw_bodies(object(), v, 3)
    with pytest.raises(L.TcdiffError, match="vertices must be"):
        shade.draw_bodies(body, torch.zeros(1, 6, 8, 3), 3)
    with pytest.raises(L.TcdiffError, match="float32"):
        shade.vertex_normals(body, v.double())
    with pytest.raises(L.TcdiffError, match="ambient"):
        shade.make_shade_style(ambient=1.5)
    with pytest.raises(L.TcdiffError, match="light"):
        shade.make_shade_style(light=(0, 0, 0))
    st = shade.make_shade_style(light=(0, 3, 4), ambient=0.25, background=(1, 2, 3))
    assert list(st.light) == [0.0, np.float32(0.6), np.float32(0.8)] and st.ambient == 0.25 and list(st.background) == [1, 2, 3]
