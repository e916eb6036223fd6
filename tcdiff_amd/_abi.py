"""The C ABI of libtcdiff_gfx950.so, read from include/tcdiff_hip.h: its integer macros, structs and prototypes as ctypes.
include/tcdiff_hip_ext.h, the launchers added since the first header was pinned, is read the same way (load_ext), and so is
include/tcdiff_gltf.h, whose function carries the prefix tcx_ (load_gltf), include/tcdiff_skin.h, prefix tcs_ (load_skin), include/tcdiff_shade.h,
prefix tcr_ (load_shade), include/tcdiff_mjpeg.h, prefix tcj_ (load_mjpeg), include/tcdiff_footlock.h, prefix tck_ (load_footlock), include/tcdiff_group.h, prefix tcg_ (load_group),
include/tcdiff_apart.h, prefix tcp_ (load_apart), include/tcdiff_ground.h, prefix tcf_ (load_ground), include/tcdiff_meshcontact.h, prefix
tcm_ (load_meshcontact), include/tcdiff_selfcontact.h, prefix tci_ (load_selfcontact), include/tcdiff_smooth.h, prefix tcw_
(load_smooth), include/tcdiff_choreo.h, prefix tcc_ (load_choreo), and include/tcdiff_beatsync.h, prefix tcb_ (load_beatsync).

The headers are the one place where the ABI is written down; _lib.py binds the library from what parse() returns.  The parser
knows the C that the header uses and nothing more, and it never guesses: a declaration it does not recognise raises
TcdiffError with the header line.  Imports neither torch nor the library.
"""
import ctypes as C
import os
import re
from collections import namedtuple

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tcdiff_hip.h")
HEADER_EXT = os.path.join(os.path.dirname(HEADER), "tcdiff_hip_ext.h")
HEADER_GLTF = os.path.join(os.path.dirname(HEADER), "tcdiff_gltf.h")
HEADER_SKIN = os.path.join(os.path.dirname(HEADER), "tcdiff_skin.h")
HEADER_SHADE = os.path.join(os.path.dirname(HEADER), "tcdiff_shade.h")
HEADER_MJPEG = os.path.join(os.path.dirname(HEADER), "tcdiff_mjpeg.h")
HEADER_FOOTLOCK = os.path.join(os.path.dirname(HEADER), "tcdiff_footlock.h")
HEADER_GROUP = os.path.join(os.path.dirname(HEADER), "tcdiff_group.h")
HEADER_APART = os.path.join(os.path.dirname(HEADER), "tcdiff_apart.h")
HEADER_GROUND = os.path.join(os.path.dirname(HEADER), "tcdiff_ground.h")
HEADER_MESHCONTACT = os.path.join(os.path.dirname(HEADER), "tcdiff_meshcontact.h")
HEADER_SELFCONTACT = os.path.join(os.path.dirname(HEADER), "tcdiff_selfcontact.h")
HEADER_SMOOTH = os.path.join(os.path.dirname(HEADER), "tcdiff_smooth.h")
HEADER_CHOREO = os.path.join(os.path.dirname(HEADER), "tcdiff_choreo.h")
HEADER_BEATSYNC = os.path.join(os.path.dirname(HEADER), "tcdiff_beatsync.h")


class TcdiffError(RuntimeError):
    pass


SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "uint32_t": C.c_uint32,
           "uint64_t": C.c_uint64, "unsigned char": C.c_ubyte, "unsigned": C.c_uint, "hipStream_t": C.c_void_p}

# constants {macro: int}; structs {C name: ctypes.Structure class}; functions {name: (restype, argtypes, the parameters' C types)}
Abi = namedtuple("Abi", "constants structs functions")

_INT = r"0[xX][0-9a-fA-F]+|0|[1-9]\d*"
_PREPROCESSOR = re.compile(r"^[ \t]*#[^\n]*", re.M)
_DEFINE = re.compile(r"[ \t]*#[ \t]*define[ \t]+(\w+)(\(?)(.*)")
_DECLARATOR = re.compile(r"\s*(\**)\s*(\w*)\s*((?:\[\s*\w*\s*\]\s*)*)")
_STRUCT = re.compile(r"\s*typedef\s+struct\s*\w*\s*\{(.*)\}\s*(\w+)\s*", re.S)
_FUNCTION = r"\s*(int|const\s+char\s*\*)\s*(%s\w+)\s*\((.*)\)\s*"          # % the functions' prefix
_STREAM = re.compile(r"\s*typedef\s+struct\s+\w+\s*\*\s*hipStream_t\s*")


def _blank(m):
    """what replaces a match that is dropped: a blank and the match's line ends, so that every later offset stays on its line"""
    return " " + "\n" * m.group().count("\n")


def parse(text: str, name: str = "include/tcdiff_hip.h", prefix: str = "tcdiff_") -> Abi:
    """``prefix``: what a function's name must start with; a prototype of another name is an unknown declaration"""
    a_function = re.compile(_FUNCTION % re.escape(prefix), re.S)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", _blank, text, flags=re.S)
    constants, structs, functions = {}, {}, {}
    types = dict(SCALARS, void=None)          # C type -> ctypes type; the structs join as they are declared

    def type_re():
        return re.compile(r"\s*(const\s+)?(" + "|".join(sorted(types, key=len, reverse=True)) + r")\b")
    a_type = type_re()

    def fail(pos, what, decl):
        pos += len(text[pos:]) - len(text[pos:].lstrip())
        raise TcdiffError(f"{name}:{text.count(chr(10), 0, pos) + 1}: {what}: {' '.join(decl.split())!r}")

    def integer(expr, pos, decl):
        toks = [str(constants.get(t, t)) for t in re.findall(_INT + r"|[-+*()]|[^\s+*()-]+", expr)]
        bad = [t for t in toks if not re.fullmatch(_INT + r"|[-+*()]", t)]
        if bad or not toks:
            fail(pos, f"{bad[0] if bad else 'nothing'!r} where an integer expression of literals, ( ) + - * is expected", decl)
        try:
            return int(eval(" ".join(toks), {"__builtins__": {}}))
        except (SyntaxError, TypeError):
            fail(pos, "malformed integer expression", decl)

    def declarators(decl, pos):
        """'const float* a, *b[3]' -> (ctypes type, C type, name, dimensions) of a and of b; an unsized dimension is None"""
        t = a_type.match(decl)
        if not t:
            fail(pos, f"unknown type {' '.join(decl.split()[:2])!r}", decl)
        base, out = types[t.group(2)], []
        for d in decl[t.end():].split(","):
            m = _DECLARATOR.fullmatch(d)
            if not m or (base is None and not m.group(1)):
                fail(pos, f"unknown declarator {d.strip()!r}", decl)
            dims = [integer(n, pos, decl) if n else None for n in re.findall(r"\[\s*(\w*)\s*\]", m.group(3))]
            out.append((C.c_void_p if m.group(1) else base, ("const " if t.group(1) else "") + t.group(2) + m.group(1), m.group(2), dims))
        return out

    def struct(body, cname, pos):
        fields = []
        for m in re.finditer(r"[^;]*[^;\s][^;]*", body):
            for ctype, _, ident, dims in declarators(m.group(), pos + m.start()):
                if not ident or None in dims:
                    fail(pos + m.start(), "a field needs a name and sized dimensions", m.group())
                for n in reversed(dims):
                    ctype = ctype * n
                fields.append((ident, ctype))
        nonlocal a_type
        structs[cname] = types[cname] = type(cname, (C.Structure,), {"_fields_": fields})
        a_type = type_re()

    def function(ret, fname, params, pos, decl):
        args = []
        for p in [] if params.strip() == "void" else params.split(","):
            if "(" in p:
                fail(pos, f"unknown parameter {p.strip()!r}", decl)
            (ctype, ctext, _, dims), = declarators(p, pos)
            args.append((C.c_void_p, ctext + "*") if dims else (ctype, ctext))      # an array parameter is a pointer
        functions[fname] = (C.c_int if ret == "int" else C.c_char_p, [a for a, _ in args], [c for _, c in args])

    # preprocessor lines: the object-like TC_* macros are the constants, everything else is skipped
    for m in _PREPROCESSOR.finditer(text):
        d = _DEFINE.fullmatch(m.group())
        if d and d.group(1).startswith("TC_") and not d.group(2):
            constants[d.group(1)] = integer(d.group(3), m.start(), m.group())
    text = _PREPROCESSOR.sub(_blank, text)
    text, externs = re.subn(r'extern\s+"C"\s*\{', _blank, text)

    # declarations: a statement ends at a ';' outside braces
    depth, start = 0, 0
    for m in re.finditer(r"[{};]", text):
        if m.group() == "{":
            depth += 1
        elif m.group() == "}" and depth == 0 and externs and not text[start:m.start()].strip():
            externs, start = externs - 1, m.end()          # the end of an extern "C" block
        elif m.group() == "}":
            depth -= 1
            if depth < 0:
                fail(m.start(), "unbalanced braces", text[start:m.end()])
        elif depth == 0:
            decl, pos, start = text[start:m.start()], start, m.end()
            s, f = _STRUCT.fullmatch(decl), a_function.fullmatch(decl)
            if s:
                struct(s.group(1), s.group(2), pos + s.start(1))
            elif f:
                function(f.group(1), f.group(2), f.group(3), pos, decl)
            elif not _STREAM.fullmatch(decl):
                fail(pos, "unknown declaration", decl)
    if depth or text[start:].strip():
        fail(start, "unterminated declaration", text[start:][:200])
    return Abi(constants, structs, functions)


def load() -> Abi:
    with open(HEADER) as f:
        return parse(f.read())


def load_ext() -> Abi:
    """the second header's own declarations; its #include of the first is a preprocessor line and is skipped"""
    with open(HEADER_EXT) as f:
        return parse(f.read(), "include/tcdiff_hip_ext.h")


def load_gltf() -> Abi:
    """the third header: one launcher, named tcx_* because the set of tcdiff_* symbols is frozen (the header says why)"""
    with open(HEADER_GLTF) as f:
        return parse(f.read(), "include/tcdiff_gltf.h", prefix="tcx_")


def load_skin() -> Abi:
    """the fourth header: one launcher, tcs_skin_vertices, and its tile sizes as constants; tcs_* because tcdiff_* and tcx_* are frozen"""
    with open(HEADER_SKIN) as f:
        return parse(f.read(), "include/tcdiff_skin.h", prefix="tcs_")


def load_shade() -> Abi:
    """the fifth header: the mesh rasteriser's two launchers, tcr_mesh_vertices and tcr_mesh_raster, its style struct and its tile
    and chunk sizes as constants; tcr_* because tcdiff_*, tcx_* and tcs_* are frozen"""
    with open(HEADER_SHADE) as f:
        return parse(f.read(), "include/tcdiff_shade.h", prefix="tcr_")


def load_mjpeg() -> Abi:
    """the sixth header: the Motion-JPEG encoder's three launchers, tcj_mjpeg_workspace, tcj_mjpeg_plan and tcj_mjpeg_write, and its
    constants; tcj_* because tcdiff_*, tcx_*, tcs_* and tcr_* are frozen"""
    with open(HEADER_MJPEG) as f:
        return parse(f.read(), "include/tcdiff_mjpeg.h", prefix="tcj_")


def load_footlock() -> Abi:
    """the seventh header: the foot lock's two functions, tck_foot_lock_workspace and tck_foot_lock, and its constants; tck_* because
    tcdiff_*, tcx_*, tcs_*, tcr_* and tcj_* are frozen"""
    with open(HEADER_FOOTLOCK) as f:
        return parse(f.read(), "include/tcdiff_footlock.h", prefix="tck_")


def load_group() -> Abi:
    """the eighth header: the group metrics' two functions, tcg_group_workspace and tcg_group_metrics, and its constants; tcg_* because
    tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_* and tck_* are frozen"""
    with open(HEADER_GROUP) as f:
        return parse(f.read(), "include/tcdiff_group.h", prefix="tcg_")


def load_apart() -> Abi:
    """the ninth header: keeping the dancers apart, tcp_keep_apart_workspace and tcp_keep_apart, and its constants; tcp_* because
    tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_* and tcg_* are frozen"""
    with open(HEADER_APART) as f:
        return parse(f.read(), "include/tcdiff_apart.h", prefix="tcp_")


def load_ground() -> Abi:
    """the tenth header: putting the dancers on the floor, tcf_ground_workspace, tcf_ground_metrics and tcf_ground, and its constants;
    tcf_* because tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_* and tcp_* are frozen"""
    with open(HEADER_GROUND) as f:
        return parse(f.read(), "include/tcdiff_ground.h", prefix="tcf_")


def load_meshcontact() -> Abi:
    """the eleventh header: mesh-level contact between the skinned bodies, tcm_mesh_contact_workspace and tcm_mesh_contact, and its
    constants; tcm_* because tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_* and tcf_* are frozen"""
    with open(HEADER_MESHCONTACT) as f:
        return parse(f.read(), "include/tcdiff_meshcontact.h", prefix="tcm_")


def load_selfcontact() -> Abi:
    """the twelfth header: a dancer's contact with itself, tci_self_contact_workspace and tci_self_contact, and its constants; tci_*
    because tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_*, tcf_* and tcm_* are frozen"""
    with open(HEADER_SELFCONTACT) as f:
        return parse(f.read(), "include/tcdiff_selfcontact.h", prefix="tci_")


def load_smooth() -> Abi:
    """the thirteenth header: the jitter scores and the rotation filter, tcw_smoothness, tcw_smooth_workspace and tcw_smooth, and its
    constants; tcw_* because tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_*, tcf_*, tcm_* and tci_* are frozen"""
    with open(HEADER_SMOOTH) as f:
        return parse(f.read(), "include/tcdiff_smooth.h", prefix="tcw_")


def load_choreo() -> Abi:
    """the fourteenth header: the choreography planner and its closing check, tcc_plan and tcc_trajectory_error, and its constants;
    tcc_* because tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_*, tcf_*, tcm_*, tci_* and tcw_* are frozen"""
    with open(HEADER_CHOREO) as f:
        return parse(f.read(), "include/tcdiff_choreo.h", prefix="tcc_")


def load_beatsync() -> Abi:
    """the fifteenth header: the kinematic beats and the time warp onto the music's, tcb_motion_beats, tcb_beat_sync and
    tcb_beat_sync_workspace, and its constants; tcb_* because tcdiff_*, tcx_*, tcs_*, tcr_*, tcj_*, tck_*, tcg_*, tcp_*, tcf_*, tcm_*,
    tci_*, tcw_* and tcc_* are frozen"""
    with open(HEADER_BEATSYNC) as f:
        return parse(f.read(), "include/tcdiff_beatsync.h", prefix="tcb_")
