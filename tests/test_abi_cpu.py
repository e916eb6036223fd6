"""The header parser behind the ctypes binding (tcdiff_amd/_abi.py) on literal header fragments: no library, no GPU."""
import ctypes as C

import pytest

from tcdiff_amd import _abi

VP, I = C.c_void_p, C.c_int


def test_prototype_over_three_lines_with_a_comment_full_of_punctuation():
    abi = _abi.parse("""
        /* out[i] = f(a, b); see g(x, y); (and more), ; ( */
        int tcdiff_demo(int dtype, const void* A,   // a line comment, with ( and ;
                        long n, float w, double s,
                        uint32_t thr, hipStream_t stream);
    """)
    assert abi.functions == {"tcdiff_demo": (I, [I, VP, C.c_long, C.c_float, C.c_double, C.c_uint32, VP],
                                             ["int", "const void*", "long", "float", "double", "uint32_t", "hipStream_t"])}


def test_array_parameter_const_unsigned_char_pointer_and_uint64():
    abi = _abi.parse("int tcdiff_a(const float view[12], const unsigned char* keep, uint64_t seed, unsigned char c, void *Kc);\n"
                     "const char* tcdiff_version(void);")
    assert abi.functions["tcdiff_a"] == (I, [VP, VP, C.c_uint64, C.c_ubyte, VP],
                                         ["const float*", "const unsigned char*", "uint64_t", "unsigned char", "void*"])
    assert abi.functions["tcdiff_version"] == (C.c_char_p, [], [])


def test_struct_declarators_arrays_and_a_macro_sized_array_of_structs():
    abi = _abi.parse("""
        #define TC_MAX_PROB (2 * 4)
        typedef struct { const void* A; float* out; int M, N; } tcdiff_problem;
        typedef struct tcdiff_group {
            int n_prob, kc;                 /* several declarators */
            void* out2; int ldc2;           /* several declarations on a line */
            void *Kc, *Vc;
            unsigned char rgb[3], grid[2][3];
            unsigned seed; long n;
            tcdiff_problem p[TC_MAX_PROB];
        } tcdiff_group;
        int tcdiff_run(const tcdiff_group* g, tcdiff_problem* one);
    """)
    prob, group = abi.structs["tcdiff_problem"], abi.structs["tcdiff_group"]
    assert prob._fields_ == [("A", VP), ("out", VP), ("M", I), ("N", I)]
    assert [n for n, _ in group._fields_] == ["n_prob", "kc", "out2", "ldc2", "Kc", "Vc", "rgb", "grid", "seed", "n", "p"]
    f = dict(group._fields_)
    assert (f["out2"], f["Vc"], f["seed"], f["n"]) == (VP, VP, C.c_uint, C.c_long)
    assert f["rgb"] is C.c_ubyte * 3 and f["grid"] is (C.c_ubyte * 3) * 2 and f["p"] is prob * 8
    assert C.sizeof(group) == 8 + 16 + 16 + 9 + 3 + 4 + 8 + 8 * C.sizeof(prob) and group.p.offset == 64
    assert abi.functions["tcdiff_run"] == (I, [VP, VP], ["const tcdiff_group*", "tcdiff_problem*"])


def test_macros_arithmetic_is_evaluated_and_function_like_macros_are_skipped():
    abi = _abi.parse("""
        #ifndef TCDIFF_HIP_H
        #define TCDIFF_HIP_H
        #define TCDIFF_ERR_ARG (-1)
        #define TC_A 0x100 /* hexadecimal */
        #define TC_TABLE (480 * 480 - 1)
        #define TC_SUM (TC_TABLE + 2 * (3 + TC_A))
        #define TC_ERR_NOCONVERGE (-5)
        #define TC_SITE_ENC(i, k) (4 * (i) + (k))
        #define TC_G_DEC(L) ((long)(L) * 198272)
        #endif
    """)
    assert abi.constants == {"TC_A": 256, "TC_TABLE": 230399, "TC_SUM": 230399 + 2 * 259, "TC_ERR_NOCONVERGE": -5}


@pytest.mark.parametrize("text, named", [
    ("\n\nint tcdiff_a(int n, size_t bytes);", "size_t"),                              # an unknown type
    ("int tcdiff_a(long long n);", "long n"),
    ("int tcdiff_a(void (*callback)(int));", "callback"),
    ("typedef struct { int a; int64_t b; } tcdiff_s;", "int64_t"),
    ("typedef struct { int a : 3; } tcdiff_s;", "a : 3"),
    ("typedef struct { union { int a; float b; } u; } tcdiff_s;", "union"),
    ("typedef struct { int a[TC_UNKNOWN]; } tcdiff_s;", "TC_UNKNOWN"),
    ("typedef struct { void v; } tcdiff_s;", "v"),
    ("#define TC_HALF (1 / 2)", "/"),
    ("#define TC_MASK (1 << 4)", "<<"),
    ("#define TC_SCALE 0.5f", ".5f"),
    ("#define TC_EMPTY", "nothing"),
    ("float tcdiff_ratio(int n);", "tcdiff_ratio"),
    ("static const int tcdiff_table_size = 4;", "tcdiff_table_size"),
    ("int tcdiff_a(int n)", "unterminated"),
])
def test_what_the_parser_does_not_know_raises_and_is_named(text, named):
    with pytest.raises(_abi.TcdiffError) as e:
        _abi.parse(text, "fragment.h")
    assert named in str(e.value) and str(e.value).startswith("fragment.h:")


def test_the_error_names_the_line_of_the_declaration():
    with pytest.raises(_abi.TcdiffError, match=r"^fragment\.h:4: unknown type 'size_t bytes'"):
        _abi.parse("/* a comment\n   of two lines */\nint tcdiff_ok(int n);\nint tcdiff_a(int n,\n  size_t bytes);", "fragment.h")
    with pytest.raises(_abi.TcdiffError, match=r"^fragment\.h:3: unknown type 'short b'"):
        _abi.parse("typedef struct {\n  int a;\n  short b;\n} tcdiff_s;", "fragment.h")


def test_the_header_itself_parses_to_the_whole_abi():
    abi = _abi.load()
    assert len(abi.structs) == 17 and len(abi.functions) == 79
    assert all(restype is I for name, (restype, _, _) in abi.functions.items() if name != "tcdiff_version")
    assert not any(name.startswith(("TC_SITE_ENC", "TC_NAV_G_DEC", "TCDIFF_")) for name in abi.constants)
