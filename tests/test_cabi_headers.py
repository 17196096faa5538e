"""The C ABI is stated once, in include/*.h and oracle/duck_oracle.h; Python reads it (cdecl.py). The ctypes
layout of every struct against the C compiler's, the reader's behaviours on small texts, and the bindings
of libduck.so and liboracle.so against the declarations. No GPU."""

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from open_duck_playground_amd import cabi, native
from open_duck_playground_amd.cdecl import CDeclError, Header
from tests import oracle_ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = ("duck_model_desc", "duck_layout", "duck_env_config", "duck_refmotion", "duck_dr_layout",
           "duck_gather_field", "duck_mlp_problem", "duck_fleet_desc", "duck_fleet_disturbance", "oracle_data")
C_NAMES = {C.c_int: "int", C.c_uint: "unsigned", C.c_float: "float", C.c_double: "double",
           C.c_uint64: "uint64_t", C.c_int64: "int64_t", C.c_uint8: "uint8_t"}


def _layout_asserts():
    """One _Static_assert per struct size and per field offset, size and scalar type."""
    structs = oracle_ffi.HEADERS.structs
    assert sorted(structs) == sorted(STRUCTS)
    assert all(cabi.HEADERS.structs[k] is structs[k] for k in STRUCTS[:-1])
    lines, nfields = [], 0
    for name in STRUCTS:
        cls = structs[name]
        lines.append(f'_Static_assert(sizeof({name}) == {C.sizeof(cls)}, "sizeof {name}");')
        for field, typ in cls._fields_:
            f, at = getattr(cls, field), f"(({name}*)0)->{field}"
            lines.append(f'_Static_assert(offsetof({name}, {field}) == {f.offset}, "offsetof {name}.{field}");')
            lines.append(f'_Static_assert(sizeof({at}) == {f.size}, "sizeof {name}.{field}");')
            while issubclass(typ, C.Array):
                typ, at = typ._type_, at + "[0]"
            if typ in C_NAMES:
                lines.append(f'_Static_assert(_Generic({at}, {C_NAMES[typ]}: 1, default: 0), "type of {name}.{field}");')
            else:
                assert typ is C.c_void_p or issubclass(typ, C._Pointer), (name, field, typ)
            nfields += 1
    return lines, nfields


def _compiles(lines) -> subprocess.CompletedProcess:
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the headers with"
    src = '#include <stddef.h>\n#include <stdint.h>\n#include "duck.h"\n#include "duck_ppo.h"\n#include "duck_fleet.h"\n' \
          '#include "duck_oracle.h"\n' + "\n".join(lines) + "\n"
    return subprocess.run([cc, "-x", "c", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "oracle"), "-"], input=src.encode(), capture_output=True)


def test_every_struct_layout_equals_the_c_compilers():
    """sizeof, and every field's offsetof, size and scalar type, asserted at compile time (nothing is run)."""
    lines, nfields = _layout_asserts()
    assert nfields >= 300   # 94 + 43 + 61 + 14 + 8 + 5 + 17 + 21 + 5 + 32 as the headers stand
    r = _compiles(lines)
    assert r.returncode == 0, r.stderr.decode()
    # the assertions do bite: a size, an offset and a type that are wrong each fail the compilation
    size = C.sizeof(native.DuckFleetDisturbance)
    off = native.DuckFleetDisturbance.noise_scale.offset
    for good, bad in ((f"sizeof(duck_fleet_disturbance) == {size},", f"sizeof(duck_fleet_disturbance) == {size + 4},"),
                      (f"offsetof(duck_fleet_disturbance, noise_scale) == {off},",
                       f"offsetof(duck_fleet_disturbance, noise_scale) == {off + 4},"),
                      ("_Generic(((duck_env_config*)0)->n_substeps, int:",
                       "_Generic(((duck_env_config*)0)->n_substeps, float:")):
        assert sum(good in ln for ln in lines) == 1, good
        assert _compiles([ln.replace(good, bad) for ln in lines]).returncode != 0, bad


def _read(text: str) -> Header:
    return Header().read(text, "inline")


def _fields(h: Header, name: str):
    return [(k, t) for k, t in h.structs[name]._fields_]


def test_reader_reads_the_subset_the_headers_use():
    h = _read("typedef struct { int a, b; const float *p, *q; float x[2], y; } s;")
    fp = C.POINTER(C.c_float)
    assert _fields(h, "s") == [("a", C.c_int), ("b", C.c_int), ("p", fp), ("q", fp), ("x", C.c_float * 2), ("y", C.c_float)]
    h = _read("#define N 3\n#define M (N * 2u)\n#define SIZE(n) (1 + 2 * (n))\n"
              "typedef struct t { double m[N][4]; float v[SIZE(M)]; unsigned long long w; uint8_t c; } t;")
    assert h.consts == {"N": 3, "M": 6}
    assert _fields(h, "t") == [("m", C.c_double * 4 * 3), ("v", C.c_float * 13), ("w", C.c_ulonglong), ("c", C.c_uint8)]
    assert (C.sizeof(h.structs["t"]), h.structs["t"].m.size, h.structs["t"].v.offset) == (96 + 52 + 4 + 8 + 8, 96, 96)
    assert _read("enum { A = 0, B, C = 7, D, E = -2, F };").consts == {"A": 0, "B": 1, "C": 7, "D": 8, "E": -2, "F": -1}
    # a comment that holds ';' and '}', and a static inline body, are skipped
    h = _read("typedef struct { int a; /* not; a } field */ int b; // nor; this }\n } s;\n"
              "static inline int twice(int v) { int w = v; { w += v; } return w; }\nint duck_after(void);")
    assert _fields(h, "s") == [("a", C.c_int), ("b", C.c_int)] and list(h.funcs) == ["duck_after"]
    # a struct whose pointers are addresses
    h = Header(address_structs=("g",)).read("typedef struct { const float* src; int n; } g;")
    assert _fields(h, "g") == [("src", C.c_void_p), ("n", C.c_int)]


def test_reader_reads_prototypes():
    h = _read("typedef struct sim sim;\ntypedef struct { int n; } desc;\n"
              "int duck_a(const desc* d, sim* s, sim** out, const float* const* w, const uint32_t key[2], float f,\n"
              "           unsigned long long seed, int64_t off, void* stream);\n"
              "const char* duck_b(void);\nvoid duck_c(double v);\nsim* duck_d(const sim* s);\n"
              "uint64_t duck_e(unsigned* out);\ndouble duck_f(int);")
    vp = C.c_void_p
    assert h.funcs["duck_a"] == (C.c_int, [C.POINTER(h.structs["desc"]), vp, vp, vp, vp, C.c_float, C.c_ulonglong,
                                           C.c_int64, vp])
    assert h.funcs["duck_b"] == (C.c_char_p, []) and h.funcs["duck_c"] == (None, [C.c_double])
    assert h.funcs["duck_d"] == (vp, [vp]) and h.funcs["duck_e"] == (C.c_uint64, [vp])
    assert h.funcs["duck_f"] == (C.c_double, [C.c_int])
    # a second reader on top of the first shares its struct classes
    h2 = Header(base=h).read("int oracle_a(desc* d);")
    assert h2.funcs == {"oracle_a": (C.c_int, [C.POINTER(h.structs["desc"])])} and "oracle_a" not in h.funcs


@pytest.mark.parametrize("text", [
    "typedef struct { int a : 3; } s;",                         # a bit-field
    "typedef struct { union { int a; float b; } u; } s;",       # a union member
    "typedef struct { void (*f)(int); } s;",                    # a function-pointer field
    "typedef struct { real_t a; } s;",                          # an unknown type name
    "typedef struct { int a[UNKNOWN]; } s;",                    # an unknown dimension
    "int duck_a(real_t x);",                                    # an unknown parameter type
    "int duck_a(int (*f)(int));",                               # a function-pointer parameter
    "int duck_a(int x, ...);",                                  # variadic
    "typedef struct sim sim;\nint duck_a(sim s);",              # an opaque struct by value
    "typedef struct { int a; } s;\ntypedef struct { int a; } s;",   # a struct defined twice
    "extern int duck_counter;",                                 # not a prototype
    "#define NAME \"text\"\n",                                  # not an integer
    "#if X\nint duck_a(void);\n#endif\n",                       # a conditional the reader cannot follow
])
def test_reader_fails_closed(text):
    with pytest.raises(CDeclError, match="inline"):
        _read(text)


def _declared_counts(paths):
    """{function: parameter count}, counted from the header text apart from the reader."""
    out = {}
    for p in paths:
        txt = re.sub(r"/\*.*?\*/", "", open(p).read(), flags=re.S)
        for m in re.finditer(r"\b((?:duck|oracle)_\w+)\s*\(([^)]*)\)\s*;", txt):
            out[m.group(1)] = 0 if m.group(2).strip() == "void" else m.group(2).count(",") + 1
    return out


@pytest.mark.parametrize("which", ["libduck", "liboracle"])
def test_every_exported_function_is_bound_as_declared(which):
    if which == "libduck":
        H, L = cabi.HEADERS, native.lib()
        paths = [os.path.join(ROOT, "include", f) for f in sorted(os.listdir(os.path.join(ROOT, "include")))]
    else:
        H, L = oracle_ffi.HEADERS, oracle_ffi.lib()
        paths = [os.path.join(ROOT, "oracle", "duck_oracle.h")]
    counts = _declared_counts(paths)
    assert set(counts) == set(H.funcs) and len(counts) > 30
    for name, (restype, argtypes) in H.funcs.items():
        f = getattr(L, name)   # both libraries export every function their headers declare
        assert f.argtypes is not None and list(f.argtypes) == argtypes and len(argtypes) == counts[name], name
        assert f.restype is restype, name
    if which == "liboracle":
        assert len(L.oracle_standing_rewards.argtypes) == 10 and L.oracle_standing_rewards.restype is None
        assert L.oracle_model_create.restype is C.c_void_p and L.oracle_get_hf_defect.restype is C.c_double
    else:
        assert native.EXPORTS == list(H.funcs) and L.duck_build_id.restype is C.c_char_p
        assert L.duck_model_fingerprint.restype is C.c_uint64 and L.duck_destroy.restype is None


def test_model_desc_pointer_fields_keep_their_cached_types():
    """ModelDescHolder tells int* from double* fields by identity with POINTER(c_int) / POINTER(c_double)."""
    kinds = {typ for _, typ in cabi.DuckModelDesc._fields_ if issubclass(typ, C._Pointer)}
    assert kinds == {cabi._I, cabi._D}
    assert cabi.DuckModelDesc.body_parentid.size == 8 and dict(cabi.DuckModelDesc._fields_)["hull_edge"] is cabi._I
