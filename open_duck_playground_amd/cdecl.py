"""Reader of the C ABI headers (``include/*.h``, ``oracle/duck_oracle.h``): the headers are the one
statement of every struct, constant and call; ``native.py``, ``cabi.py`` and ``tests/oracle_ffi.py``
build their ctypes classes and bindings from what this module reads.

It reads the subset of C the headers use -- integer ``#define``s (plain and function-like), anonymous
enums, ``typedef struct`` of scalars, fixed arrays and pointers, opaque struct typedefs, prototypes --
and raises ``CDeclError`` on anything else rather than skipping it. Comments, ``#ifdef __cplusplus``
blocks and the bodies of ``static inline`` functions are dropped.

Types: a struct is a ``ctypes.Structure``; a pointer field is ``POINTER(scalar)``, or ``c_void_p`` in
the structs named in ``address_structs`` (their pointers are device addresses, which callers hold as
integers). In a prototype a pointer to a struct is ``POINTER(struct)`` and every other pointer is
``c_void_p``, which takes integers, ``byref``, ctypes arrays and pointers, and ``None``.
"""

from __future__ import annotations

import ctypes as C
import re

SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "float": C.c_float, "double": C.c_double,
           "char": C.c_char, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
           "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "uint16_t": C.c_uint16,
           "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
_WORDS = {"const", "void"} | {w for k in SCALARS for w in k.split()}
_SUFFIX = re.compile(r"\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]+\b")   # 16u, 0xF1EEu
_WORD = re.compile(r"\s*(\w+)")
_DECLARATOR = re.compile(r"((?:\*|const\b|\s)*)(\w*)\s*((?:\[[^\]]*\]\s*)*)$")
_DIRECTIVES = ("include", "ifndef", "endif", "define")


class CDeclError(ValueError):
    pass


def _split(text: str, sep: str) -> list:
    """``text`` cut at every ``sep`` outside (), [] and {}."""
    out, depth, start = [], 0, 0
    for i, c in enumerate(text):
        depth += (c in "([{") - (c in ")]}")
        if c == sep and depth == 0:
            out.append(text[start:i])
            start = i + 1
    return [s.strip() for s in out + [text[start:]]]


class Header:
    def __init__(self, *paths: str, address_structs=(), base: "Header" = None):
        """Reads ``paths`` in order. ``base``: a reader whose constants and types these headers build on
        (the same struct classes, so the two readers' bindings take each other's instances)."""
        self.consts, self.macros, self.structs, self.opaque, self.funcs = {}, {}, {}, set(), {}
        if base is not None:
            self.consts, self.macros = dict(base.consts), dict(base.macros)
            self.structs, self.opaque = dict(base.structs), set(base.opaque)
        self._address_structs = set(address_structs)
        for path in paths:
            with open(path) as f:
                self.read(f.read(), path)

    def _fail(self, what: str, text: str):
        raise CDeclError(f"{self._where}: {what}: {' '.join(text.split())!r}")

    def value(self, expr: str) -> int:
        """An integer expression over the constants and macros read so far."""
        env, nothing = dict(self.consts), {"__builtins__": {}}
        env.update({k: eval(f"lambda {a}: {b}", nothing, env) for k, (a, b) in self.macros.items()})
        try:
            v = eval(_SUFFIX.sub(r"\1", expr).replace("/", "//"), nothing, env)
            assert isinstance(v, int)
        except Exception:
            self._fail("not an integer expression", expr)
        return v

    def read(self, text: str, where: str = "<text>") -> "Header":
        self._where = where
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        text = re.sub(r"^[ \t]*#[ \t]*ifdef __cplusplus\b.*?^[ \t]*#[ \t]*endif\b", " ", text, flags=re.S | re.M)
        for line in re.findall(r"^[ \t]*#[ \t]*(.*)$", text, re.M):
            m = re.match(r"define\s+(\w+)(\(([\w\s,]*)\))?(.*)$", line)
            if m and m.group(2):
                self.macros[m.group(1)] = (m.group(3), m.group(4).replace("/", "//"))
                self.value(f"{m.group(1)}({','.join('1' for _ in m.group(3).split(','))})")
            elif m and m.group(4).strip():
                self.consts[m.group(1)] = self.value(m.group(4))
            elif not line.startswith(_DIRECTIVES):
                self._fail("unsupported directive", "#" + line)
        text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
        depth = start = 0
        for i, c in enumerate(text):   # top-level statements end at ';', a function body at its '}'
            depth += (c == "{") - (c == "}")
            if depth == 0 and (c == ";" or c == "}" and text[start:i].lstrip().startswith("static inline")):
                if c == ";" and text[start:i].strip():
                    self._statement(" ".join(text[start:i].split()))
                start = i + 1
        if depth or text[start:].strip():
            self._fail("unterminated declaration", text[start:][:80])
        return self

    def _statement(self, s: str):
        if m := re.fullmatch(r"enum\s*\w*\s*\{(.*)\}", s):
            v = -1
            for item in filter(None, _split(m.group(1), ",")):
                name, eq, expr = item.partition("=")
                v = self.value(expr) if eq else v + 1
                self.consts[name.strip()] = v
        elif m := re.fullmatch(r"typedef struct (\w+) (\w+)", s):
            self.opaque.add(m.group(2))
        elif m := re.fullmatch(r"typedef struct\s*\w*\s*\{(.*)\}\s*(\w+)", s):
            fields = []
            for decl in filter(None, _split(m.group(1), ";")):
                base, rest = self._base(decl)
                for d in _split(rest, ","):
                    name, ptr, dims = self._declarator(d, decl)
                    if not name or base == "void" and not ptr:
                        self._fail("unsupported field", decl)
                    ty = self.structs.get(base) or SCALARS.get(base)
                    if ptr:
                        void = ptr > 1 or ty is None or m.group(2) in self._address_structs
                        ty = C.c_void_p if void else C.POINTER(ty)
                    elif ty is None:
                        self._fail("an opaque struct by value", decl)
                    for n in reversed(dims):
                        ty = ty * n
                    fields.append((name, ty))
            if m.group(2) in self.structs:
                self._fail("a struct defined twice", m.group(2))
            self.structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        elif m := re.fullmatch(r"(.*?)(\w+)\s*\((.*)\)", s):
            params = [] if m.group(3).strip() == "void" else [self._ctype(p) for p in _split(m.group(3), ",")]
            if None in params:
                self._fail("a void parameter", s)
            self.funcs[m.group(2)] = (self._ctype(m.group(1), ret=True), params)
        else:
            self._fail("unsupported declaration", s)

    def _base(self, decl: str):
        """(type name without qualifiers, the declarators after it)."""
        words, pos = [], 0
        while (m := _WORD.match(decl, pos)) and m.group(1) in _WORDS | self.structs.keys() | self.opaque:
            words.append(m.group(1))
            pos = m.end()
        base = " ".join(w for w in words if w != "const")
        if base != "void" and base not in SCALARS and base not in self.structs and base not in self.opaque:
            self._fail("unknown type", decl)
        return base, decl[pos:]

    def _declarator(self, d: str, decl: str):
        """(name, pointer depth, array dimensions) of one declarator."""
        m = _DECLARATOR.fullmatch(d.strip())
        if not m or m.group(2) in _WORDS:
            self._fail("unsupported declarator", decl)
        return m.group(2), m.group(1).count("*"), [self.value(x) for x in re.findall(r"\[([^\]]*)\]", m.group(3))]

    def _ctype(self, decl: str, ret: bool = False):
        """The ctypes type of a parameter, or of a return type (None for void)."""
        base, rest = self._base(decl)
        _, ptr, dims = self._declarator(rest, decl)
        ptr += bool(dims)   # an array parameter is a pointer
        if ptr:
            if ptr == 1 and base in self.structs:
                return C.POINTER(self.structs[base])
            return C.c_char_p if ret and ptr == 1 and base == "char" else C.c_void_p
        if base in self.opaque:
            self._fail("an opaque struct by value", decl)
        return None if base == "void" else self.structs.get(base) or SCALARS[base]

    def bind(self, lib) -> None:
        """Set ``argtypes`` and ``restype`` of every declared function that ``lib`` exports."""
        for name, (restype, argtypes) in self.funcs.items():
            if hasattr(lib, name):
                f = getattr(lib, name)
                f.restype, f.argtypes = restype, argtypes
