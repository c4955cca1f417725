"""The one reader of include/stylesinger_hip.h: integer defines, enumerators, struct layouts and function prototypes are parsed
from the header (once, at import), so no Python copy of the C-ABI can drift from it. No torch import.

The struct grammar is exactly what the header uses; anything else RAISES with the offending declaration instead of producing a
plausible `ctypes.Structure` (tests/test_host_cpu.py checks every field's offset and size against the C compiler).
"""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stylesinger_hip.h")

_VALUE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_POINTEE = set(_VALUE) | {"void", "uint16_t"}   # what a `type*` member may point to; every pointer is a c_void_p
_CTYPE = dict(_VALUE, int=C.c_int, void=None)   # scalars of the function prototypes


class HeaderError(ValueError):
    pass


def strip_comments(txt):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", txt, flags=re.S))


def parse_defines(txt):
    """{name: value} of every `#define SS_<NAME> <integer>`."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(SS_\w+)[ \t]+(-?\d+)[ \t]*$", txt, flags=re.M)}


def parse_enums(txt):
    """{name: value} of every enumerator of the `enum { NAME = int, ... };` blocks; an enumerator without an explicit value is refused."""
    out = {}
    for body in re.findall(r"\benum\s*\w*\s*\{(.*?)\}", txt, flags=re.S):
        for item in filter(None, (" ".join(i.split()) for i in body.split(","))):
            m = re.fullmatch(r"(\w+) ?= ?(-?\d+)", item)
            if not m:
                raise HeaderError(f"enumerator without an explicit integer value: '{item}'")
            out[m.group(1)] = int(m.group(2))
    return out


def _field(decl, defines):
    """One member declaration (no ';') -> [(name, ctype)], one entry per declarator."""
    if ":" in decl:
        raise HeaderError(f"bit-field: '{decl}'")
    if re.search(r"\b(struct|union)\b|[{}]", decl):
        raise HeaderError(f"nested struct or union: '{decl}'")
    m = re.fullmatch(r"(?:const )?(\w+) ?(\*?) ?(.*)", decl)
    base, star, rest = m.groups() if m else (None, "", "")
    if base not in _POINTEE:
        raise HeaderError(f"unknown base type '{base}': '{decl}'")
    fields, pointers = [], set()
    for i, d in enumerate(rest.split(",")):
        m = re.fullmatch(r"(\*?) ?(\w+) ?((?: ?\[ ?\w+ ?\]){0,3})", d.strip())
        if not m:
            raise HeaderError(f"cannot read declarator '{d.strip()}': '{decl}'")
        ptr = bool(m.group(1)) or (i == 0 and bool(star))
        if ptr and i == 0 and star and m.group(1):
            raise HeaderError(f"pointer to pointer: '{decl}'")
        pointers.add(ptr)
        if not ptr and base not in _VALUE:
            raise HeaderError(f"unknown base type '{base}': '{decl}'")
        t = C.c_void_p if ptr else _VALUE[base]
        for n in reversed(re.findall(r"\w+", m.group(3))):   # the first bracket is the outermost dimension
            if not n.isdigit() and n not in defines:
                raise HeaderError(f"dimension '{n}' is neither a literal nor a known define: '{decl}'")
            t = t * (int(n) if n.isdigit() else defines[n])
        fields.append((m.group(2), t))
    if len(pointers) > 1:
        raise HeaderError(f"declarator list mixes pointer and non-pointer members: '{decl}'")
    return fields


def parse_structs(txt, defines):
    """{name: [(field, ctype)]} of every `typedef struct X { ... } X;` in comment-free text."""
    out = {}
    for m in re.finditer(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w*)\s*;", txt, flags=re.S):
        name, body = m.group(1), m.group(2)
        pre = re.search(r"^[ \t]*#.*$", body, flags=re.M)
        if pre:
            raise HeaderError(f"preprocessor line inside struct {name}: '{pre.group(0).strip()}'")
        fields = [f for decl in body.split(";") if decl.strip() for f in _field(" ".join(decl.split()), defines)]
        if m.group(3) != name:   # also where a nested body's '}' ended the match early and its members were all readable
            raise HeaderError(f"struct {name}: expected '}} {name};', found '}} {m.group(3)};'")
        out[name] = fields
    if len(out) != len(re.findall(r"\bstruct\b\s*\w*\s*\{", txt)):
        raise HeaderError("a struct definition that is not of the form `typedef struct X { ... } X;`")
    return out


with open(HEADER) as _fh:
    _TEXT = strip_comments(_fh.read())
DEFINES = parse_defines(_TEXT)
ENUMS = parse_enums(_TEXT)
STRUCTS = parse_structs(_TEXT, DEFINES)
STRUCTURES = {name: type(name, (C.Structure,), {"_fields_": fields}) for name, fields in STRUCTS.items()}


def declarations():
    """{name: (restype, [argtypes])} parsed from the public header, so the binding cannot drift from it."""
    out = {}
    for m in re.finditer(r"(const\s+char\s*\*|int64_t|int)\s+(ss_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", _TEXT, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        restype = C.c_char_p if "char" in ret else _CTYPE[ret]
        argtypes = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    argtypes.append(C.c_void_p)
                else:
                    base = [t for t in a.replace("const", " ").split() if t in _CTYPE]
                    assert base, f"cannot parse parameter '{a}' of {name}"
                    argtypes.append(_CTYPE[base[0]])
        out[name] = (restype, argtypes)
    return out


def declared_symbols():
    """Every `ss_*` function the public header declares."""
    return sorted(declarations())
