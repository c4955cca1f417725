"""The one reader of include/stylesinger_hip.h: integer defines, enumerators, struct layouts and function prototypes are parsed
from the header (once, at import), so no Python copy of the C-ABI can drift from it. No torch import. Pointers keep what they
point to (PROTOTYPES, STRUCT_POINTEES): lib.py checks tensors against it before a launch.

The struct grammar is exactly what the header uses; anything else RAISES with the offending declaration instead of producing a
plausible `ctypes.Structure` (tests/test_host_cpu.py checks every field's offset and size against the C compiler).
"""
import collections
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


def _field(decl, defines, pointees=None):
    """One member declaration (no ';') -> [(name, ctype)], one entry per declarator; pointees[name] = the pointee of every pointer member."""
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
        if ptr and pointees is not None:
            pointees[m.group(2)] = base
    if len(pointers) > 1:
        raise HeaderError(f"declarator list mixes pointer and non-pointer members: '{decl}'")
    return fields


def parse_structs(txt, defines, pointees=None):
    """{name: [(field, ctype)]} of every `typedef struct X { ... } X;` in comment-free text; pointees[name] = {pointer member: pointee}."""
    out = {}
    for m in re.finditer(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w*)\s*;", txt, flags=re.S):
        name, body = m.group(1), m.group(2)
        pre = re.search(r"^[ \t]*#.*$", body, flags=re.M)
        if pre:
            raise HeaderError(f"preprocessor line inside struct {name}: '{pre.group(0).strip()}'")
        ptrs = {}
        fields = [f for decl in body.split(";") if decl.strip() for f in _field(" ".join(decl.split()), defines, ptrs)]
        if m.group(3) != name:   # also where a nested body's '}' ended the match early and its members were all readable
            raise HeaderError(f"struct {name}: expected '}} {name};', found '}} {m.group(3)};'")
        out[name] = fields
        if pointees is not None:
            pointees[name] = ptrs
    if len(out) != len(re.findall(r"\bstruct\b\s*\w*\s*\{", txt)):
        raise HeaderError("a struct definition that is not of the form `typedef struct X { ... } X;`")
    return out


Param = collections.namedtuple("Param", "name ctype pointee const")   # ctype: a scalar's ctypes type, None for a pointer; pointee: None for a scalar
Prototype = collections.namedtuple("Prototype", "name restype params launch text")   # launch: the last parameter is the stream

_PROTOTYPE = r"(const\s+char\s*\*|int64_t|int)\s+(ss_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;"
_PARAM_POINTEE = ("float", "double", "int32_t", "int64_t", "int16_t", "uint16_t", "uint8_t", "uint64_t", "int", "char", "void")


def parse_prototypes(txt, structs=()):
    """{name: Prototype} of every `ss_*` function declared in comment-free text; `structs` = the struct names a parameter may point to."""
    out = {}
    for m in re.finditer(_PROTOTYPE, txt, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        params = []
        for a in ([] if args in ("", "void") else args.split(",")):
            p = re.fullmatch(r"(const )?(\w+) ?(\*?) ?(\w+)?", a.strip())
            if not p or not p.group(4):
                raise HeaderError(f"{name}: parameter without a name, or not of the form `[const] type[*] name`: '{a.strip()}'")
            const, base, star, pname = p.groups()
            if star and base not in _PARAM_POINTEE and base not in structs:
                raise HeaderError(f"{name}: unknown pointee '{base}': '{a.strip()}'")
            if not star and _CTYPE.get(base) is None:
                raise HeaderError(f"{name}: unknown scalar type '{base}': '{a.strip()}'")
            params.append(Param(pname, None if star else _CTYPE[base], base if star else None, bool(const)))
        launch = bool(params) and params[-1].pointee == "void" and params[-1].name in ("stream", "stream_")
        out[name] = Prototype(name, C.c_char_p if "char" in ret else _CTYPE[ret], tuple(params), launch, f"{' '.join(ret.split())} {name}({args})")
    return out


with open(HEADER) as _fh:
    _TEXT = strip_comments(_fh.read())
DEFINES = parse_defines(_TEXT)
ENUMS = parse_enums(_TEXT)
STRUCT_POINTEES = {}   # [struct][pointer member] -> pointee
STRUCTS = parse_structs(_TEXT, DEFINES, STRUCT_POINTEES)
STRUCTURES = {name: type(name, (C.Structure,), {"_fields_": fields}) for name, fields in STRUCTS.items()}
PROTOTYPES = parse_prototypes(_TEXT, STRUCTS)


def declarations():
    """{name: (restype, [argtypes])} of PROTOTYPES: what ctypes needs (every pointer is a c_void_p)."""
    return {name: (p.restype, [C.c_void_p if a.pointee else a.ctype for a in p.params]) for name, p in PROTOTYPES.items()}


def declared_symbols():
    """Every `ss_*` function the public header declares."""
    return sorted(declarations())
