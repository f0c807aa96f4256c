"""Parser of include/fi_mi355.h: the C ABI as ctypes structures, prototypes and constants.

The header is the one place that knows the ABI; ``_lib`` binds whatever this module reads from it.  The parser is a
few regular expressions over the comment-stripped text and knows only the forms the header uses:
``typedef struct tag { ... } name_t;``, ``FI_API <ret> fi_xxx(<params>);``, ``#define FI_NAME <literal>`` and enums
whose enumerators all carry explicit values.  Anything else is refused with a HeaderError that names it: a
declaration that is skipped would surface as a shifted pointer inside a kernel.
"""
from __future__ import annotations

import ctypes as C
import keyword
import re
from typing import Dict, List, NamedTuple, Tuple


class HeaderError(ImportError):
    """The header holds something this parser does not read."""


class Abi(NamedTuple):
    structs: Dict[str, type]                       # typedef name -> ctypes.Structure subclass, in header order
    prototypes: Dict[str, Tuple[type, List[type]]]  # symbol -> (restype, argtypes), in header order
    constants: Dict[str, object]                   # every FI_ #define and every enumerator -> int | float


_SCALARS = {
    "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
    "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "fi_stream_t": C.c_void_p,
}
_POINTEES = set(_SCALARS) - {"fi_stream_t"} | {"void", "char", "uint8_t", "uint16_t"}

_INT = re.compile(r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)(?:ll|LL)?$")
_FLOAT = re.compile(r"([-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?)[fF]?$")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(FI_\w+)[ \t]+(\S.*?)[ \t]*$", re.M)
_ENUM = re.compile(r"\benum\s+\w+\s*\{([^{}]*)\}\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"FI_API\s+([\w\s*]+?)\b(fi_\w+)\s*\(([^()]*)\)\s*;")
_DECL = re.compile(r"(\w+)\s*(\**)\s*(\w+(?:\s*,\s*\w+)*)$")


def _literal(text: str, what: str):
    text = text.strip()
    if text.startswith("(") and text.endswith(")"):
        text = text[1:-1].strip()
    if _INT.match(text):
        return int(text.rstrip("lL"), 0)
    m = _FLOAT.match(text)
    if m:
        return float(m.group(1))
    raise HeaderError(f"{what}: {text!r} is not an integer or float literal")


def _ctype(base: str, stars: str, structs: Dict[str, type], decl: str, is_return: bool = False):
    if not stars:
        if base in _SCALARS:
            return _SCALARS[base]
        if base in structs:
            return structs[base]
    elif stars == "*":
        if base in structs:
            return C.POINTER(structs[base])
        if base == "int64_t":
            return C.POINTER(C.c_int64)
        if base in _POINTEES:
            return C.c_char_p if is_return and base == "char" else C.c_void_p
    raise HeaderError(f"unknown type {base + stars!r} in declaration {decl!r}")


def _declaration(decl: str, structs: Dict[str, type]):
    """'const int64_t a, b' -> (c_int64, ['a', 'b'])"""
    m = _DECL.match(re.sub(r"\bconst\b", " ", decl).strip())
    if not m:
        raise HeaderError(f"cannot read declaration {decl!r}")
    base, stars, names = m.groups()
    return _ctype(base, stars, structs, decl), [n.strip() for n in names.split(",")]


def _each(pattern: "re.Pattern[str]", opener: str, text: str):
    """Match ``pattern`` at every occurrence of ``opener``; an occurrence it does not match is refused, so the
    number of parsed declarations always equals the number of openers in the text."""
    for start in re.finditer(opener, text):
        m = pattern.match(text, start.start())
        if not m:
            raise HeaderError(f"cannot read the declaration starting at {text[start.start():start.start() + 80]!r}")
        yield m


def _add(table: dict, name: str, value) -> None:
    if name in table:
        raise HeaderError(f"{name} is declared twice")
    table[name] = value


def parse(text: str) -> Abi:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)

    constants: Dict[str, object] = {}
    for name, value in _DEFINE.findall(text):
        if name != "FI_API":  # the export attribute, not a constant
            _add(constants, name, _literal(value, f"#define {name}"))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    for m in _each(_ENUM, r"\benum\b", text):
        for item in filter(None, (i.strip() for i in m.group(1).split(","))):
            name, eq, value = item.partition("=")
            if not eq:
                raise HeaderError(f"enumerator {item!r} has no explicit value")
            _add(constants, name.strip(), _literal(value, f"enumerator {name.strip()}"))

    structs: Dict[str, type] = {}
    for m in _each(_STRUCT, r"\btypedef\s+struct\b", text):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            ctype, names = _declaration(decl, structs)
            fields += [(n + "_" if keyword.iskeyword(n) else n, ctype) for n in names]
        _add(structs, m.group(2), type(m.group(2), (C.Structure,), {"_fields_": fields}))

    prototypes: Dict[str, Tuple[type, List[type]]] = {}
    for m in _each(_PROTO, r"\bFI_API\b", text):
        ret, name, params = m.groups()
        rm = re.match(r"(\w+)\s*(\**)$", re.sub(r"\bconst\b", " ", ret).strip())
        if not rm:
            raise HeaderError(f"cannot read the return type {ret!r} of {name}")
        restype = _ctype(rm.group(1), rm.group(2), structs, f"{ret.strip()} {name}(...)", is_return=True)
        params = [] if params.strip() == "void" else params.split(",")
        _add(prototypes, name, (restype, [_declaration(decl, structs)[0] for decl in params]))
    return Abi(structs, prototypes, constants)
