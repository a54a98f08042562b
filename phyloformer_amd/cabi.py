"""The C ABI as ``include/phyloformer_amd.h`` states it: prototypes, constants and which functions a library may lack.

The header is the one description of an entry point; :mod:`engine` and :mod:`hostio` take their ctypes prototypes and
status codes from here.  A type outside ``SCALARS``, ``void`` and pointers raises at import.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, NamedTuple, Tuple

from .build import INCLUDE

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t}


class Prototype(NamedTuple):
    restype: object          # a ctypes type, or None for void
    argtypes: list
    call_time: bool          # under a banner "(additive to ABI n)": a library of this ABI version may lack it
    text: str                # the prototype as the header writes it, on one line


def _ctype(decl: str, proto: str, param: bool):
    """One C type (a parameter with or without its name, or a return type) as ctypes."""
    tokens = [t for t in re.findall(r"\w+|\*", decl) if t != "const"]
    words = [t for t in tokens if t != "*"]
    stars = len(tokens) - len(words)
    if param and len(words) == 2:
        words.pop()          # the parameter's name
    if len(words) != 1:
        raise TypeError(f"cannot read the type '{decl.strip()}' of {proto}")
    if stars:                # const char* / char*: bytes in, bytes out; any other pointer is an address
        return C.c_char_p if (words[0], stars) == ("char", 1) else C.c_void_p
    if words[0] == "void" and not param:
        return None
    if words[0] not in SCALARS:
        raise TypeError(f"no ctypes type for '{decl.strip()}' in {proto}")
    return SCALARS[words[0]]


def _comment(m) -> str:
    """What a comment leaves in the code: nothing, or - a section banner - a line that says whether it carries the marker."""
    text = m.group(0)
    return "\f%d\n" % ("(additive to ABI" in text.split("\n")[0]) if text.startswith("/* ----") else " "


def parse(text: str) -> Tuple[Dict[str, Prototype], Dict[str, int]]:
    """``(prototypes by name, constants by name)`` of a header's text: every ``pf_*`` prototype (return type and name on
    one line), and the integer ``#define PF_*`` and ``PF_* = n`` enumerators."""
    code = re.sub(r"/\*.*?\*/|//[^\n]*", _comment, text, flags=re.S)
    protos, call_time = {}, False
    for m in re.finditer(r"^\f([01])$|^([\w \t*]+?)\b(pf_\w+)\s*\(([^()]*)\)\s*;", code, re.M):
        if m.group(1):
            call_time = m.group(1) == "1"
            continue
        proto = " ".join(m.group(0).split())
        args = [] if m.group(4).strip() in ("", "void") else m.group(4).split(",")
        protos[m.group(3)] = Prototype(_ctype(m.group(2), proto, False), [_ctype(a, proto, True) for a in args], call_time, proto)
    consts = {}
    for a, b, c, d in re.findall(r"^#define\s+(PF_\w+)\s+\(?(-?\d+)\)?\s*$|^\s*(PF_\w+)\s*=\s*(-?\d+)\s*,?\s*$", code, re.M):
        consts[a or c] = int(b or d)
    return protos, consts


with open(os.path.join(INCLUDE, "phyloformer_amd.h")) as _fh:
    PROTOTYPES, CONSTANTS = parse(_fh.read())
