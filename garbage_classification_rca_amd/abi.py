"""The C ABI of libmmrca.so as include/mmrca.h declares it: prototypes as ctypes types, struct field names, enum values.

The header is the one statement of a signature.  lib.load() and jpeg.py type their shared objects from these prototypes (bind), so
no second table exists in Python; the compiler holds every definition in csrc/ to the same header.  tests/test_lib_abi_cpu.py holds
the loaded library and every wrapper's launch arguments against the prototypes without a GPU, and lib.py's conv byte table reads
launch arguments by the parameter names found here.  The parser accepts only the grammar the header's "Conventions" comment states
and raises on anything else -- nothing is guessed.  Imports neither torch nor lib.py.
"""
import ctypes as C
import os
import re
from typing import NamedTuple

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmrca.h")

SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}
RESTYPES = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}
_POINTEES = {"void", "char", "float", "int", "int32_t", "int64_t", "uint64_t"}
_IDENT = re.compile(r"[A-Za-z_]\w*\Z")


class MmrcaError(RuntimeError):
    """a header this parser cannot read or parse (lib.py re-raises it as its own MmrcaError)"""


class Header(NamedTuple):
    functions: dict     # name -> (restype, [(ctype, parameter name), ...])
    structs: dict       # typedef name -> [field name, ...]
    enums: list         # one {name: value} per enum, in header order


def _param(text, fn, structs, struct_pointers):
    if "(" in text or ")" in text:
        raise MmrcaError(f"{fn}: function-pointer or macro parameter '{text}' is outside the header grammar")
    words = [w for w in text.replace("*", " ").split() if w != "const"]
    if len(words) != 2 or not all(_IDENT.match(w) for w in words):
        raise MmrcaError(f"{fn}: cannot parse parameter '{text}' (expected [const] type[*] name)")
    base, name = words
    if "*" in text:
        if base not in _POINTEES and base not in structs:
            raise MmrcaError(f"{fn}: parameter '{text}' points to the unknown type '{base}'")
        return struct_pointers.get(base, C.c_void_p), name
    if base not in SCALARS:
        raise MmrcaError(f"{fn}: parameter '{text}' has the unknown scalar type '{base}'")
    return SCALARS[base], name


def parse(header_path=HEADER_PATH, struct_pointers=None) -> Header:
    """struct_pointers: typedef name -> ctype of a pointer to that struct (every other pointer is a c_void_p)"""
    struct_pointers = struct_pointers or {}
    try:
        text = open(header_path).read()
    except OSError as e:
        raise MmrcaError(f"C ABI header {header_path} cannot be read ({e}): the ctypes binding is derived from it") from None
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    structs, enums = {}, []

    def struct(m):
        fields = [re.search(r"([A-Za-z_]\w*)\s*(\[\w+\])?\Z", part.strip()) for d in m.group(1).split(";") if d.strip() for part in d.split(",")]
        if not all(fields):
            raise MmrcaError(f"{m.group(2)}: cannot parse a field declaration")
        structs[m.group(2)] = [f.group(1) for f in fields]
        return " "

    def enum(m):
        items = [re.match(r"\s*([A-Za-z_]\w*)\s*=\s*(-?\w+)\s*\Z", item) for item in m.group(1).split(",")]
        if not all(items):
            raise MmrcaError(f"enum '{' '.join(m.group(1).split())[:60]}': every enumerator needs an explicit integer value")
        enums.append({i.group(1): int(i.group(2), 0) for i in items})
        return " "

    text = re.sub(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    text = re.sub(r"enum\s*\{(.*?)\}\s*;", enum, text, flags=re.S)
    functions = {}
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        if not stmt:
            continue
        m = re.match(r"(const char ?\*|int64_t\b|int\b) ?(mmrca_\w+) ?\((.*)\)\Z", stmt)
        if m is None:
            named = re.search(r"mmrca_\w+", stmt)
            raise MmrcaError(f"{named.group(0) if named else stmt[:60]!r}: not a prototype of the header grammar: '{stmt[:120]}'")
        ret, fn, params = m.groups()
        if fn in functions:
            raise MmrcaError(f"{fn}: declared twice")
        params = [] if params.strip() == "void" else [_param(p.strip(), fn, structs, struct_pointers) for p in params.split(",")]
        functions[fn] = (RESTYPES[ret.replace(" *", "*")], params)
    return Header(functions, structs, enums)


def prototypes(header_path=HEADER_PATH, struct_pointers=None) -> dict:
    """name -> (restype, [(ctype, parameter name), ...]) of every function the header declares"""
    return parse(header_path, struct_pointers).functions


def bind(cdll, functions) -> None:
    """set restype and argtypes of every function of `functions` (name -> prototype, as prototypes() gives them) on the loaded
    shared object: a call through it is then converted and range-checked as the header declares"""
    for name, (restype, params) in functions.items():
        try:
            fn = getattr(cdll, name)
        except AttributeError:
            raise MmrcaError(f"{name} is declared in the header but {getattr(cdll, '_name', 'the shared object')} does not export it: "
                             "rebuild the library (__graft_entry__.build())") from None
        fn.restype, fn.argtypes = restype, [ctype for ctype, _ in params]
