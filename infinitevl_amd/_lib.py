"""ctypes binding of libivl_hip.so, derived from the C ABI's one declaration: include/ivl_hip.h.

The header is read at import (no library needed): its `#define IVL_*` integers become module attributes, every `struct
ivl_<x>_args` a ctypes class (`SwaArgs`, `SampleArgs`, `LoraArgs` in `ARG_STRUCTS`; a companion group such as `SampleAdjArgs` in `GROUP_STRUCTS`;
the struct of an in-place edit such as `BanArgs` in `EDIT_STRUCTS`), and every `IVL_API` prototype an entry of `PROTOTYPES`, which `bind`
applies to a CDLL.
The library is built in-tree by `__graft_entry__.build()` / `make -C infinitevl_amd/csrc`.
There is NO fallback: if the shared object is missing, importing an operator raises.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libivl_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ivl_hip.h")

# every C type the header may use; a pointer to anything else is handed over as void*
_C_TYPES = {"int": c_int, "float": c_float, "size_t": c_size_t, "int64_t": c_int64, "const char*": c_char_p}
_DECL = r"(.+?[\s*])\s*"                                    # the type in front of a declared name


def _ctype(c_type: str, where: str, known: dict):
    c_type = re.sub(r"\s*\*\s*", "*", " ".join(c_type.split()))
    if c_type in known:
        return known[c_type]
    if c_type.endswith("*"):
        return c_void_p
    raise ImportError(f"ivl_hip.h: {where}: no ctypes type for the C type {c_type!r}")


def _int_expr(expr: str, where: str) -> int:
    """Integer literals, unary minus, + / - and parentheses: what the header's constants are written with."""
    toks = re.findall(r"\d+|\S", expr)

    def term():
        t = toks.pop(0)
        if t == "-":
            return -term()
        if t != "(":
            return int(t)
        v = total()
        if toks.pop(0) != ")":
            raise ValueError
        return v

    def total():
        v = term()
        while toks and toks[0] in "+-":
            v += term() if toks.pop(0) == "+" else -term()
        return v
    try:
        v = total()
        if toks:
            raise ValueError
        return v
    except (ValueError, IndexError):
        raise ImportError(f"ivl_hip.h: {where}: not an integer expression: {expr!r}") from None


def parse_header(text: str, structs: dict = None, groups: dict = None, edits: dict = None):
    """(constants {name: int}, the SwaArgs class, prototypes {name: (restype, [argument types])}) of a header text.  `structs`,
    when given, receives every `typedef struct ivl_<x>_args` of the header that some entry point takes as its FIRST parameter
    as {"ivl_<x>_args": its ctypes class}; `groups`, when given, the others: a companion group, which only ever rides beside
    another struct (ivl_sample_adj_args beside ivl_sample_args).  A struct whose FIRST member is a writable pointer (`void* logits`
    of ivl_ban_args: its entry point edits that buffer in place and computes nothing else) is neither: it goes to `edits`, when
    given, whoever takes it."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(IVL_\w+)[ \t]+(\S[^\n]*)", text, re.M)     # (the include guard has no value)
    consts = {name: _int_expr(expr, "#define " + name) for name, expr in defines if name != "IVL_API"}
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    out, structs, writable = structs, {}, set()
    for tag, body in re.findall(r"typedef\s+struct\s+(ivl_\w+_args)\s*\{(.*?)\}\s*\1\s*;", text, re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(_DECL + r"(\w+(?:\s*,\s*\w+)*)", decl, re.S)
            if m is None:
                raise ImportError(f"ivl_hip.h: {tag}: cannot read the field declaration {decl!r}")
            fields += [(name, _ctype(m.group(1), f"{tag}.{name}", _C_TYPES)) for name in re.split(r"\s*,\s*", m.group(2))]
        if re.match(r"\s*(?!const\b)\w[\w\s]*\*", body):
            writable.add(tag)
        cls = "".join(w.capitalize() for w in tag.split("_")[1:])                                  # ivl_swa_args -> SwaArgs
        structs[tag] = type(cls, (Structure,), {"_fields_": fields, "__doc__": f"struct {tag} (include/ivl_hip.h)."})
    if "ivl_swa_args" not in structs:
        raise ImportError("ivl_hip.h: struct ivl_swa_args not found")
    known = {**_C_TYPES, **{f"const {tag}*": POINTER(cls) for tag, cls in structs.items()}}
    protos = {}
    first = set()
    for ret, name, params in re.findall(r"\bIVL_API\s+" + _DECL + r"(\w+)\s*\(([^()]*)\)\s*;", text, re.S):
        types = []
        first.update(re.findall(r"^\s*const\s+(ivl_\w+_args)\s*\*", params))
        for param in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(_DECL + r"\w+", param.strip(), re.S)
            types.append(_ctype(m.group(1) if m else param, name, known))
        protos[name] = (_ctype(ret, name, known), types)
    if len(protos) != len(re.findall(r"\bIVL_API\b", text)):
        raise ImportError(f"ivl_hip.h: only {len(protos)} of its IVL_API declarations are readable prototypes (the last one "
                          f"read: {list(protos)[-1:]})")
    # (the rule is read off the prototypes: an entry point that took a companion group first would move it to `structs`)
    for tag, cls in structs.items():
        into = edits if tag in writable else out if tag in first else groups
        if into is not None:
            into[tag] = cls
    return consts, structs["ivl_swa_args"], protos


if not os.path.exists(HEADER_PATH):
    raise ImportError(f"{HEADER_PATH} not found: the package is used in-tree and reads the C ABI from the header at import.")
ARG_STRUCTS = {}                                             # every `ivl_<x>_args` struct an entry point takes first: {"ivl_swa_args": SwaArgs, ...}
GROUP_STRUCTS = {}                                           # the companion groups: {"ivl_sample_adj_args": SampleAdjArgs}
EDIT_STRUCTS = {}                                            # the structs of in-place edits: {"ivl_ban_args": BanArgs}
with open(HEADER_PATH) as _f:
    CONSTANTS, SwaArgs, PROTOTYPES = parse_header(_f.read(), ARG_STRUCTS, GROUP_STRUCTS, EDIT_STRUCTS)
SampleArgs, LoraArgs = ARG_STRUCTS["ivl_sample_args"], ARG_STRUCTS["ivl_lora_args"]
SampleAdjArgs = GROUP_STRUCTS["ivl_sample_adj_args"]
BanArgs = EDIT_STRUCTS["ivl_ban_args"]
# the two wide argument structs (32 fields and more) whose sizes and key offsets tests/test_header_binding_cpu.py pins as numbers
STRUCTS = {"ivl_swa_args": SwaArgs, "ivl_sample_args": SampleArgs}
globals().update(CONSTANTS)                                  # IVL_ABI_VERSION, IVL_BF16, ..., IVL_OK, IVL_ERR_*, IVL_GDN_*
EXPORTED_SYMBOLS = tuple(PROTOTYPES)


class IvlError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libivl_hip error {code}: {msg}")
        self.code = code


def bind(cdll: ctypes.CDLL, require_all: bool = True) -> ctypes.CDLL:
    """Declare every prototype of the header on `cdll`.  require_all: a symbol the object lacks raises AttributeError (the
    product library); otherwise it is skipped (an older build of the library in a developer A/B)."""
    for name in PROTOTYPES:
        if require_all or hasattr(cdll, name):
            fn = getattr(cdll, name)
            fn.restype, fn.argtypes = PROTOTYPES[name]
    return cdll


_lib = None


def load(path: str = None) -> ctypes.CDLL:
    """Load the shared object once and declare every prototype.  `path` (developer tools only: the
    instrumented build libivl_hip_trace.so, an older build) must be given before the first operator call."""
    global _lib
    if _lib is not None:
        return _lib
    if path is not None:
        globals()["LIB_PATH"] = path
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found. The MI355X kernels are mandatory (there is no CPU or PyTorch fallback): "
            "build them with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C infinitevl_amd/csrc`.")
    _lib = lib = bind(ctypes.CDLL(LIB_PATH), require_all=path is None)
    # the one environment switch, on the Python side: IVL_GDN_RESIDENT_BLOCKS=0 forces the two-launch form of the fused GDN call
    env = os.environ.get("IVL_GDN_RESIDENT_BLOCKS", "")
    if env.strip() and hasattr(lib, "ivl_gdn_resident_blocks"):
        lib.ivl_gdn_resident_blocks(int(env))
    return lib


def check(rc: int) -> None:
    """Map a C status to the Python exception types the reference raises
    (SURVEY.md section 8b "Error conventions")."""
    if rc == IVL_OK:
        return
    msg = load().ivl_last_error().decode("utf-8", "replace")
    if rc in (IVL_ERR_INVALID_ARG, IVL_ERR_UNSUPPORTED):
        raise ValueError(f"libivl_hip ({rc}): {msg}")
    raise IvlError(rc, msg)
