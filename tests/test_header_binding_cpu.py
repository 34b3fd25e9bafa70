"""CPU (-m "not gpu"): the ctypes binding is what include/ivl_hip.h declares.  The header reader of infinitevl_amd/_lib.py on
small synthetic headers (every type form the real header uses; an unknown type is an error that names it), on the real header
(prototype count, constants), against a host C compiler (sizeof / offsetof of ivl_swa_args and ivl_sample_args, the values of the
constants), and `bind` on the built library and on a stand-in object that lacks a symbol."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_size_t, c_void_p

import pytest

from conftest import ROOT
from infinitevl_amd import _lib

HEADER = os.path.join(ROOT, "include", "ivl_hip.h")
CONSTANT_NAMES = {"IVL_ABI_VERSION", "IVL_BF16", "IVL_F32", "IVL_FP8_E4M3", "IVL_OK", "IVL_ERR_INVALID_ARG", "IVL_ERR_UNSUPPORTED",
                  "IVL_ERR_WORKSPACE", "IVL_ERR_LAUNCH", "IVL_ERR_SYNC", "IVL_GDN_SYNC_BYTES", "IVL_GDN_RESIDENT_QUERY"}

STRUCT = """
typedef struct ivl_swa_args {
  const void* q;      /* a comment; with, punctuation (and parentheses) */
  void* o;
  int64_t q_sb, q_st,
          q_sh;
  int B, T;           // a line comment
  const int64_t* pos_dev;
  float scaling;
  size_t workspace_bytes;
} ivl_swa_args;
"""
STRUCT2 = """
typedef struct ivl_pick_args {
  /* a group */
  const float* w; int32_t* out;
  int n, k;
  int64_t ld;
} ivl_pick_args;
"""
SYNTHETIC = """
#ifndef IVL_HIP_H
#define IVL_HIP_H
#include <stddef.h>
#define IVL_API __attribute__((visibility("default")))
#define IVL_ABI_VERSION 12
#define IVL_ERR_SYNC (-5)   /* a wait ran out (see ivl_f) */
#define IVL_QUERY (-2147483647 - 1)
  #  define IVL_SUM (1 + (2 - -3))
""" + STRUCT + STRUCT2 + """
IVL_API int ivl_version(void);
IVL_API const char* ivl_last_error(void);
/* IVL_API int ivl_commented_out(int x); */
IVL_API size_t ivl_bytes(int B, int64_t ld);
IVL_API int ivl_f(const void* x, void* y, const float* g, /* between, arguments */ const int64_t* pos,
          int64_t* counter,
          int n, float scale, size_t bytes, int64_t delta,   // trailing
          const int32_t *cu, void* stream);
IVL_API int ivl_swa(const ivl_swa_args* args, void* stream);
IVL_API int ivl_pick(const ivl_pick_args *args, const ivl_swa_args* other, void* stream);
#endif
"""


def test_reader_on_synthetic_headers():
    structs = {}
    consts, swa, protos = _lib.parse_header(SYNTHETIC, structs)
    assert consts == {"IVL_ABI_VERSION": 12, "IVL_ERR_SYNC": -5, "IVL_QUERY": -2 ** 31, "IVL_SUM": 6}
    assert issubclass(swa, ctypes.Structure) and list(structs) == ["ivl_swa_args", "ivl_pick_args"] and structs["ivl_swa_args"] is swa
    pick = structs["ivl_pick_args"]
    assert issubclass(pick, ctypes.Structure) and pick.__name__ == "PickArgs"
    assert pick._fields_ == [("w", c_void_p), ("out", c_void_p), ("n", c_int), ("k", c_int), ("ld", c_int64)]
    assert swa._fields_ == [("q", c_void_p), ("o", c_void_p), ("q_sb", c_int64), ("q_st", c_int64), ("q_sh", c_int64), ("B", c_int),
                            ("T", c_int), ("pos_dev", c_void_p), ("scaling", c_float), ("workspace_bytes", c_size_t)]
    vp = c_void_p
    assert list(protos) == ["ivl_version", "ivl_last_error", "ivl_bytes", "ivl_f", "ivl_swa", "ivl_pick"]          # header order
    assert protos["ivl_version"] == (c_int, [])
    assert protos["ivl_last_error"] == (c_char_p, [])
    assert protos["ivl_bytes"] == (c_size_t, [c_int, c_int64])
    assert protos["ivl_f"] == (c_int, [vp, vp, vp, vp, vp, c_int, c_float, c_size_t, c_int64, vp, vp])
    assert protos["ivl_swa"] == (c_int, [POINTER(swa), vp])
    assert protos["ivl_pick"] == (c_int, [POINTER(pick), POINTER(swa), vp])


@pytest.mark.parametrize("decl, named", [
    ("IVL_API int ivl_g(const void* x, double scale);", ("ivl_g", "double")),
    ("IVL_API int ivl_g(unsigned n, void* stream);", ("ivl_g", "unsigned")),
    ("IVL_API double ivl_g(void);", ("ivl_g", "double")),
    ("IVL_API int ivl_g(ivl_swa_args args);", ("ivl_g", "ivl_swa_args")),
    ("IVL_API int ivl_g(int (*callback)(int));", ("1 of", "ivl_first")),       # not skipped: the count and the last one read
    ("#define IVL_WIDE 16384u", ("IVL_WIDE", "16384u")),
    ("#define IVL_HEX 0x10", ("IVL_HEX",)),
    ("#define IVL_SHIFT (1 << 4)", ("IVL_SHIFT",)),
    ("#define IVL_OPEN (1 + 2", ("IVL_OPEN",)),
], ids=["double_arg", "unsigned_arg", "double_return", "struct_by_value", "function_pointer", "suffix", "hex", "shift", "open_paren"])
def test_reader_refuses_what_it_does_not_know(decl, named):
    with pytest.raises(ImportError) as e:
        _lib.parse_header(STRUCT + "IVL_API int ivl_first(void);\n" + decl + "\n")
    for word in named:
        assert word in str(e.value), (word, str(e.value))


def test_reader_refuses_an_unknown_struct_field_type():
    with pytest.raises(ImportError, match=r"ivl_swa_args\.ratio.*'double'"):
        _lib.parse_header(STRUCT.replace("float scaling;", "float scaling; double ratio;"))
    with pytest.raises(ImportError, match=r"ivl_pick_args\.k.*'unsigned'"):
        _lib.parse_header(STRUCT + STRUCT2.replace("int n, k;", "int n; unsigned k;"))
    with pytest.raises(ImportError, match=r"ivl_pick_args: cannot read"):
        _lib.parse_header(STRUCT + STRUCT2.replace("int n, k;", "int n, k[2];"))
    for text in ("IVL_API int ivl_first(void);", STRUCT2):               # a header without ivl_swa_args
        with pytest.raises(ImportError, match="ivl_swa_args not found"):
            _lib.parse_header(text)


def test_real_header_prototype_count_and_constants():
    hdr = open(HEADER).read()
    declared = re.findall(r"^IVL_API [^\n(]*?\b(ivl_[a-z0-9_]+)\s*\(", hdr, flags=re.M)
    assert len(_lib.PROTOTYPES) == len(declared) >= 37
    assert list(_lib.EXPORTED_SYMBOLS) == list(_lib.PROTOTYPES) == declared                          # header order
    assert set(_lib.CONSTANTS) == CONSTANT_NAMES
    for name, value in _lib.CONSTANTS.items():
        assert getattr(_lib, name) == value and type(value) is int
    assert (_lib.IVL_ABI_VERSION, _lib.IVL_BF16, _lib.IVL_F32, _lib.IVL_FP8_E4M3, _lib.IVL_OK) == (12, 0, 2, 3, 0)
    assert _lib.SwaArgs.__name__ == "SwaArgs" and issubclass(_lib.SwaArgs, ctypes.Structure)
    assert _lib.PROTOTYPES["ivl_swa_fwd"] == (c_int, [POINTER(_lib.SwaArgs), c_void_p])
    assert _lib.SampleArgs.__name__ == "SampleArgs" and issubclass(_lib.SampleArgs, ctypes.Structure)
    assert _lib.STRUCTS == {"ivl_swa_args": _lib.SwaArgs, "ivl_sample_args": _lib.SampleArgs}
    assert _lib.PROTOTYPES["ivl_sample_rows_fwd"] == (c_int, [POINTER(_lib.SampleArgs), c_void_p])
    assert _lib.PROTOTYPES["ivl_last_error"] == (c_char_p, [])


def _host_cc():
    """`cc`, else the clang that ships beside hipcc: a machine that can build the library has one."""
    hipcc = os.path.realpath(shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(hipcc))
    for cand in (shutil.which("cc"), os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang")):
        if cand and os.path.exists(cand):
            return cand
    raise AssertionError(f"no host C compiler: neither `cc` nor a clang under {rocm}")


def test_struct_layout_and_constants_against_the_c_compiler(tmp_path):
    fields = [name for name, _ in _lib.SwaArgs._fields_]
    assert len(fields) >= 32 and {"pos", "scaling", "workspace", "pos_min"} <= set(fields)
    lines = ['#include <stdio.h>', '#include "ivl_hip.h"', 'int main(void) {']
    for tag, cls in _lib.STRUCTS.items():
        lines += [f'  printf("sizeof {tag} %zu\\n", sizeof({tag}));']
        lines += [f'  printf("offsetof {tag} {f} %zu\\n", offsetof({tag}, {f}));' for f, _ in cls._fields_]
    lines += [f'  printf("const {c} %lld\\n", (long long)({c}));' for c in sorted(CONSTANT_NAMES)]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([_host_cc(), "-I", os.path.dirname(HEADER), str(src), "-o", exe], check=True, capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {tuple(ln.split()[:-1]): int(ln.split()[-1]) for ln in out.splitlines()}
    assert got[("sizeof", "ivl_swa_args")] == ctypes.sizeof(_lib.SwaArgs) == 208
    assert got[("sizeof", "ivl_sample_args")] == ctypes.sizeof(_lib.SampleArgs) == 312
    for tag, cls in _lib.STRUCTS.items():
        assert len(cls._fields_) >= 32
        for f, _ in cls._fields_:
            assert got[("offsetof", tag, f)] == getattr(cls, f).offset, (tag, f)
    assert [got[("offsetof", "ivl_swa_args", f)] for f in ("pos", "scaling", "workspace", "pos_min")] == [128, 144, 152, 200]
    assert [got[("offsetof", "ivl_sample_args", f)] for f in ("temperature", "hist_ld", "n_states", "score_only")] == \
        [24, 176, 272, 304]
    for c in CONSTANT_NAMES:
        assert got[("const", c)] == getattr(_lib, c), c
    assert got[("const", "IVL_GDN_RESIDENT_QUERY")] == -2 ** 31 and got[("const", "IVL_GDN_SYNC_BYTES")] == 16384


def test_load_declares_every_symbol_of_the_product_library():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert len(_lib.PROTOTYPES) >= 37
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    fresh = _lib.bind(ctypes.CDLL(so))                                                             # the product rule on a new handle
    assert fresh.ivl_abi_version() == _lib.IVL_ABI_VERSION == 12


class _Fn:
    pass


class _OlderBuild:
    """A stand-in for a library that exports everything but `missing`."""

    def __init__(self, missing):
        for name in _lib.PROTOTYPES:
            if name not in missing:
                setattr(self, name, _Fn())


def test_bind_skips_missing_symbols_only_for_a_developer_library():
    missing = {"ivl_linear_m256_fwd", "ivl_swa_decode_rows_fwd"}
    obj = _lib.bind(_OlderBuild(missing), require_all=False)
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        if name in missing:
            assert not hasattr(obj, name)
        else:
            assert getattr(obj, name).restype is restype and getattr(obj, name).argtypes == argtypes, name
    with pytest.raises(AttributeError, match="ivl_linear_m256_fwd|ivl_swa_decode_rows_fwd"):
        _lib.bind(_OlderBuild(missing), require_all=True)
    with pytest.raises(AttributeError):
        _lib.bind(_OlderBuild(missing))                                                             # the default is the product rule
