"""CPU (-m "not gpu"): argument validation of ivl_linear_m256_fwd returns its error codes (and a message) without touching a GPU."""
import ctypes
import os

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def test_linear_m256_argument_validation(lib):
    from infinitevl_amd import _lib
    one = ctypes.c_void_p(0x1000)       # never dereferenced: validation fails first
    f = lib.ivl_linear_m256_fwd
    assert f(None, one, None, one, 256, 64, 64, 0, None) == _lib.IVL_ERR_INVALID_ARG and b"NULL" in lib.ivl_last_error()
    assert f(one, None, None, one, 256, 64, 64, 1, None) == _lib.IVL_ERR_INVALID_ARG
    assert f(one, one, None, None, 256, 64, 64, 0, None) == _lib.IVL_ERR_INVALID_ARG
    assert f(one, one, None, one, 0, 64, 64, 0, None) == _lib.IVL_ERR_INVALID_ARG
    assert f(one, one, None, one, 257, 64, 64, 0, None) == _lib.IVL_ERR_UNSUPPORTED           # more than 256 rows
    assert b"M=257" in lib.ivl_last_error()
    assert f(one, one, None, one, 4096, 64, 64, 1, None) == _lib.IVL_ERR_UNSUPPORTED
    assert f(one, one, None, one, 256, 100, 136, 0, None) == _lib.IVL_ERR_UNSUPPORTED         # K % 64
    assert f(one, one, None, one, 256, 64, 16384 + 64, 0, None) == _lib.IVL_ERR_UNSUPPORTED   # K too large
    assert f(one, one, None, one, 256, 102, 128, 0, None) == _lib.IVL_ERR_UNSUPPORTED         # N % 4
    assert f(one, one, None, one, 256, 600000, 4096, 1, None) == _lib.IVL_ERR_UNSUPPORTED      # 32-bit DMA offsets
    odd = ctypes.c_void_p(0x1008)
    assert f(odd, one, None, one, 256, 64, 64, 0, None) == _lib.IVL_ERR_INVALID_ARG           # x not 16-byte aligned
    with pytest.raises(ValueError):
        _lib.check(f(one, one, None, one, 257, 64, 64, 0, None))
