"""CPU tests of the pack's C ABI (include/zstd_mi355x.h "Packs"): the symbols exist and are typed, ZSTDMI_packBound is the formula the
header states, and the cases that never reach a kernel answer as the header says.  No kernel is launched here."""
import ctypes
import os

import pytest

from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

SYMBOLS = ["ZSTDMI_packBound", "ZSTDMI_compressPack", "ZSTDMI_debugLastPackAlone", "ZSTDMI_debugLastPackFrames"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zstd_mi355x.h")


def sizes_of(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


@pytest.fixture
def cctx():
    lib = _ffi.load()
    c = lib.ZSTD_createCCtx()
    yield c
    lib.ZSTD_freeCCtx(c)


def test_pack_symbols_are_exported_and_typed():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    sig = _ffi.SIGNATURES
    assert sig["ZSTDMI_packBound"][0] is ctypes.c_size_t and len(sig["ZSTDMI_packBound"][1]) == 2
    assert sig["ZSTDMI_compressPack"][0] is ctypes.c_size_t and len(sig["ZSTDMI_compressPack"][1]) == 6
    assert sig["ZSTDMI_debugLastPackAlone"][0] is ctypes.c_int
    assert sig["ZSTDMI_debugLastPackFrames"][0] is ctypes.c_longlong


def test_header_declares_the_four_calls():
    text = " ".join(open(HEADER).read().split())
    for line in ["size_t ZSTDMI_packBound(const size_t* srcSizes, size_t n);",
                 "size_t ZSTDMI_compressPack(ZSTD_CCtx* cctx, void* d_dst, size_t dstCapacity, const void* const* srcs, const size_t* srcSizes, size_t n);",
                 "int ZSTDMI_debugLastPackAlone(const ZSTD_CCtx* cctx);",
                 "long long ZSTDMI_debugLastPackFrames(const ZSTD_CCtx* cctx);"]:
        assert line in text, line


@pytest.mark.parametrize("sizes", [[], [0], [1], [4095, 4096, 65536, 65537]])
def test_pack_bound_is_the_formula(sizes):
    lib = _ffi.load()
    want = sum(lib.ZSTD_compressBound(s) for s in sizes) + 17 + 8 * sum(s // 4096 + 1 for s in sizes)
    assert lib.ZSTDMI_packBound(sizes_of(sizes), len(sizes)) == want
    # one entry: the single call's two bounds
    for s in sizes:
        assert lib.ZSTDMI_packBound(sizes_of([s]), 1) == lib.ZSTD_compressBound(s) + lib.ZSTDMI_seekTableBound(s)


def test_pack_bound_overflow_and_null():
    lib = _ffi.load()
    for sizes in ([(1 << 64) - 1], [1 << 63, 1 << 63], [(1 << 63) - 1] * 3, [5, (1 << 64) - 200]):
        r = lib.ZSTDMI_packBound(sizes_of(sizes), len(sizes))
        assert is_error(r), sizes
    r = lib.ZSTDMI_packBound(None, 2)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert lib.ZSTDMI_packBound(None, 0) == 17


def test_null_context_and_null_arrays_are_generic(cctx):
    lib = _ffi.load()
    dst = ctypes.create_string_buffer(b"\xA5" * 64, 64)
    srcs = (ctypes.c_void_p * 2)()
    sizes = sizes_of([0, 0])
    for n in (0, 2):
        r = lib.ZSTDMI_compressPack(None, dst, 64, srcs, sizes, n)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    for a, b in ((None, sizes), (srcs, None), (None, None)):
        r = lib.ZSTDMI_compressPack(cctx, dst, 64, a, b, 2)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert dst.raw == b"\xA5" * 64


def test_debug_calls_without_a_context_and_on_a_fresh_one(cctx):
    lib = _ffi.load()
    assert lib.ZSTDMI_debugLastPackAlone(None) == -1 and lib.ZSTDMI_debugLastPackFrames(None) == -1
    assert lib.ZSTDMI_debugLastPackAlone(cctx) == 0 and lib.ZSTDMI_debugLastPackFrames(cctx) == 0


def test_pack_fails_loudly_without_gpu(cctx):
    """No CPU fallback: without a gfx950 device the call fails as a whole with init_missing and touches nothing."""
    lib = _ffi.load()
    if lib.ZSTDMI_deviceCount() > 0:
        pytest.skip("a GPU is visible here")
    dst = ctypes.create_string_buffer(b"\xA5" * 64, 64)
    r = lib.ZSTDMI_compressPack(cctx, dst, 64, None, None, 0)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_init_missing
    assert dst.raw == b"\xA5" * 64
