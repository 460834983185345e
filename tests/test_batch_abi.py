"""CPU tests of the batched calls' C ABI (include/zstd_mi355x.h "Many small buffers in one call"): the symbols exist and are typed,
and the cases that never reach a kernel answer as the header says.  No kernel is launched here."""
import ctypes

import pytest

from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

SYMBOLS = ["ZSTDMI_compressBatch", "ZSTDMI_decompressBatch", "ZSTDMI_debugLastBatchAlone", "ZSTDMI_debugLastBatchAloneD"]


def _arrays(n):
    ptrs = (ctypes.c_void_p * max(n, 1))()
    sizes = (ctypes.c_size_t * max(n, 1))()
    return ptrs, sizes


def test_batch_symbols_are_exported_and_typed():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    assert _ffi.SIGNATURES["ZSTDMI_compressBatch"][0] is ctypes.c_size_t and len(_ffi.SIGNATURES["ZSTDMI_compressBatch"][1]) == 7
    assert _ffi.SIGNATURES["ZSTDMI_debugLastBatchAlone"][0] is ctypes.c_int


SIDES = {"compress": ("ZSTDMI_compressBatch", "ZSTD_createCCtx", "ZSTD_freeCCtx", "ZSTDMI_debugLastBatchAlone"),
         "decompress": ("ZSTDMI_decompressBatch", "ZSTD_createDCtx", "ZSTD_freeDCtx", "ZSTDMI_debugLastBatchAloneD")}


@pytest.fixture(params=list(SIDES))
def side(request):
    """-> (the batch call, a context of its kind, its diagnostic)"""
    lib = _ffi.load()
    call, create, free, alone = SIDES[request.param]
    ctx = getattr(lib, create)()
    yield getattr(lib, call), ctx, getattr(lib, alone)
    getattr(lib, free)(ctx)


def test_empty_batch_returns_zero(side):
    call, ctx, alone = side
    srcs, sizes = _arrays(0)
    dsts, caps = _arrays(0)
    got = (ctypes.c_size_t * 1)()
    assert call(ctx, srcs, sizes, 0, dsts, caps, got) == 0
    assert call(ctx, None, None, 0, None, None, None) == 0      # (n == 0: the arrays are not looked at)
    assert alone(ctx) == 0


def test_null_context_is_an_error(side):
    call, _, alone = side
    srcs, sizes = _arrays(1)
    dsts, caps = _arrays(1)
    got = (ctypes.c_size_t * 1)()
    for n in (0, 1):
        r = call(None, srcs, sizes, n, dsts, caps, got)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert alone(None) == -1


def test_null_array_with_entries_is_an_error(side):
    call, ctx, _ = side
    for missing in range(5):
        srcs, sizes = _arrays(2)
        dsts, caps = _arrays(2)
        got = (ctypes.c_size_t * 2)()
        args = [srcs, sizes, dsts, caps, got]
        args[missing] = None
        r = call(ctx, args[0], args[1], 2, args[2], args[3], args[4])
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC, missing


def test_batch_fails_loudly_without_gpu(side):
    """No CPU fallback: without a gfx950 device a batch of n > 0 fails as a whole with init_missing and touches nothing."""
    if _ffi.load().ZSTDMI_deviceCount() > 0:
        pytest.skip("a GPU is visible here")
    call, ctx, _ = side
    src = ctypes.create_string_buffer(bytes([0x28, 0xB5, 0x2F, 0xFD, 0x20, 0x00, 0x01, 0x00, 0x00]), 9)
    dst = ctypes.create_string_buffer(b"\xA5" * 64, 64)
    srcs, sizes = _arrays(1)
    dsts, caps = _arrays(1)
    srcs[0], sizes[0], dsts[0], caps[0] = ctypes.addressof(src), 9, ctypes.addressof(dst), 64
    got = (ctypes.c_size_t * 1)(12345)
    r = call(ctx, srcs, sizes, 1, dsts, caps, got)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_init_missing
    assert got[0] == 12345 and dst.raw == b"\xA5" * 64
