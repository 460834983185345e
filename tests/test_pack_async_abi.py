"""CPU tests of the C ABI of ZSTDMI_compressPackAsync / ZSTDMI_CCtx_packAsyncBound (include/zstd_mi355x.h "a pack enqueued from the
device"): the symbols exist, are typed and declared, and the answers that need no device are the header's.  No kernel is launched here;
a canary buffer passed as the destination stays untouched throughout."""
import ctypes
import os
import re

from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ZSTDMI_CCtx_packAsyncBound", "ZSTDMI_compressPackAsync"]
GENERIC, STAGE_WRONG = ZSTD_ErrorCode.ZSTD_error_GENERIC, ZSTD_ErrorCode.ZSTD_error_stage_wrong
DST_NULL, TOO_SMALL = ZSTD_ErrorCode.ZSTD_error_dstBuffer_null, ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall


def _code(r):
    assert is_error(r), r
    return get_error_code(r)


class Canary:
    """host memory standing in for every pointer of the call: nothing may read or write it in a call that is refused on the host"""

    def __init__(self):
        self.dst = ctypes.create_string_buffer(b"\xA5" * 256, 256)
        self.cols = (ctypes.c_size_t * 8)(*[0x5A5A5A5A] * 8)
        self.out = (ctypes.c_size_t * 2)(0x5A5A5A5A, 0x5A5A5A5A)

    def untouched(self):
        return self.dst.raw == b"\xA5" * 256 and list(self.cols) == [0x5A5A5A5A] * 8 and list(self.out) == [0x5A5A5A5A] * 2

    def call(self, lib, ctx, dst="dst", cap=256, srcs="cols", sizes="cols", n=4, out="out", ends=None):
        ptr = {"dst": ctypes.addressof(self.dst), "cols": ctypes.addressof(self.cols), "out": ctypes.addressof(self.out), None: None}
        return lib.ZSTDMI_compressPackAsync(ctx, ptr[dst], cap, ptr[srcs], ptr[sizes], n, ptr[out], ptr[ends])


def test_symbols_are_exported_and_typed():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    v, s = ctypes.c_void_p, ctypes.c_size_t
    assert _ffi.SIGNATURES["ZSTDMI_CCtx_packAsyncBound"] == (s, [v, s])
    assert _ffi.SIGNATURES["ZSTDMI_compressPackAsync"] == (s, [v, v, s, v, v, s, v, v])


def test_the_header_declares_both_calls_verbatim():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read())
    assert "size_t ZSTDMI_CCtx_packAsyncBound(const ZSTD_CCtx* cctx, size_t n);" in text
    assert ("size_t ZSTDMI_compressPackAsync(ZSTD_CCtx* cctx, void* d_dst, size_t dstCapacity, const void* const* d_srcs, const size_t* d_srcSizes, "
            "size_t n, size_t* d_packSize, size_t* d_entryEnds /* may be NULL */);") in text


def test_null_arguments_are_answered_on_the_host():
    lib = _ffi.load()
    k = Canary()
    assert _code(k.call(lib, None)) == GENERIC
    assert _code(lib.ZSTDMI_CCtx_packAsyncBound(None, 4)) == GENERIC
    ctx = lib.ZSTD_createCCtx()
    try:
        assert _code(k.call(lib, ctx, out=None)) == GENERIC
        assert _code(k.call(lib, ctx, srcs=None)) == GENERIC
        assert _code(k.call(lib, ctx, sizes=None)) == GENERIC
        assert _code(k.call(lib, ctx, out=None, n=0, srcs=None, sizes=None)) == GENERIC
        assert _code(k.call(lib, ctx, dst=None, cap=256)) == DST_NULL
        assert _code(k.call(lib, ctx, dst=None, cap=0)) == TOO_SMALL
        assert _code(k.call(lib, ctx, dst=None, cap=0, n=0, srcs=None, sizes=None)) == TOO_SMALL
        assert k.untouched()
        assert lib.ZSTDMI_debugHostWaits(ctx) == 0 and lib.ZSTDMI_debugDeviceAllocs(ctx) == 0
    finally:
        lib.ZSTD_freeCCtx(ctx)


def test_stage_wrong_without_a_valid_prepare():
    lib = _ffi.load()
    k = Canary()
    ctx = lib.ZSTD_createCCtx()
    try:
        assert _code(lib.ZSTDMI_CCtx_packAsyncBound(ctx, 0)) == STAGE_WRONG
        assert _code(lib.ZSTDMI_CCtx_packAsyncBound(ctx, 4)) == STAGE_WRONG
        assert _code(k.call(lib, ctx)) == STAGE_WRONG
        assert _code(k.call(lib, ctx, ends="cols")) == STAGE_WRONG
        assert _code(k.call(lib, ctx, n=0, srcs=None, sizes=None)) == STAGE_WRONG         # (the empty table needs a prepare too)
        # a refused prepare leaves the context without one
        assert lib.ZSTDMI_CCtx_setSeekTable(ctx, 1) == 0
        assert _code(lib.ZSTDMI_CCtx_prepareBatchAsync(ctx, 16, 4096)) == ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
        assert _code(k.call(lib, ctx)) == STAGE_WRONG
        assert _code(lib.ZSTDMI_CCtx_packAsyncBound(ctx, 4)) == STAGE_WRONG
        assert k.untouched()
        assert lib.ZSTDMI_debugHostWaits(ctx) == 0 and lib.ZSTDMI_debugDeviceAllocs(ctx) == 0
    finally:
        lib.ZSTD_freeCCtx(ctx)
