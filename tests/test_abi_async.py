"""CPU tests of the C ABI of the batch enqueued from the device (include/zstd_mi355x.h "a batch enqueued from the device"): the symbols
exist and are typed, and the answers that need no device are the header's.  No kernel is launched here."""
import ctypes

from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

SYMBOLS = ["ZSTDMI_CCtx_prepareBatchAsync", "ZSTDMI_compressBatchAsync", "ZSTDMI_debugHostWaits", "ZSTDMI_debugDeviceAllocs"]


def _code(r):
    assert is_error(r), r
    return get_error_code(r)


def test_async_symbols_are_exported_and_typed():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    assert _ffi.SIGNATURES["ZSTDMI_compressBatchAsync"][0] is ctypes.c_size_t and len(_ffi.SIGNATURES["ZSTDMI_compressBatchAsync"][1]) == 7
    assert _ffi.SIGNATURES["ZSTDMI_CCtx_prepareBatchAsync"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t])
    for name in SYMBOLS[2:]:
        assert _ffi.SIGNATURES[name][0] is ctypes.c_longlong


def test_debug_counters_without_a_context():
    lib = _ffi.load()
    assert lib.ZSTDMI_debugHostWaits(None) == -1
    assert lib.ZSTDMI_debugDeviceAllocs(None) == -1
    ctx = lib.ZSTD_createCCtx()
    try:
        assert lib.ZSTDMI_debugHostWaits(ctx) == 0 and lib.ZSTDMI_debugDeviceAllocs(ctx) == 0
    finally:
        lib.ZSTD_freeCCtx(ctx)


def test_null_context_is_generic():
    lib = _ffi.load()
    for n in (0, 1):
        assert _code(lib.ZSTDMI_compressBatchAsync(None, 8, 8, n, 8, 8, 8)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert _code(lib.ZSTDMI_CCtx_prepareBatchAsync(None, 16, 4096)) == ZSTD_ErrorCode.ZSTD_error_GENERIC


def test_answers_that_touch_no_device():
    """n == 0 is 0 whatever the arrays are; a NULL array with entries is GENERIC; without a prepare the call is stage_wrong; the prepare
    refuses a bound of 0, a bound above one block, the seek-table switch and too many entries before it looks for a device."""
    lib = _ffi.load()
    ctx = lib.ZSTD_createCCtx()
    try:
        assert lib.ZSTDMI_compressBatchAsync(ctx, None, None, 0, None, None, None) == 0
        for missing in range(5):
            args = [8, 8, 8, 8, 8]
            args[missing] = None
            assert _code(lib.ZSTDMI_compressBatchAsync(ctx, args[0], args[1], 2, args[2], args[3], args[4])) == ZSTD_ErrorCode.ZSTD_error_GENERIC
        assert _code(lib.ZSTDMI_compressBatchAsync(ctx, 8, 8, 1, 8, 8, 8)) == ZSTD_ErrorCode.ZSTD_error_stage_wrong
        unsupported = ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
        assert _code(lib.ZSTDMI_CCtx_prepareBatchAsync(ctx, 16, 0)) == unsupported
        assert _code(lib.ZSTDMI_CCtx_prepareBatchAsync(ctx, 16, 65537)) == unsupported
        assert _code(lib.ZSTDMI_CCtx_prepareBatchAsync(ctx, 16385, 4096)) == unsupported
        assert lib.ZSTDMI_CCtx_setSeekTable(ctx, 1) == 0
        assert _code(lib.ZSTDMI_CCtx_prepareBatchAsync(ctx, 16, 4096)) == unsupported
        assert lib.ZSTDMI_debugHostWaits(ctx) == 0 and lib.ZSTDMI_debugDeviceAllocs(ctx) == 0
    finally:
        lib.ZSTD_freeCCtx(ctx)
