"""CPU tests of the C ABI of ZSTDMI_CCtx_prepareBatchAsyncLimits / ZSTDMI_CCtx_getBatchAsyncPlan (include/zstd_mi355x.h "entries of
several blocks: the second prepare"): the symbols exist and are typed, and the answers that need no device are the header's.  No kernel
is launched here."""
import ctypes

from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

SYMBOLS = ["ZSTDMI_CCtx_prepareBatchAsyncLimits", "ZSTDMI_CCtx_getBatchAsyncPlan"]
FOUR_MIB = 4 << 20


def _code(r):
    assert is_error(r), r
    return get_error_code(r)


def _limits(maxEntries=16, srcSizeBound=262144, maxChunks=0, reserved=(0, 0, 0)):
    return _ffi.CBatchLimits(maxEntries, srcSizeBound, maxChunks, (ctypes.c_size_t * 3)(*reserved))


def _prepare(lib, ctx, **fields):
    return lib.ZSTDMI_CCtx_prepareBatchAsyncLimits(ctx, ctypes.byref(_limits(**fields)))


def test_symbols_are_exported_and_typed():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    assert _ffi.SIGNATURES["ZSTDMI_CCtx_prepareBatchAsyncLimits"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.POINTER(_ffi.CBatchLimits)])
    size_p = ctypes.POINTER(ctypes.c_size_t)
    assert _ffi.SIGNATURES["ZSTDMI_CCtx_getBatchAsyncPlan"] == (ctypes.c_size_t, [ctypes.c_void_p, size_p, size_p, size_p])
    # the struct is six size_t: maxEntries, srcSizeBound, maxChunks, reserved[3]
    assert ctypes.sizeof(_ffi.CBatchLimits) == 6 * ctypes.sizeof(ctypes.c_size_t)
    assert [f[0] for f in _ffi.CBatchLimits._fields_] == ["maxEntries", "srcSizeBound", "maxChunks", "reserved"]


def test_null_context_and_null_limits_are_generic():
    lib = _ffi.load()
    generic = ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert _code(lib.ZSTDMI_CCtx_prepareBatchAsyncLimits(None, ctypes.byref(_limits()))) == generic
    out = ctypes.c_size_t(0)
    assert _code(lib.ZSTDMI_CCtx_getBatchAsyncPlan(None, ctypes.byref(out), None, None)) == generic
    ctx = lib.ZSTD_createCCtx()
    try:
        assert _code(lib.ZSTDMI_CCtx_prepareBatchAsyncLimits(ctx, None)) == generic
    finally:
        lib.ZSTD_freeCCtx(ctx)


def test_out_of_bound_limits_are_answered_without_a_device():
    lib = _ffi.load()
    bound = ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    ctx = lib.ZSTD_createCCtx()
    try:
        for bad in (dict(maxEntries=0), dict(maxEntries=16385), dict(srcSizeBound=0), dict(srcSizeBound=FOUR_MIB), dict(srcSizeBound=FOUR_MIB + 1),
                    dict(maxChunks=16385), dict(reserved=(1, 0, 0)), dict(reserved=(0, 1, 0)), dict(reserved=(0, 0, 1))):
            assert _code(_prepare(lib, ctx, **bad)) == bound, bad
        # the pass limit follows ZSTDMI_CCtx_setPassChunks
        assert lib.ZSTDMI_CCtx_setPassChunks(ctx, 1000) == 0
        assert _code(_prepare(lib, ctx, maxEntries=1001)) == bound
        assert _code(_prepare(lib, ctx, maxEntries=10, maxChunks=1001)) == bound
        assert lib.ZSTDMI_debugHostWaits(ctx) == 0 and lib.ZSTDMI_debugDeviceAllocs(ctx) == 0
    finally:
        lib.ZSTD_freeCCtx(ctx)


def test_device_free_refusals_and_the_plan_without_a_prepare():
    lib = _ffi.load()
    unsupported, stage_wrong = ZSTD_ErrorCode.ZSTD_error_parameter_unsupported, ZSTD_ErrorCode.ZSTD_error_stage_wrong
    ctx = lib.ZSTD_createCCtx()
    try:
        a, b, c = ctypes.c_size_t(7), ctypes.c_size_t(7), ctypes.c_size_t(7)
        assert _code(lib.ZSTDMI_CCtx_getBatchAsyncPlan(ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))) == stage_wrong
        assert (a.value, b.value, c.value) == (7, 7, 7)
        assert lib.ZSTDMI_CCtx_setSeekTable(ctx, 1) == 0
        assert _code(_prepare(lib, ctx)) == unsupported
        assert _code(_prepare(lib, ctx, maxEntries=0)) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound      # (out of bound comes first)
        assert lib.ZSTDMI_CCtx_setSeekTable(ctx, 0) == 0
        prefix = ctypes.create_string_buffer(b"some prefix of more than eight bytes")
        assert lib.ZSTD_CCtx_refPrefix(ctx, prefix, 36) == 0
        assert _code(_prepare(lib, ctx)) == unsupported
        assert _code(_prepare(lib, ctx)) == unsupported           # (the prefix stays pending)
        assert _code(lib.ZSTDMI_CCtx_getBatchAsyncPlan(ctx, None, None, None)) == stage_wrong
        assert _code(lib.ZSTDMI_compressBatchAsync(ctx, 8, 8, 1, 8, 8, 8)) == stage_wrong
        assert lib.ZSTDMI_debugHostWaits(ctx) == 0 and lib.ZSTDMI_debugDeviceAllocs(ctx) == 0
    finally:
        lib.ZSTD_freeCCtx(ctx)


def test_the_first_prepare_still_refuses_a_bound_above_one_block():
    lib = _ffi.load()
    ctx = lib.ZSTD_createCCtx()
    try:
        assert _code(lib.ZSTDMI_CCtx_prepareBatchAsync(ctx, 16, 65537)) == ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
        assert _code(lib.ZSTDMI_CCtx_prepareBatchAsync(ctx, 16385, 4096)) == ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
    finally:
        lib.ZSTD_freeCCtx(ctx)
