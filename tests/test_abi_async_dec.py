"""CPU tests of the C ABI of the batch decoded with no host round trip (include/zstd_mi355x.h "the decompress counterpart"): the symbols
exist and are typed, and the answers that need no device are the header's.  No kernel is launched here."""
import ctypes

from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

SYMBOLS = ["ZSTDMI_batchAsyncWorkspaceD", "ZSTDMI_DCtx_prepareBatchAsync", "ZSTDMI_decompressBatchAsync", "ZSTDMI_debugHostWaitsD",
           "ZSTDMI_debugDeviceAllocsD"]
FIELDS = ["maxEntries", "srcSizeBound", "maxContent", "maxFrames", "maxBlocks", "maxSequences"]


def _code(r):
    assert is_error(r), r
    return get_error_code(r)


def _limits(**kw):
    v = dict(maxEntries=64, srcSizeBound=8192, maxContent=1 << 20, maxFrames=0, maxBlocks=0, maxSequences=0)
    v.update(kw)
    return _ffi.DBatchLimits(*[v[f] for f in FIELDS])


def test_async_symbols_are_exported_and_typed():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    assert [f for f, _ in _ffi.DBatchLimits._fields_] == FIELDS
    assert ctypes.sizeof(_ffi.DBatchLimits) == 6 * ctypes.sizeof(ctypes.c_size_t)
    assert _ffi.SIGNATURES["ZSTDMI_decompressBatchAsync"][0] is ctypes.c_size_t and len(_ffi.SIGNATURES["ZSTDMI_decompressBatchAsync"][1]) == 7
    assert _ffi.SIGNATURES["ZSTDMI_DCtx_prepareBatchAsync"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.POINTER(_ffi.DBatchLimits)])
    assert _ffi.SIGNATURES["ZSTDMI_batchAsyncWorkspaceD"] == (ctypes.c_size_t, [ctypes.POINTER(_ffi.DBatchLimits)])
    for name in SYMBOLS[3:]:
        assert _ffi.SIGNATURES[name][0] is ctypes.c_longlong


def test_debug_counters_without_a_context():
    lib = _ffi.load()
    assert lib.ZSTDMI_debugHostWaitsD(None) == -1
    assert lib.ZSTDMI_debugDeviceAllocsD(None) == -1
    ctx = lib.ZSTD_createDCtx()
    try:
        assert lib.ZSTDMI_debugHostWaitsD(ctx) == 0 and lib.ZSTDMI_debugDeviceAllocsD(ctx) == 0
    finally:
        lib.ZSTD_freeDCtx(ctx)


def test_null_context_is_generic():
    lib = _ffi.load()
    for n in (0, 1):
        assert _code(lib.ZSTDMI_decompressBatchAsync(None, 8, 8, n, 8, 8, 8)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert _code(lib.ZSTDMI_DCtx_prepareBatchAsync(None, ctypes.byref(_limits()))) == ZSTD_ErrorCode.ZSTD_error_GENERIC


def test_answers_that_touch_no_device():
    """n == 0 is 0 whatever the arrays are; a NULL array with entries is GENERIC; without a prepare the call is stage_wrong; the prepare
    refuses NULL limits, limits out of bound, ZSTDMI_DCtx_setLongFrames(2) and a pending prefix before it looks for a device."""
    lib = _ffi.load()
    generic, bound, unsupported = ZSTD_ErrorCode.ZSTD_error_GENERIC, ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound, ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
    ctx = lib.ZSTD_createDCtx()
    try:
        assert lib.ZSTDMI_decompressBatchAsync(ctx, None, None, 0, None, None, None) == 0
        for missing in range(5):
            args = [8, 8, 8, 8, 8]
            args[missing] = None
            assert _code(lib.ZSTDMI_decompressBatchAsync(ctx, args[0], args[1], 2, args[2], args[3], args[4])) == generic
        assert _code(lib.ZSTDMI_decompressBatchAsync(ctx, 8, 8, 1, 8, 8, 8)) == ZSTD_ErrorCode.ZSTD_error_stage_wrong
        assert _code(lib.ZSTDMI_DCtx_prepareBatchAsync(ctx, None)) == generic
        for bad in (dict(maxEntries=0), dict(maxContent=0), dict(srcSizeBound=0), dict(srcSizeBound=(4 << 20) + 1), dict(maxFrames=(1 << 26) + 1),
                    dict(maxBlocks=0xFFFFFFF1), dict(maxEntries=(1 << 26) + 1)):
            assert _code(lib.ZSTDMI_DCtx_prepareBatchAsync(ctx, ctypes.byref(_limits(**bad)))) == bound, bad
        assert lib.ZSTDMI_DCtx_setLongFrames(ctx, 2) == 0
        assert _code(lib.ZSTDMI_DCtx_prepareBatchAsync(ctx, ctypes.byref(_limits()))) == unsupported
        assert lib.ZSTDMI_DCtx_setLongFrames(ctx, 0) == 0
        prefix = ctypes.create_string_buffer(b"a prefix of more than eight bytes")
        assert lib.ZSTD_DCtx_refPrefix(ctx, prefix, 33) == 0
        assert _code(lib.ZSTDMI_DCtx_prepareBatchAsync(ctx, ctypes.byref(_limits()))) == unsupported
        assert _code(lib.ZSTDMI_DCtx_prepareBatchAsync(ctx, ctypes.byref(_limits()))) == unsupported       # (the prefix stays pending)
        assert _code(lib.ZSTDMI_decompressBatchAsync(ctx, 8, 8, 1, 8, 8, 8)) == ZSTD_ErrorCode.ZSTD_error_stage_wrong
        assert lib.ZSTDMI_debugHostWaitsD(ctx) == 0 and lib.ZSTDMI_debugDeviceAllocsD(ctx) == 0
    finally:
        lib.ZSTD_freeDCtx(ctx)


def test_workspace_is_monotone_and_defaults_are_what_they_stand_for():
    lib = _ffi.load()
    ws = lambda **kw: lib.ZSTDMI_batchAsyncWorkspaceD(ctypes.byref(_limits(**kw)))
    assert lib.ZSTDMI_batchAsyncWorkspaceD(None) == 0
    assert ws(maxEntries=0) == 0 and ws(srcSizeBound=(4 << 20) + 1) == 0
    base = dict(maxEntries=64, srcSizeBound=8192, maxContent=1 << 20, maxFrames=100, maxBlocks=300, maxSequences=50000)
    w0 = ws(**base)
    assert w0 > (1 << 20)                   # (the literal scratch alone holds maxContent bytes)
    for f in ("maxEntries", "maxContent", "maxFrames", "maxBlocks", "maxSequences"):
        prev = w0
        for step in (1, 7, 1000):
            w = ws(**dict(base, **{f: base[f] + step}))
            assert w > prev, (f, step)
            prev = w
    assert ws(**dict(base, srcSizeBound=4 << 20)) >= w0        # (the bound sizes nothing: it only admits entries)
    # the defaults: maxFrames = maxEntries, maxBlocks = maxFrames + maxContent / 16384, maxSequences = maxContent / 3 + 64
    e, c = 64, (1 << 20) + 5
    assert ws(maxEntries=e, maxContent=c) == ws(maxEntries=e, maxContent=c, maxFrames=e, maxBlocks=e + c // 16384, maxSequences=c // 3 + 64)
    assert ws(maxEntries=e, maxContent=c, maxFrames=200) == ws(maxEntries=e, maxContent=c, maxFrames=200, maxBlocks=200 + c // 16384, maxSequences=c // 3 + 64)
    assert ws(maxEntries=e, maxContent=c, maxBlocks=5) < ws(maxEntries=e, maxContent=c)
    assert ws(maxEntries=e, maxContent=c, maxSequences=10) < ws(maxEntries=e, maxContent=c)
