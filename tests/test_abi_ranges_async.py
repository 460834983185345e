"""CPU tests of the C ABI of gather reads enqueued from the device (include/zstd_mi355x.h "gather reads enqueued from the device"): the
symbols exist and are typed, and the answers that need no device are the header's.  No kernel is launched here."""
import ctypes
import os

from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

SYMBOLS = ["ZSTDMI_rangesAsyncWorkspaceD", "ZSTDMI_DCtx_prepareRangesAsync", "ZSTDMI_DCtx_getRangesAsyncPlan", "ZSTDMI_decompressRangesAsync",
           "ZSTDMI_DRangesLimits"]
FIELDS = ["maxRanges", "maxRangeBytes", "maxContent", "maxFrames", "maxBlocks", "maxSequences"]
GENERIC, STAGE_WRONG = ZSTD_ErrorCode.ZSTD_error_GENERIC, ZSTD_ErrorCode.ZSTD_error_stage_wrong
OUT_OF_BOUND, UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound, ZSTD_ErrorCode.ZSTD_error_parameter_unsupported


def _code(r):
    assert is_error(r), r
    return get_error_code(r)


def _limits(**kw):
    v = dict(maxRanges=64, maxRangeBytes=8192, maxContent=1 << 20, maxFrames=0, maxBlocks=0, maxSequences=0)
    v.update(kw)
    return _ffi.DRangesLimits(*[v[f] for f in FIELDS])


def test_symbols_are_exported_and_typed():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS[:4]:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    header = open(os.path.join(os.path.dirname(os.path.dirname(_ffi.LIB_PATH)), "include", "zstd_mi355x.h")).read()
    for name in SYMBOLS:
        assert name in header, f"{name} is not declared in the header"
    assert [f for f, _ in _ffi.DRangesLimits._fields_] == FIELDS
    assert all(t is ctypes.c_size_t for _, t in _ffi.DRangesLimits._fields_)
    assert ctypes.sizeof(_ffi.DRangesLimits) == 6 * ctypes.sizeof(ctypes.c_size_t)
    # (the struct's fields stand in the header in this order)
    body = header[header.index("typedef struct {", header.index("gather reads enqueued from the device")):header.index("} ZSTDMI_DRangesLimits;")]
    assert [f for f in FIELDS if f in body] == FIELDS and sorted(FIELDS, key=body.index) == FIELDS
    lim = ctypes.POINTER(_ffi.DRangesLimits)
    assert _ffi.SIGNATURES["ZSTDMI_rangesAsyncWorkspaceD"] == (ctypes.c_size_t, [lim, ctypes.c_size_t])
    assert _ffi.SIGNATURES["ZSTDMI_DCtx_prepareRangesAsync"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, lim])
    assert _ffi.SIGNATURES["ZSTDMI_DCtx_getRangesAsyncPlan"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_ulonglong)])
    assert _ffi.SIGNATURES["ZSTDMI_decompressRangesAsync"][0] is ctypes.c_size_t and len(_ffi.SIGNATURES["ZSTDMI_decompressRangesAsync"][1]) == 7


def test_null_context_is_generic():
    lib = _ffi.load()
    for n in (0, 1):
        assert _code(lib.ZSTDMI_decompressRangesAsync(None, 8, 8, n, 8, 8, 8)) == GENERIC
    assert _code(lib.ZSTDMI_DCtx_prepareRangesAsync(None, 8, 100, ctypes.byref(_limits()))) == GENERIC
    assert _code(lib.ZSTDMI_DCtx_getRangesAsyncPlan(None, None, None)) == GENERIC


def test_answers_that_touch_no_device():
    """n == 0 is 0 whatever the arrays are; a NULL array with entries is GENERIC; without a prepare the call and the plan getter are
    stage_wrong; the prepare refuses NULL limits, every limit out of bound, ZSTDMI_DCtx_setLongFrames(2) and a pending prefix before
    it looks for a device — the counters of waits and allocations stay at zero."""
    lib = _ffi.load()
    ctx = lib.ZSTD_createDCtx()
    try:
        assert lib.ZSTDMI_decompressRangesAsync(ctx, None, None, 0, None, None, None) == 0
        assert lib.ZSTDMI_decompressRangesAsync(ctx, 8, 8, 0, 8, 8, 8) == 0
        for missing in range(5):
            args = [8, 8, 8, 8, 8]
            args[missing] = None
            assert _code(lib.ZSTDMI_decompressRangesAsync(ctx, args[0], args[1], 2, args[2], args[3], args[4])) == GENERIC
        assert _code(lib.ZSTDMI_decompressRangesAsync(ctx, 8, 8, 1, 8, 8, 8)) == STAGE_WRONG
        n, total = ctypes.c_size_t(7), ctypes.c_ulonglong(7)
        assert _code(lib.ZSTDMI_DCtx_getRangesAsyncPlan(ctx, ctypes.byref(n), ctypes.byref(total))) == STAGE_WRONG
        assert (n.value, total.value) == (7, 7)
        assert _code(lib.ZSTDMI_DCtx_prepareRangesAsync(ctx, 8, 100, None)) == GENERIC
        for bad in (dict(maxRanges=0), dict(maxContent=0), dict(maxRangeBytes=0), dict(maxRangeBytes=(4 << 20) + 1), dict(maxRanges=0xFFFFFFF1),
                    dict(maxContent=(1 << 48) + 1), dict(maxFrames=(1 << 26) + 1), dict(maxBlocks=0xFFFFFFF1), dict(maxSequences=(1 << 48) + 1),
                    dict(maxContent=1 << 48, maxFrames=1)):         # (the default for the blocks leaves the index range)
            assert _code(lib.ZSTDMI_DCtx_prepareRangesAsync(ctx, 8, 100, ctypes.byref(_limits(**bad)))) == OUT_OF_BOUND, bad
        assert lib.ZSTDMI_DCtx_setLongFrames(ctx, 2) == 0
        assert _code(lib.ZSTDMI_DCtx_prepareRangesAsync(ctx, 8, 100, ctypes.byref(_limits()))) == UNSUPPORTED
        assert lib.ZSTDMI_DCtx_setLongFrames(ctx, 0) == 0
        prefix = ctypes.create_string_buffer(b"a prefix of more than eight bytes")
        assert lib.ZSTD_DCtx_refPrefix(ctx, prefix, 33) == 0
        assert _code(lib.ZSTDMI_DCtx_prepareRangesAsync(ctx, 8, 100, ctypes.byref(_limits()))) == UNSUPPORTED
        assert _code(lib.ZSTDMI_DCtx_prepareRangesAsync(ctx, 8, 100, ctypes.byref(_limits()))) == UNSUPPORTED      # (the prefix stays pending)
        assert _code(lib.ZSTDMI_decompressRangesAsync(ctx, 8, 8, 1, 8, 8, 8)) == STAGE_WRONG
        assert lib.ZSTDMI_debugHostWaitsD(ctx) == 0 and lib.ZSTDMI_debugDeviceAllocsD(ctx) == 0
    finally:
        lib.ZSTD_freeDCtx(ctx)


def test_workspace_is_monotone_and_defaults_are_what_they_stand_for():
    lib = _ffi.load()
    ws = lambda entries=1000, **kw: lib.ZSTDMI_rangesAsyncWorkspaceD(ctypes.byref(_limits(**kw)), entries)
    assert lib.ZSTDMI_rangesAsyncWorkspaceD(None, 1000) == 0
    assert ws(maxRanges=0) == 0 and ws(maxContent=0) == 0 and ws(maxRangeBytes=0) == 0 and ws(maxRangeBytes=(4 << 20) + 1) == 0
    assert ws(maxFrames=(1 << 26) + 1) == 0 and ws(maxBlocks=0xFFFFFFF1) == 0
    assert ws(entries=(1 << 27) + 1) == 0 and ws(entries=(1 << 26) + 1) == 0       # (a count no table has; maxFrames 0 = a count beyond the lists)
    base = dict(maxRanges=64, maxRangeBytes=8192, maxContent=1 << 20, maxFrames=100, maxBlocks=300, maxSequences=50000)
    w0 = ws(**base)
    assert w0 > 2 * (1 << 20)                # (the arena and the literal scratch hold maxContent bytes each)
    for f in ("maxRanges", "maxContent", "maxFrames", "maxBlocks", "maxSequences"):
        prev = w0
        for step in (1, 7, 1000):
            w = ws(**dict(base, **{f: base[f] + step}))
            assert w > prev, (f, step)
            prev = w
    assert ws(**dict(base, maxRangeBytes=4 << 20)) >= w0         # (it sizes a grid, no buffer)
    prev = 0
    for entries in (0, 1, 99, 100, 101, 1023, 1024, 1025, 100000):
        for kw in (base, dict(base, maxFrames=0)):
            assert ws(entries, **kw) > 0
        w = ws(entries, **base)
        assert w >= prev, entries
        prev = w
    assert ws(1025, **base) > ws(1, **base) and ws(100000, **base) > ws(1025, **base)
    assert ws(2000, **dict(base, maxFrames=0)) > ws(1000, **dict(base, maxFrames=0))
    # the defaults: maxFrames = the table's entries, maxBlocks = maxFrames + maxContent / 16384, maxSequences = maxContent / 3 + 64
    n, c = 777, (1 << 20) + 5
    assert ws(n, maxContent=c) == ws(n, maxContent=c, maxFrames=n, maxBlocks=n + c // 16384, maxSequences=c // 3 + 64)
    assert ws(n, maxContent=c, maxFrames=200) == ws(n, maxContent=c, maxFrames=200, maxBlocks=200 + c // 16384, maxSequences=c // 3 + 64)
    assert ws(n, maxContent=c, maxBlocks=5) < ws(n, maxContent=c)
    assert ws(n, maxContent=c, maxSequences=10) < ws(n, maxContent=c)
