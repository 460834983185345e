"""CPU tests of the C ABI of the enqueued cuts (include/zstd_mi355x.h "Cuts and digests enqueued from the device"): the symbols exist,
are typed and declared; ZSTDMI_cutsAsyncWorkspace against the arithmetic the header writes down, the default candidate room included;
and every answer the prepare, the plan, the call and the debug hook give before they look for a device, in the stated order.  No kernel
is launched."""
import ctypes
import os

import pytest

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd._ffi import CutLimits
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zstd_mi355x.h")
E = ZSTD_ErrorCode
s, v, u, ull = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint, ctypes.c_ulonglong
ps, pu, pl = ctypes.POINTER(s), ctypes.POINTER(u), ctypes.POINTER(CutLimits)
SYMBOLS = {
    "ZSTDMI_cutsAsyncWorkspace": (s, [pl]),
    "ZSTDMI_CCtx_prepareCutsAsync": (s, [v, pl]),
    "ZSTDMI_CCtx_getCutsAsyncPlan": (s, [v, ps, ps, ps]),
    "ZSTDMI_contentCutsAsync": (s, [v, v, s, v, v, s, v, s, v, v]),
    "ZSTDMI_debugCutSelectParallel": (s, [v, pu, s, ull, u, pu, s, ps]),
    "ZSTDMI_debugCutsAsyncStages": (s, [v, v, s, ctypes.POINTER(ctypes.c_float)]),
}
TOP = (1 << 32) - 1


def code(r):
    return get_error_code(r) if is_error(r) else None


def limits(bound, avg_log=12, kind=0, max_cand=0, reserved=(0, 0, 0)):
    return CutLimits(bound, avg_log, kind, max_cand, (ctypes.c_size_t * 3)(*reserved))


@pytest.fixture
def cctx():
    lib = _ffi.load()
    c = lib.ZSTD_createCCtx()
    yield c
    lib.ZSTD_freeCCtx(c)


def test_symbols_are_exported_typed_and_declared():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, sig in SYMBOLS.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert _ffi.SIGNATURES[name] == sig, name
    assert [f[0] for f in CutLimits._fields_] == ["srcSizeBound", "avgLog", "kind", "maxCandidates", "reserved"] and ctypes.sizeof(CutLimits) == 48
    text = " ".join(open(HEADER).read().split())
    for line in ["typedef struct { size_t srcSizeBound; /* bytes of one call's source, 1 .. 2^32 - 1 */ unsigned avgLog; /* 12 .. 16 */ unsigned kind;",
                 "size_t maxCandidates; /* 0 = 4 * (srcSizeBound >> (avgLog - 1)) + 1024 */ size_t reserved[3]; /* must be 0 */ } ZSTDMI_CutLimits;",
                 "size_t ZSTDMI_cutsAsyncWorkspace(const ZSTDMI_CutLimits* limits);",
                 "size_t ZSTDMI_CCtx_prepareCutsAsync(ZSTD_CCtx* cctx, const ZSTDMI_CutLimits* limits);",
                 "size_t ZSTDMI_CCtx_getCutsAsyncPlan(const ZSTD_CCtx* cctx, size_t* maxPieces, size_t* maxCandidates, size_t* digestSize);",
                 "size_t ZSTDMI_contentCutsAsync(ZSTD_CCtx* cctx, const void* d_src, size_t srcSize, size_t* d_pieceSizes, const void** d_pieceSrcs, "
                 "size_t capacity, void* d_digests, size_t digestsCapacity, size_t* d_nPieces, size_t* d_status);",
                 "size_t ZSTDMI_debugCutSelectParallel(ZSTD_CCtx* cctx, const unsigned* cands, size_t nCand, unsigned long long n, unsigned avgLog, "
                 "unsigned* ends, size_t cap, size_t* nEnds);",
                 "size_t ZSTDMI_debugCutsAsyncStages(ZSTD_CCtx* cctx, const void* d_src, size_t srcSize, float* ms);"]:
        assert line in text, line
    assert callable(z.content_cuts_async) and callable(z.Compressor.PrepareCutsAsync) and callable(z.Compressor.cuts_async_plan)
    # the digests' not-done list no longer names what this call is
    assert "Out of scope: device-array outputs and an enqueued form" not in text


def workspace(bound, avg_log, kind, cand):
    """the header's arithmetic"""
    def r(x):
        return (x + 255) // 256 * 256
    t = (bound + 16383) // 16384
    c = min(cand if cand else 4 * (bound >> (avg_log - 1)) + 1024, (1 << 32) - 16)
    p = bound // (1 << (avg_log - 2)) + 1
    d = {0: 0, 1: 8, 2: 32}[kind]
    b = (c + 2 + 1023) // 1024
    return r(8 * (t + 16) + 256) + r(4 * c + 64) + 4 * r(4 * (c + 2)) + r(c + 2) + 2 * r(4 * (b + 16)) + 256 + r(4 * (p + 1)) + r(p * d)


def test_workspace_is_the_headers_arithmetic():
    lib = _ffi.load()
    for bound in (1, 1023, 16384, 16385, 65536, 1 << 20, (1 << 20) + 1, 1 << 30, TOP):
        for avg_log in (12, 13, 14, 15, 16):
            for kind in (0, 1, 2):
                for cand in (0, 1, 16, 1000, 1 << 20, 1 << 33):
                    assert lib.ZSTDMI_cutsAsyncWorkspace(ctypes.byref(limits(bound, avg_log, kind, cand))) == workspace(bound, avg_log, kind, cand), (bound, avg_log, kind, cand)


def test_default_candidate_room():
    """maxCandidates 0 is 4 * (srcSizeBound >> (avgLog - 1)) + 1024: the workspace equals the one of that number stated, and differs
    from its neighbours'"""
    lib = _ffi.load()
    for bound, avg_log in ((1, 12), (1 << 20, 12), (1 << 20, 16), (1 << 30, 14), (TOP, 12)):
        default = 4 * (bound >> (avg_log - 1)) + 1024
        w = lib.ZSTDMI_cutsAsyncWorkspace(ctypes.byref(limits(bound, avg_log, 2, 0)))
        assert w == lib.ZSTDMI_cutsAsyncWorkspace(ctypes.byref(limits(bound, avg_log, 2, default)))
        assert w < lib.ZSTDMI_cutsAsyncWorkspace(ctypes.byref(limits(bound, avg_log, 2, default + 256)))
        assert w > lib.ZSTDMI_cutsAsyncWorkspace(ctypes.byref(limits(bound, avg_log, 2, default - 256)))


BAD_LIMITS = [limits(0), limits(TOP + 1), limits(1 << 40), limits(1 << 20, 11), limits(1 << 20, 17), limits(1 << 20, 0), limits(1 << 20, 12, 3),
              limits(1 << 20, 12, 0xFFFFFFFF), limits(1 << 20, 12, 0, 0, (1, 0, 0)), limits(1 << 20, 12, 0, 0, (0, 1, 0)), limits(1 << 20, 12, 0, 0, (0, 0, 7))]


def test_prepare_answers_in_their_order(cctx):
    lib = _ffi.load()
    prep, ws = lib.ZSTDMI_CCtx_prepareCutsAsync, lib.ZSTDMI_cutsAsyncWorkspace
    good = limits(1 << 20, 12, 2)
    # a NULL context or NULL limits, whatever else is wrong
    assert code(prep(None, ctypes.byref(good))) == E.ZSTD_error_GENERIC
    assert code(prep(None, ctypes.byref(BAD_LIMITS[0]))) == E.ZSTD_error_GENERIC
    assert code(prep(cctx, None)) == E.ZSTD_error_GENERIC
    assert code(ws(None)) == E.ZSTD_error_GENERIC
    # limits out of bound: in front of several device workers and of the device
    for bad in BAD_LIMITS:
        assert code(prep(cctx, ctypes.byref(bad))) == E.ZSTD_error_parameter_outOfBound
        assert code(ws(ctypes.byref(bad))) == E.ZSTD_error_parameter_outOfBound
    for ok in (limits(1), limits(TOP, 16, 1), limits(1 << 20, 12, 2, 16)):
        assert not is_error(ws(ctypes.byref(ok)))
    # behind them a device is looked for
    r = prep(cctx, ctypes.byref(good))
    if lib.ZSTDMI_deviceCount() > 0:
        assert r == 0
    else:
        assert code(r) == E.ZSTD_error_init_missing
        mp = ctypes.c_size_t(77)
        assert code(lib.ZSTDMI_CCtx_getCutsAsyncPlan(cctx, ctypes.byref(mp), None, None)) == E.ZSTD_error_stage_wrong and mp.value == 77


def test_plan_and_call_answers_without_a_prepare(cctx):
    lib = _ffi.load()
    call, plan = lib.ZSTDMI_contentCutsAsync, lib.ZSTDMI_CCtx_getCutsAsyncPlan
    assert code(plan(None, None, None, None)) == E.ZSTD_error_GENERIC
    assert code(plan(cctx, None, None, None)) == E.ZSTD_error_stage_wrong
    # (the pointers are never read: no prepare, nothing is enqueued)
    a = 0x1000
    assert code(call(None, a, 10, a, a, 4, None, 0, a, a)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, a, 10, a, a, 4, None, 0, None, a)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, a, 10, a, a, 4, None, 0, a, None)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, a, 10, None, a, 4, None, 0, a, a)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, a, 10, a, a, 4, None, 0, a, a)) == E.ZSTD_error_stage_wrong
    assert code(call(cctx, None, 10, None, None, 0, None, 0, a, a)) == E.ZSTD_error_stage_wrong       # (in front of the NULL source)
    assert code(call(cctx, a, TOP + 1, a, a, 4, a, 0, a, a)) == E.ZSTD_error_stage_wrong               # (and of the size)
    ms = (ctypes.c_float * 3)()
    stages = lib.ZSTDMI_debugCutsAsyncStages
    assert code(stages(None, a, 10, ms)) == E.ZSTD_error_GENERIC and code(stages(cctx, a, 10, None)) == E.ZSTD_error_GENERIC
    assert code(stages(cctx, None, 0, ms)) == E.ZSTD_error_stage_wrong


def test_debug_hook_answers_before_a_device(cctx):
    lib = _ffi.load()
    call = lib.ZSTDMI_debugCutSelectParallel
    cands, ends, got = (u * 4)(1024, 2048, 3000, 4096), (u * 8)(), ctypes.c_size_t(77)
    assert code(call(None, cands, 4, 5000, 12, ends, 8, ctypes.byref(got))) == E.ZSTD_error_GENERIC
    assert code(call(cctx, cands, 4, 5000, 12, ends, 8, None)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, None, 4, 5000, 12, ends, 8, ctypes.byref(got))) == E.ZSTD_error_GENERIC
    assert code(call(cctx, cands, 4, 5000, 12, None, 8, ctypes.byref(got))) == E.ZSTD_error_GENERIC
    for avg_log in (0, 11, 17):
        assert code(call(cctx, cands, 4, 5000, avg_log, ends, 8, ctypes.byref(got))) == E.ZSTD_error_parameter_outOfBound
    assert code(call(cctx, cands, 4, TOP + 1, 12, ends, 8, ctypes.byref(got))) == E.ZSTD_error_srcSize_wrong
    assert code(call(cctx, cands, 4, 3, 12, ends, 8, ctypes.byref(got))) == E.ZSTD_error_srcSize_wrong
    assert list(ends) == [0] * 8
    if lib.ZSTDMI_deviceCount() == 0:
        assert code(call(cctx, cands, 4, 5000, 12, ends, 8, ctypes.byref(got))) == E.ZSTD_error_init_missing


def test_python_prepare_refuses_a_bad_kind():
    with z.Compressor(1) as c:
        with pytest.raises(ValueError):
            c.PrepareCutsAsync(1 << 20, 12, kind="md5")
        with pytest.raises(z.ZstdException) as e:
            c.PrepareCutsAsync(1 << 20, 12, kind=7)
        assert e.value.code == E.ZSTD_error_parameter_outOfBound
        with pytest.raises(z.ZstdException) as e:
            c.cuts_async_plan()
        assert e.value.code == E.ZSTD_error_stage_wrong
