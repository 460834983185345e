"""CPU tests of the C ABI of content-defined cuts (include/zstd_mi355x.h "Content-defined cuts"): the symbols exist, are typed and
declared; the setter answers without a device; ZSTDMI_contentCutsBound is the formula and covers ZSTDMI_packBound of the piece lists the
rule allows; NULL handling; the header states rule version 1.  No kernel is launched."""
import ctypes
import json
import os

import pytest

import content_cuts_cases as cc
import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zstd_mi355x.h")
E = ZSTD_ErrorCode
s, v, u, ll, ps = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint, ctypes.c_longlong, ctypes.POINTER(ctypes.c_size_t)
SYMBOLS = {
    "ZSTDMI_CCtx_setContentCuts": (s, [v, u]),
    "ZSTDMI_contentCutsBound": (s, [s, u]),
    "ZSTDMI_contentCuts": (s, [v, v, s, u, ps, s, ps]),
    "ZSTDMI_debugLastContentCuts": (ll, [v]),
}


def sizes_of(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


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
    text = " ".join(open(HEADER).read().split())
    for line in ["size_t ZSTDMI_CCtx_setContentCuts(ZSTD_CCtx* cctx, unsigned avgLog);",
                 "size_t ZSTDMI_contentCutsBound(size_t srcSize, unsigned avgLog);",
                 "size_t ZSTDMI_contentCuts(ZSTD_CCtx* cctx, const void* d_src, size_t srcSize, unsigned avgLog, size_t* pieceSizes, size_t capacity, size_t* nPieces);",
                 "long long ZSTDMI_debugLastContentCuts(const ZSTD_CCtx* cctx);"]:
        assert line in text, line
    assert isinstance(z.Compressor.content_cuts, property) and callable(z.content_cuts)


def test_header_states_rule_version_1():
    text = " ".join(open(HEADER).read().split())
    assert "The cut rule, version 1" in text
    for part in ["gear[i] = splitmix64(i)", "h = (h << 1) + gear[byte]", "bits = avgLog - 1, min = 1 << (avgLog - 2) and max = 65536",
                 "the smallest candidate e with e - s >= min, if e - s <= max", "avgLog is 12 to 16"]:
        assert part in text, part
    cuts_h = open(os.path.join(ROOT, "zstdsharp_amd", "csrc", "zmi_cuts.h")).read()
    assert "kCutRuleVersion = 1" in cuts_h
    assert json.load(open(cc.GOLDEN))["rule_version"] == 1


def test_setter_answers_without_a_device(cctx):
    lib = _ffi.load()
    for avg_log in (0, 12, 13, 14, 15, 16, 0):
        assert lib.ZSTDMI_CCtx_setContentCuts(cctx, avg_log) == 0
    for avg_log in (1, 5, 11, 17, 64, 0xFFFFFFFF):
        assert get_error_code(lib.ZSTDMI_CCtx_setContentCuts(cctx, avg_log)) == E.ZSTD_error_parameter_outOfBound
    assert get_error_code(lib.ZSTDMI_CCtx_setContentCuts(None, 12)) == E.ZSTD_error_GENERIC
    assert get_error_code(lib.ZSTDMI_CCtx_setContentCuts(None, 3)) == E.ZSTD_error_GENERIC


def test_property_is_sticky_and_refuses_bad_values():
    c = z.Compressor(1)
    assert c.content_cuts == 0
    c.content_cuts = 14
    assert c.content_cuts == 14
    with pytest.raises(ZstdException) as e:
        c.content_cuts = 11
    assert e.value.code == E.ZSTD_error_parameter_outOfBound and c.content_cuts == 14
    c.content_cuts = 0
    assert c.content_cuts == 0
    c.Dispose()


def test_rsyncable_stays_unsupported(cctx):
    lib = _ffi.load()
    ZSTD_c_rsyncable = 500      # ZSTD_c_experimentalParam1
    assert get_error_code(lib.ZSTD_CCtx_setParameter(cctx, ZSTD_c_rsyncable, 1)) == E.ZSTD_error_parameter_unsupported


@pytest.mark.parametrize("avg_log", [12, 13, 14, 15, 16])
def test_bound_is_the_formula(avg_log):
    lib = _ffi.load()
    mn = 1 << (avg_log - 2)
    for n in (0, 1, mn - 1, mn, mn + 1, 4095, 4096, 65535, 65536, 65537, 1 << 20, (1 << 32) - 1, 1 << 40):
        p = n // mn + 1
        assert lib.ZSTDMI_contentCutsBound(n, avg_log) == n + (n >> 8) + 64 * p + 17 + 8 * (n // 4096 + p) == cc.bound(n, avg_log)


def test_bound_errors():
    lib = _ffi.load()
    for avg_log in (0, 1, 11, 17, 0xFFFFFFFF):
        assert get_error_code(lib.ZSTDMI_contentCutsBound(1000, avg_log)) == E.ZSTD_error_parameter_outOfBound
    for n in ((1 << 64) - 1, (1 << 64) - 200, 15 << 60):
        r = lib.ZSTDMI_contentCutsBound(n, 12)
        assert is_error(r) and get_error_code(r) == E.ZSTD_error_srcSize_wrong, n


@pytest.mark.parametrize("avg_log", [12, 14, 16])
def test_bound_covers_the_pack_bound_of_allowed_piece_lists(avg_log):
    lib = _ffi.load()
    mn = 1 << (avg_log - 2)
    lists = []
    for n in (0, 1, mn, 5 * mn, 5 * mn + 1, 100 * mn + mn - 1, 1 << 20):
        lists.append([mn] * (n // mn) + ([n % mn] if n % mn else []))           # all-min, the shortest tail
        lists.append([65536] * (n // 65536) + ([n % 65536] if n % 65536 else []))
    for case in json.load(open(cc.GOLDEN))["cases"]:
        if case["avgLog"] == avg_log:
            lists.append(case["pieces"])
    for kind in ("rand", "text", "flat"):
        lists.append(cc.piece_sizes(cc.base(kind)[:300000], avg_log))
    for pieces in lists:
        assert lib.ZSTDMI_contentCutsBound(sum(pieces), avg_log) >= lib.ZSTDMI_packBound(sizes_of(pieces), len(pieces)), (avg_log, len(pieces))
    # ZSTD_compressBound alone is not enough for small raw pieces: the reason the call has a bound of its own
    assert sum(lib.ZSTD_compressBound(mn) for _ in range(64)) > lib.ZSTD_compressBound(64 * mn) or avg_log > 12


def test_null_handling(cctx):
    lib = _ffi.load()
    sizes, got = sizes_of([0] * 4), ctypes.c_size_t(77)
    assert lib.ZSTDMI_debugLastContentCuts(None) == -1 and lib.ZSTDMI_debugLastContentCuts(cctx) == 0
    assert get_error_code(lib.ZSTDMI_contentCuts(None, None, 0, 12, sizes, 4, ctypes.byref(got))) == E.ZSTD_error_GENERIC
    assert get_error_code(lib.ZSTDMI_contentCuts(cctx, None, 0, 12, sizes, 4, None)) == E.ZSTD_error_GENERIC
    assert get_error_code(lib.ZSTDMI_contentCuts(cctx, None, 0, 12, None, 4, ctypes.byref(got))) == E.ZSTD_error_GENERIC
    for avg_log in (0, 11, 17):
        assert get_error_code(lib.ZSTDMI_contentCuts(cctx, None, 0, avg_log, sizes, 4, ctypes.byref(got))) == E.ZSTD_error_parameter_outOfBound
    assert get_error_code(lib.ZSTDMI_contentCuts(cctx, None, 1 << 32, 12, sizes, 4, ctypes.byref(got))) == E.ZSTD_error_parameter_unsupported
    assert got.value == 0


def test_cut_calls_fail_loudly_without_gpu(cctx):
    """No CPU fallback: without a gfx950 device the chunker and a cut call answer init_missing and touch nothing."""
    lib = _ffi.load()
    if lib.ZSTDMI_deviceCount() > 0:
        pytest.skip("a GPU is visible here")
    sizes, got = sizes_of([0] * 4), ctypes.c_size_t(0)
    assert get_error_code(lib.ZSTDMI_contentCuts(cctx, b"abc", 3, 12, sizes, 4, ctypes.byref(got))) == E.ZSTD_error_init_missing
    assert lib.ZSTDMI_CCtx_setContentCuts(cctx, 12) == 0
    dst = ctypes.create_string_buffer(b"\xA5" * 64, 64)
    assert get_error_code(lib.ZSTD_compress2(cctx, dst, 64, b"abc", 3)) == E.ZSTD_error_init_missing
    assert dst.raw == b"\xA5" * 64
