"""CPU tests of the long-distance-matching parameters (ZSTD_c_enableLongDistanceMatching .. ZSTD_c_ldmHashRateLog): bounds as
ZSTD_cParam_getBounds (U/ZstdCompress.cs:560-595), values read back as set, the documented hashRateLog floor.  No kernel runs."""
import ctypes

import pytest

from zstdsharp_amd import _ffi
from zstdsharp_amd.compressor import (ZSTD_c_enableLongDistanceMatching, ZSTD_c_ldmBucketSizeLog, ZSTD_c_ldmHashLog,
                                      ZSTD_c_ldmHashRateLog, ZSTD_c_ldmMinMatch, ZSTD_ps_auto, ZSTD_ps_disable, ZSTD_ps_enable)
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

BOUNDS = {
    ZSTD_c_enableLongDistanceMatching: (0, 2),
    ZSTD_c_ldmHashLog: (6, 30),
    ZSTD_c_ldmMinMatch: (4, 4096),
    ZSTD_c_ldmBucketSizeLog: (1, 8),
    ZSTD_c_ldmHashRateLog: (0, 25),
}


@pytest.fixture
def cctx():
    lib = _ffi.load()
    c = lib.ZSTD_createCCtx()
    yield lib, c
    lib.ZSTD_freeCCtx(c)


def _get(lib, c, p):
    v = ctypes.c_int(-1)
    assert lib.ZSTD_CCtx_getParameter(c, p, ctypes.byref(v)) == 0
    return v.value


def test_switch_values_and_defaults(cctx):
    lib, c = cctx
    assert (ZSTD_ps_auto, ZSTD_ps_enable, ZSTD_ps_disable) == (0, 1, 2)
    for p in BOUNDS:
        assert _get(lib, c, p) == 0, "every LDM parameter starts at 0 (auto / from the window)"
    for v in (ZSTD_ps_enable, ZSTD_ps_disable, ZSTD_ps_auto):
        assert lib.ZSTD_CCtx_setParameter(c, ZSTD_c_enableLongDistanceMatching, v) == v
        assert _get(lib, c, ZSTD_c_enableLongDistanceMatching) == v


@pytest.mark.parametrize("param", sorted(BOUNDS))
def test_in_bound_values_are_accepted_and_read_back(cctx, param):
    lib, c = cctx
    lo, hi = BOUNDS[param]
    values = {0, lo, hi, (lo + hi) // 2}
    if param == ZSTD_c_ldmHashRateLog:
        values = {0, 5, 7, 12, 25}
    for v in sorted(values):
        r = lib.ZSTD_CCtx_setParameter(c, param, v)
        assert not is_error(r), (param, v, get_error_code(r))
        assert r == v
        assert _get(lib, c, param) == v


@pytest.mark.parametrize("param", sorted(BOUNDS))
def test_out_of_bound_values_are_refused(cctx, param):
    lib, c = cctx
    lo, hi = BOUNDS[param]
    bad = [-1, hi + 1, 1 << 20]
    if lo > 1:
        bad.append(lo - 1)
    lib.ZSTD_CCtx_setParameter(c, param, lo)
    for v in bad:
        r = lib.ZSTD_CCtx_setParameter(c, param, v)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound, (param, v)
        assert _get(lib, c, param) == lo, "a refused value leaves the parameter as it was"


def test_hash_rate_log_floor_is_unsupported_not_ignored(cctx):
    """hashRateLog 1..4 (a split every 2..16 bytes) is more than the split workspace holds: parameter_unsupported"""
    lib, c = cctx
    assert lib.ZSTD_CCtx_setParameter(c, ZSTD_c_ldmHashRateLog, 9) == 9
    for v in (1, 2, 3, 4):
        r = lib.ZSTD_CCtx_setParameter(c, ZSTD_c_ldmHashRateLog, v)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_unsupported, v
        assert _get(lib, c, ZSTD_c_ldmHashRateLog) == 9
