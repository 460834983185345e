"""CPU tests of ZSTDMI_CCtx_setDictIndexStrategy, the reach of ZSTDMI_CCtx_setDictIndex over the strategies: its argument checks,
what the debug counter answers under either setting, and the Python property.  No device is bound and no kernel is launched: the
setter touches no device."""
import pytest

from zstdsharp_amd import _ffi
from zstdsharp_amd.compressor import Compressor
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error


def test_setter_argument_checks():
    lib = _ffi.load()
    r = lib.ZSTDMI_CCtx_setDictIndexStrategy(None, 1)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    cctx = lib.ZSTD_createCCtx()
    assert cctx
    try:
        for bad in (0, 3, 9):       # (3 and above: kept for the chain finder)
            r = lib.ZSTDMI_CCtx_setDictIndexStrategy(cctx, bad)
            assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound, bad
        for v in (1, 2, 2, 1, 2, 1, 1):
            assert lib.ZSTDMI_CCtx_setDictIndexStrategy(cctx, v) == 0, v
        # the switch itself keeps its own range: 2 is no mode of it, whatever the reach is set to
        assert lib.ZSTDMI_CCtx_setDictIndexStrategy(cctx, 2) == 0
        r = lib.ZSTDMI_CCtx_setDictIndex(cctx, 2)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    finally:
        lib.ZSTD_freeCCtx(cctx)


@pytest.mark.parametrize("setting", [1, 2])
@pytest.mark.parametrize("setting_first", [False, True])
def test_debug_counter_answers_as_before(setting, setting_first):
    """What the index covers is a matter of the switch and the dictionary, not of how far up the strategies it is used."""
    lib = _ffi.load()
    cctx = lib.ZSTD_createCCtx()
    assert cctx
    try:
        raw = bytes(range(200)) * 3
        if setting_first:
            assert lib.ZSTDMI_CCtx_setDictIndexStrategy(cctx, setting) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 0
        assert lib.ZSTD_CCtx_loadDictionary(cctx, raw, len(raw)) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 0           # (switch off: the setting alone indexes nothing)
        assert lib.ZSTDMI_CCtx_setDictIndex(cctx, 1) == 0
        if not setting_first:
            assert lib.ZSTDMI_CCtx_setDictIndexStrategy(cctx, setting) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == len(raw)
        assert lib.ZSTDMI_CCtx_setDictIndexStrategy(cctx, 3 - setting) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == len(raw)
        assert lib.ZSTD_CCtx_loadDictionary(cctx, raw, 7) == 0  # (below 8 bytes: no dictionary)
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 0
        big = bytes(250000)
        assert lib.ZSTD_CCtx_loadDictionary(cctx, big, len(big)) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 188 << 10
        assert lib.ZSTDMI_CCtx_setDictIndex(cctx, 0) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 0
    finally:
        lib.ZSTD_freeCCtx(cctx)
    assert lib.ZSTDMI_debugDictIndexed(None) == -1


def test_python_property_round_trips():
    c = Compressor()
    try:
        assert c.dict_index_strategy == 1
        assert c.dict_index is False
        c.dict_index_strategy = 2
        assert c.dict_index_strategy == 2
        assert c.dict_index is False                # (the reach is not the switch)
        c.dict_index = True
        assert c.dict_index is True and c.dict_index_strategy == 2
        for bad in (0, 3):
            with pytest.raises(ZstdException):
                c.dict_index_strategy = bad
            assert c.dict_index_strategy == 2       # (a refused value leaves the property where it was)
        c.dict_index_strategy = 1
        assert c.dict_index_strategy == 1 and c.dict_index is True
    finally:
        c.Dispose()
