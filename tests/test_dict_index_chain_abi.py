"""CPU tests of ZSTDMI_CCtx_setDictIndexChain, the switch that lets ZSTDMI_CCtx_setDictIndex serve the chain finder (levels 5 and up):
its argument checks, what the two debug hooks answer without a device, and the Python property.  No device is bound and no kernel is
launched: the setter touches no device."""
import pytest

from zstdsharp_amd import _ffi
from zstdsharp_amd.compressor import Compressor
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error


def test_symbols_exist():
    lib = _ffi.load()
    assert hasattr(lib, "ZSTDMI_CCtx_setDictIndexChain") and hasattr(lib, "ZSTDMI_debugLastRegionChunks")


def test_setter_argument_checks():
    lib = _ffi.load()
    r = lib.ZSTDMI_CCtx_setDictIndexChain(None, 1)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    cctx = lib.ZSTD_createCCtx()
    assert cctx
    try:
        for bad in (2, 9):
            r = lib.ZSTDMI_CCtx_setDictIndexChain(cctx, bad)
            assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound, bad
        for v in (0, 1, 1, 0, 1):
            assert lib.ZSTDMI_CCtx_setDictIndexChain(cctx, v) == 0, v
        # the reach over the strategies keeps its own range, whatever this switch says
        for bad in (0, 3):
            r = lib.ZSTDMI_CCtx_setDictIndexStrategy(cctx, bad)
            assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound, bad
    finally:
        lib.ZSTD_freeCCtx(cctx)


@pytest.mark.parametrize("order", ["dic", "cid", "icd", "dci"])
def test_no_device_is_touched_and_the_hooks_answer(order):
    """d = ZSTD_CCtx_loadDictionary, i = ZSTDMI_CCtx_setDictIndex, c = ZSTDMI_CCtx_setDictIndexChain, in any order, on a machine that
    may have no device at all: every call succeeds, the index covers what the switch and the dictionary say, no region kernel ran."""
    lib = _ffi.load()
    cctx = lib.ZSTD_createCCtx()
    assert cctx
    try:
        raw = bytes(range(200)) * 3
        for step in order:
            if step == "d":
                assert lib.ZSTD_CCtx_loadDictionary(cctx, raw, len(raw)) == 0
            elif step == "i":
                assert lib.ZSTDMI_CCtx_setDictIndex(cctx, 1) == 0
            else:
                assert lib.ZSTDMI_CCtx_setDictIndexChain(cctx, 1) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == len(raw)
        assert lib.ZSTDMI_debugLastRegionChunks(cctx) == 0
        assert lib.ZSTDMI_CCtx_setDictIndexChain(cctx, 0) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == len(raw)        # (what the index covers is the other switch's matter)
        assert lib.ZSTDMI_CCtx_setDictIndex(cctx, 0) == 0
        assert lib.ZSTDMI_CCtx_setDictIndexChain(cctx, 1) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 0               # (this switch alone indexes nothing)
    finally:
        lib.ZSTD_freeCCtx(cctx)
    assert lib.ZSTDMI_debugLastRegionChunks(None) == -1


def test_python_property_round_trips():
    c = Compressor()
    try:
        assert c.dict_index_chain is False and c.dict_index is False and c.dict_index_strategy == 1
        c.dict_index_chain = True
        assert c.dict_index_chain is True and c.dict_index is False and c.dict_index_strategy == 1
        c.dict_index = True
        c.dict_index_chain = False
        assert c.dict_index_chain is False and c.dict_index is True
        with pytest.raises(ZstdException):
            c.dict_index_strategy = 3
    finally:
        c.Dispose()
