"""CPU tests of the ZSTDMI_CCtx_setDictIndex switch: its argument checks, its debug counter without a context, and the Python property.
No device is bound and no kernel is launched: the setter touches no device."""
from zstdsharp_amd import _ffi
from zstdsharp_amd.compressor import Compressor
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error


def test_setter_argument_checks():
    lib = _ffi.load()
    r = lib.ZSTDMI_CCtx_setDictIndex(None, 1)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    cctx = lib.ZSTD_createCCtx()
    assert cctx
    try:
        r = lib.ZSTDMI_CCtx_setDictIndex(cctx, 2)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
        for mode in (1, 0, 1, 1, 0):
            assert lib.ZSTDMI_CCtx_setDictIndex(cctx, mode) == 0
        # a raw-content dictionary is held on the host until a call needs it: the counter answers from there, no device bound
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 0
        raw = bytes(range(200)) * 3
        assert lib.ZSTD_CCtx_loadDictionary(cctx, raw, len(raw)) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 0           # (switch off)
        assert lib.ZSTDMI_CCtx_setDictIndex(cctx, 1) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == len(raw)
        assert lib.ZSTD_CCtx_loadDictionary(cctx, raw, 7) == 0  # (below 8 bytes: no dictionary)
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 0
        assert lib.ZSTD_CCtx_loadDictionary(cctx, None, 0) == 0
        assert lib.ZSTDMI_debugDictIndexed(cctx) == 0
    finally:
        lib.ZSTD_freeCCtx(cctx)


def test_debug_counter_without_a_context():
    assert _ffi.load().ZSTDMI_debugDictIndexed(None) == -1


def test_python_property_round_trips():
    c = Compressor(1)
    try:
        assert c.dict_index is False
        c.dict_index = True
        assert c.dict_index is True
        c.dict_index = False
        assert c.dict_index is False
    finally:
        c.Dispose()
