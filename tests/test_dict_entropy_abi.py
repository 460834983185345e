"""CPU tests of ZSTDMI_CCtx_setDictEntropy: the symbol and its type, the setter's answers with and without a context, the Python
property, and that the switch touches no device (it is accepted, and sticks, on a machine without one).  No kernel is launched."""
import ctypes

import pytest

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code


def test_symbol_is_exported_and_typed():
    lib = _ffi.load()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(raw, "ZSTDMI_CCtx_setDictEntropy")
    assert "ZSTDMI_CCtx_setDictEntropy" in _ffi.SIGNATURES
    assert lib.ZSTDMI_CCtx_setDictEntropy.restype is ctypes.c_size_t
    assert lib.ZSTDMI_CCtx_setDictEntropy.argtypes == [ctypes.c_void_p, ctypes.c_uint]
    assert isinstance(z.Compressor.dict_entropy, property)


def test_switch_values_and_null_context():
    lib = _ffi.load()
    c = z.Compressor(1)
    assert lib.ZSTDMI_CCtx_setDictEntropy(c.cctx, 1) == 0 and lib.ZSTDMI_CCtx_setDictEntropy(c.cctx, 0) == 0
    for mode in (2, 3, 0x7FFFFFFF, 0xFFFFFFFF):
        assert get_error_code(lib.ZSTDMI_CCtx_setDictEntropy(c.cctx, mode)) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    assert get_error_code(lib.ZSTDMI_CCtx_setDictEntropy(None, 1)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert get_error_code(lib.ZSTDMI_CCtx_setDictEntropy(None, 7)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    c.Dispose()


def test_property_defaults_off_and_is_sticky():
    c = z.Compressor(3)
    assert c.dict_entropy is False
    c.dict_entropy = True
    assert c.dict_entropy is True
    c.Level = 5                     # another parameter does not reset it
    assert c.dict_entropy is True
    c.dict_entropy = 0
    assert c.dict_entropy is False
    c.Dispose()
    with pytest.raises(RuntimeError):
        c.dict_entropy = True


def test_switch_is_accepted_around_a_dictionary_load_without_a_device():
    """the call touches no device: with a formatted dictionary's bytes loaded (validated at first use when no device is bound) the
    switch still answers 0 both ways; compressing then fails loudly where there is no GPU, as every call does"""
    import os
    lib = _ffi.load()
    dic = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_16k.dict"), "rb").read()
    c = z.Compressor(1)
    c.dict_entropy = True
    if lib.ZSTDMI_deviceCount() == 0:
        c.LoadDictionary(dic)
        assert lib.ZSTDMI_CCtx_setDictEntropy(c.cctx, 0) == 0 and lib.ZSTDMI_CCtx_setDictEntropy(c.cctx, 1) == 0
        with pytest.raises(ZstdException) as e:
            c.Wrap(b"hello hello hello hello")
        assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_init_missing
    c.Dispose()
