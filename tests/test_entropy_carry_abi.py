"""CPU tests of ZSTDMI_CCtx_setEntropyCarry and ZSTDMI_debugLastCarryGroups: the symbols and their types, the setter's answers with
and without a context (those of ZSTDMI_CCtx_setDictEntropy), the Python property, and that the switch touches no device (it is
accepted, and sticks, on a machine without one).  No kernel is launched."""
import ctypes

import pytest

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code


def test_symbols_are_exported_and_typed():
    lib = _ffi.load()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(raw, "ZSTDMI_CCtx_setEntropyCarry") and hasattr(raw, "ZSTDMI_debugLastCarryGroups")
    assert "ZSTDMI_CCtx_setEntropyCarry" in _ffi.SIGNATURES and "ZSTDMI_debugLastCarryGroups" in _ffi.SIGNATURES
    assert lib.ZSTDMI_CCtx_setEntropyCarry.restype is ctypes.c_size_t
    assert lib.ZSTDMI_CCtx_setEntropyCarry.argtypes == [ctypes.c_void_p, ctypes.c_uint]
    assert lib.ZSTDMI_debugLastCarryGroups.restype is ctypes.c_longlong
    assert lib.ZSTDMI_debugLastCarryGroups.argtypes == [ctypes.c_void_p]
    assert isinstance(z.Compressor.entropy_carry, property)


def test_switch_values_and_null_context():
    lib = _ffi.load()
    c = z.Compressor(3)
    assert lib.ZSTDMI_CCtx_setEntropyCarry(c.cctx, 1) == 0 and lib.ZSTDMI_CCtx_setEntropyCarry(c.cctx, 0) == 0
    for mode in (2, 3, 0x7FFFFFFF, 0xFFFFFFFF):
        assert get_error_code(lib.ZSTDMI_CCtx_setEntropyCarry(c.cctx, mode)) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    assert get_error_code(lib.ZSTDMI_CCtx_setEntropyCarry(None, 1)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert get_error_code(lib.ZSTDMI_CCtx_setEntropyCarry(None, 7)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    c.Dispose()


def test_counter_without_a_context_and_before_any_call():
    lib = _ffi.load()
    assert lib.ZSTDMI_debugLastCarryGroups(None) == -1
    c = z.Compressor(3)
    assert lib.ZSTDMI_debugLastCarryGroups(c.cctx) == 0
    c.entropy_carry = True
    assert lib.ZSTDMI_debugLastCarryGroups(c.cctx) == 0         # the switch alone walks nothing
    c.Dispose()


def test_property_defaults_off_and_is_sticky():
    c = z.Compressor(3)
    assert c.entropy_carry is False
    c.entropy_carry = True
    assert c.entropy_carry is True
    c.Level = 5                     # another parameter does not reset it
    assert c.entropy_carry is True
    c.entropy_carry = 0
    assert c.entropy_carry is False
    c.Dispose()
    with pytest.raises(RuntimeError):
        c.entropy_carry = True


def test_switch_is_accepted_without_a_device():
    """the call touches no device: the switch answers 0 both ways; compressing then fails loudly where there is no GPU, as every call does"""
    lib = _ffi.load()
    c = z.Compressor(3)
    c.entropy_carry = True
    if lib.ZSTDMI_deviceCount() == 0:
        assert lib.ZSTDMI_CCtx_setEntropyCarry(c.cctx, 0) == 0 and lib.ZSTDMI_CCtx_setEntropyCarry(c.cctx, 1) == 0
        with pytest.raises(ZstdException) as e:
            c.Wrap(b"hello hello hello hello " * 8000)
        assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_init_missing
        assert lib.ZSTDMI_debugLastCarryGroups(c.cctx) == 0
    c.Dispose()
