"""CPU tests of ZSTDMI_CCtx_setFarOffsets and ZSTDMI_debugLastFarPlane: the symbols and their types, the header's declarations, the
setter's four answers (0 for off and on, parameter_outOfBound for any other mode, GENERIC without a context), the Python property, and
that the switch touches no device (it is accepted, and sticks, on a machine without one).  No kernel is launched."""
import ctypes
import os

import pytest

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_typed():
    lib = _ffi.load()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(raw, "ZSTDMI_CCtx_setFarOffsets") and hasattr(raw, "ZSTDMI_debugLastFarPlane")
    assert _ffi.SIGNATURES["ZSTDMI_CCtx_setFarOffsets"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_uint])
    assert lib.ZSTDMI_CCtx_setFarOffsets.restype is ctypes.c_size_t
    assert lib.ZSTDMI_CCtx_setFarOffsets.argtypes == [ctypes.c_void_p, ctypes.c_uint]
    assert _ffi.SIGNATURES["ZSTDMI_debugLastFarPlane"] == (ctypes.c_int, [ctypes.c_void_p])
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    assert "size_t ZSTDMI_CCtx_setFarOffsets(ZSTD_CCtx* cctx, unsigned mode);" in header
    assert "int ZSTDMI_debugLastFarPlane(const ZSTD_DCtx* dctx);" in header
    assert isinstance(z.Compressor.far_offsets, property)


def test_the_setters_four_answers():
    lib = _ffi.load()
    c = z.Compressor(1)
    assert lib.ZSTDMI_CCtx_setFarOffsets(c.cctx, 0) == 0
    assert lib.ZSTDMI_CCtx_setFarOffsets(c.cctx, 1) == 0
    for mode in (2, 3, 0x7FFFFFFF, 0xFFFFFFFF):
        assert get_error_code(lib.ZSTDMI_CCtx_setFarOffsets(c.cctx, mode)) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    assert get_error_code(lib.ZSTDMI_CCtx_setFarOffsets(None, 1)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert get_error_code(lib.ZSTDMI_CCtx_setFarOffsets(None, 2)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    c.Dispose()


def test_property_defaults_off_and_is_sticky():
    c = z.Compressor(3)
    assert c.far_offsets is False
    c.far_offsets = True
    assert c.far_offsets is True
    c.Level = 5                     # another parameter does not reset it
    c.single_frame = True
    c.sliding_ldm = True
    assert c.far_offsets is True
    c.far_offsets = 0
    assert c.far_offsets is False and c.sliding_ldm is True and c.single_frame is True
    c.Dispose()
    with pytest.raises(RuntimeError):
        c.far_offsets = True


def test_a_refused_mode_leaves_the_switch_as_it_was():
    lib = _ffi.load()
    c = z.Compressor(1)
    c.far_offsets = True
    assert get_error_code(lib.ZSTDMI_CCtx_setFarOffsets(c.cctx, 7)) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    assert c.far_offsets is True
    c.Dispose()


def test_far_plane_hook_without_a_context_and_before_any_call():
    lib = _ffi.load()
    assert lib.ZSTDMI_debugLastFarPlane(None) == -1
    d = z.Decompressor()
    assert lib.ZSTDMI_debugLastFarPlane(d.dctx) == 0
    d.Dispose()
