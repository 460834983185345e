"""CPU tests of ZSTDMI_CCtx_setSingleFrame: the symbol and its type, the header's declaration, the setter's answers with and without a
context, the Python property and the CompressionStream argument, and that the switch touches no device (it is accepted, and sticks,
on a machine without one).  No kernel is launched."""
import ctypes
import io
import os

import pytest

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_typed():
    lib = _ffi.load()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(raw, "ZSTDMI_CCtx_setSingleFrame")
    assert _ffi.SIGNATURES["ZSTDMI_CCtx_setSingleFrame"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_uint])
    assert lib.ZSTDMI_CCtx_setSingleFrame.restype is ctypes.c_size_t
    assert lib.ZSTDMI_CCtx_setSingleFrame.argtypes == [ctypes.c_void_p, ctypes.c_uint]
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    assert "size_t ZSTDMI_CCtx_setSingleFrame(ZSTD_CCtx* cctx, unsigned mode);" in header
    assert isinstance(z.Compressor.single_frame, property)


def test_switch_values_and_null_context():
    lib = _ffi.load()
    c = z.Compressor(1)
    assert lib.ZSTDMI_CCtx_setSingleFrame(c.cctx, 1) == 0 and lib.ZSTDMI_CCtx_setSingleFrame(c.cctx, 0) == 0
    for mode in (2, 3, 0x7FFFFFFF, 0xFFFFFFFF):
        assert get_error_code(lib.ZSTDMI_CCtx_setSingleFrame(c.cctx, mode)) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    assert get_error_code(lib.ZSTDMI_CCtx_setSingleFrame(None, 1)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert get_error_code(lib.ZSTDMI_CCtx_setSingleFrame(None, 2)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    c.Dispose()


def test_property_defaults_off_and_is_sticky():
    c = z.Compressor(3)
    assert c.single_frame is False
    c.single_frame = True
    assert c.single_frame is True
    c.Level = 5                     # another parameter does not reset it
    assert c.single_frame is True
    c.single_frame = 0
    assert c.single_frame is False
    c.Dispose()
    with pytest.raises(RuntimeError):
        c.single_frame = True


def test_compression_stream_argument_sets_the_compressors_switch():
    c = z.Compressor(3)
    z.CompressionStream(io.BytesIO(), compressor=c)
    assert c.single_frame is False                      # None leaves the compressor as it is
    z.CompressionStream(io.BytesIO(), compressor=c, single_frame=True)
    assert c.single_frame is True
    z.CompressionStream(io.BytesIO(), compressor=c)
    assert c.single_frame is True
    z.CompressionStream(io.BytesIO(), compressor=c, single_frame=False)
    assert c.single_frame is False
    c.Dispose()


def test_switch_is_accepted_without_a_device():
    """the call touches no device: the switch answers 0 both ways beside the settings it is later refused with (the refusal belongs to
    the consuming call); compressing then fails loudly where there is no GPU, as every call does"""
    lib = _ffi.load()
    c = z.Compressor(1)
    assert lib.ZSTDMI_CCtx_setSeekTable(c.cctx, 1) == 0
    c.SetParameter(101, 12)                             # ZSTD_c_windowLog
    c.single_frame = True
    assert lib.ZSTDMI_CCtx_setSingleFrame(c.cctx, 0) == 0 and lib.ZSTDMI_CCtx_setSingleFrame(c.cctx, 1) == 0
    if lib.ZSTDMI_deviceCount() == 0:
        with pytest.raises(ZstdException) as e:
            c.Wrap(b"hello hello hello hello" * 4000)
        assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_init_missing
    c.Dispose()
