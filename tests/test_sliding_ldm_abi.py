"""CPU tests of ZSTDMI_CCtx_setSlidingLdm: the symbol and its type, the header's declaration, the setter's answers with and without a
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
    assert hasattr(raw, "ZSTDMI_CCtx_setSlidingLdm")
    assert _ffi.SIGNATURES["ZSTDMI_CCtx_setSlidingLdm"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_uint])
    assert lib.ZSTDMI_CCtx_setSlidingLdm.restype is ctypes.c_size_t
    assert lib.ZSTDMI_CCtx_setSlidingLdm.argtypes == [ctypes.c_void_p, ctypes.c_uint]
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    assert "size_t ZSTDMI_CCtx_setSlidingLdm(ZSTD_CCtx* cctx, unsigned mode);" in header
    assert isinstance(z.Compressor.sliding_ldm, property)


def test_switch_values_and_null_context():
    lib = _ffi.load()
    c = z.Compressor(1)
    assert lib.ZSTDMI_CCtx_setSlidingLdm(c.cctx, 1) == 0 and lib.ZSTDMI_CCtx_setSlidingLdm(c.cctx, 0) == 0
    for mode in (2, 3, 0x7FFFFFFF, 0xFFFFFFFF):
        assert get_error_code(lib.ZSTDMI_CCtx_setSlidingLdm(c.cctx, mode)) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    assert get_error_code(lib.ZSTDMI_CCtx_setSlidingLdm(None, 1)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert get_error_code(lib.ZSTDMI_CCtx_setSlidingLdm(None, 2)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    c.Dispose()


def test_property_defaults_off_and_is_sticky():
    c = z.Compressor(3)
    assert c.sliding_ldm is False
    c.sliding_ldm = True
    assert c.sliding_ldm is True
    c.Level = 5                     # another parameter does not reset it
    c.single_frame = True           # nor does the switch it works under
    assert c.sliding_ldm is True
    c.sliding_ldm = 0
    assert c.sliding_ldm is False and c.single_frame is True
    c.Dispose()
    with pytest.raises(RuntimeError):
        c.sliding_ldm = True


def test_compression_stream_argument_sets_the_compressors_switch():
    c = z.Compressor(3)
    z.CompressionStream(io.BytesIO(), compressor=c)
    assert c.sliding_ldm is False                       # None leaves the compressor as it is
    z.CompressionStream(io.BytesIO(), compressor=c, single_frame=True, sliding_ldm=True)
    assert c.sliding_ldm is True and c.single_frame is True
    z.CompressionStream(io.BytesIO(), compressor=c)
    assert c.sliding_ldm is True
    z.CompressionStream(io.BytesIO(), compressor=c, sliding_ldm=False)
    assert c.sliding_ldm is False and c.single_frame is True
    c.Dispose()


def test_switch_is_accepted_without_a_device():
    """the call touches no device: the switch answers 0 both ways beside the settings it is later refused with (the refusal belongs to
    the consuming call); compressing then fails loudly where there is no GPU, as every call does"""
    lib = _ffi.load()
    c = z.Compressor(1)
    assert lib.ZSTDMI_CCtx_setSeekTable(c.cctx, 1) == 0
    c.SetParameter(101, 29)                             # ZSTD_c_windowLog
    c.SetParameter(160, 1)                              # ZSTD_c_enableLongDistanceMatching = ZSTD_ps_enable
    c.single_frame = True
    c.sliding_ldm = True
    assert lib.ZSTDMI_CCtx_setSlidingLdm(c.cctx, 0) == 0 and lib.ZSTDMI_CCtx_setSlidingLdm(c.cctx, 1) == 0
    if lib.ZSTDMI_deviceCount() == 0:
        with pytest.raises(ZstdException) as e:
            c.Wrap(b"hello hello hello hello" * 4000)
        assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_init_missing
    c.Dispose()
