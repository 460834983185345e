"""CPU tests of ZSTD_CCtx_refPrefix / ZSTD_DCtx_refPrefix: the symbols and their types, the host-side answers (NULL contexts, the size
limit, what is refused while a prefix is pending and what cancels it), the Python mirrors, the loud failure without a device, and
the libzstd-made delta fixtures under the oracle's decoder.  No kernel is launched."""
import ctypes
import hashlib
import json
import os

import pytest

import oracle_lib
import prefix_cases
import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GENERIC, UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_GENERIC, ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
INIT_MISSING = ZSTD_ErrorCode.ZSTD_error_init_missing


def manifest():
    return json.load(open(os.path.join(GOLDEN, "manifest_prefix.json")))["cases"]


def test_symbols_are_exported_and_typed():
    lib = _ffi.load()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("ZSTD_CCtx_refPrefix", "ZSTD_DCtx_refPrefix"):
        assert hasattr(raw, name), name
        assert _ffi.SIGNATURES[name] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]), name
        assert getattr(lib, name).restype is ctypes.c_size_t
    for cls in (z.Compressor, z.Decompressor):
        assert callable(cls.RefPrefix) and cls.ref_prefix is cls.RefPrefix


def test_null_contexts_null_prefix_and_the_size_limit():
    lib = _ffi.load()
    some = ctypes.create_string_buffer(64)
    assert get_error_code(lib.ZSTD_CCtx_refPrefix(None, some, 64)) == GENERIC
    assert get_error_code(lib.ZSTD_DCtx_refPrefix(None, some, 64)) == GENERIC
    c, d = z.Compressor(1), z.Decompressor()
    assert lib.ZSTD_CCtx_refPrefix(c.cctx, None, 0) == 0 and lib.ZSTD_DCtx_refPrefix(d.dctx, None, 0) == 0
    assert lib.ZSTD_CCtx_refPrefix(c.cctx, some, 64) == 0 and lib.ZSTD_DCtx_refPrefix(d.dctx, some, 64) == 0
    # above 1 GiB: refused by the size alone (the 64 bytes behind the pointer are never read)
    for size in ((1 << 30) + 1, 1 << 40):
        assert get_error_code(lib.ZSTD_CCtx_refPrefix(c.cctx, some, size)) == UNSUPPORTED
        assert get_error_code(lib.ZSTD_DCtx_refPrefix(d.dctx, some, size)) == UNSUPPORTED
    assert lib.ZSTD_CCtx_refPrefix(c.cctx, some, 1 << 30) == 0 and lib.ZSTD_DCtx_refPrefix(d.dctx, some, 1 << 30) == 0
    assert lib.ZSTD_CCtx_refPrefix(c.cctx, None, 0) == 0 and lib.ZSTD_DCtx_refPrefix(d.dctx, None, 0) == 0
    c.Dispose(); d.Dispose()


def _cstream(lib, c):
    """ZSTD_compressStream2 with nothing to do: a hint, or the error a pending prefix makes it return"""
    out = ctypes.create_string_buffer(64)
    ob, ib = ZSTD_outBuffer(ctypes.cast(out, ctypes.c_void_p), 64, 0), ZSTD_inBuffer(None, 0, 0)
    return lib.ZSTD_compressStream2(c.cctx, ctypes.byref(ob), ctypes.byref(ib), 0)


def _dstream(lib, d):
    out = ctypes.create_string_buffer(64)
    ob, ib = ZSTD_outBuffer(ctypes.cast(out, ctypes.c_void_p), 64, 0), ZSTD_inBuffer(None, 0, 0)
    return lib.ZSTD_decompressStream(d.dctx, ctypes.byref(ob), ctypes.byref(ib))


def test_pending_prefix_is_refused_by_the_stream_calls_and_cancelled_by_load_dictionary():
    lib = _ffi.load()
    prefix = bytes(range(256)) * 4
    c, d = z.Compressor(1), z.Decompressor()
    assert not is_error(_cstream(lib, c)) and not is_error(_dstream(lib, d))
    c.RefPrefix(prefix); d.RefPrefix(prefix)
    assert get_error_code(_cstream(lib, c)) == UNSUPPORTED and get_error_code(_dstream(lib, d)) == UNSUPPORTED
    # still pending after the refusal; ZSTD_*_loadDictionary cancels it
    assert get_error_code(_cstream(lib, c)) == UNSUPPORTED and get_error_code(_dstream(lib, d)) == UNSUPPORTED
    c.LoadDictionary(b"a raw-content dictionary of more than eight bytes")
    d.LoadDictionary(b"a raw-content dictionary of more than eight bytes")
    assert not is_error(_cstream(lib, c)) and not is_error(_dstream(lib, d))
    # a later prefix replaces an earlier one; NULL / 0 cancels it
    c.RefPrefix(prefix); c.RefPrefix(prefix[:100]); d.RefPrefix(prefix); d.RefPrefix(prefix[:100])
    assert get_error_code(_cstream(lib, c)) == UNSUPPORTED and get_error_code(_dstream(lib, d)) == UNSUPPORTED
    c.RefPrefix(None); d.RefPrefix(b"")
    assert not is_error(_cstream(lib, c)) and not is_error(_dstream(lib, d))
    c.Dispose(); d.Dispose()


def test_python_mirrors_keep_the_prefix_alive_until_the_consuming_call_returned():
    lib = _ffi.load()
    c, d = z.Compressor(1), z.Decompressor()
    p = bytearray(b"0123456789" * 50)
    c.RefPrefix(p); d.RefPrefix(memoryview(p))
    assert c._prefix_keep is not None and d._prefix_keep is not None
    frame = bytes([0x28, 0xB5, 0x2F, 0xFD, 0x20, 0x01, 0x09, 0x00, 0x00, 0x41])      # content "A": a raw last block of 1 byte
    if lib.ZSTDMI_deviceCount() == 0:       # without a device both consuming calls fail loudly
        with pytest.raises(ZstdException) as e:
            c.Wrap(b"hello, world")
        assert e.value.Code == INIT_MISSING
        with pytest.raises(ZstdException) as e:
            d.Unwrap(frame)
        assert e.value.Code == INIT_MISSING
    else:
        assert d.Unwrap(c.Wrap(b"hello, world")) == b"hello, world"
    # consumed either way: nothing is kept, and the stream calls are no longer refused
    assert c._prefix_keep is None and d._prefix_keep is None
    assert not is_error(_cstream(lib, c)) and not is_error(_dstream(lib, d))
    with pytest.raises(TypeError):
        c.RefPrefix(12345)
    c.Dispose(); d.Dispose()


@pytest.mark.parametrize("case", manifest(), ids=lambda c: c["case"])
def test_fixture_decodes_under_the_oracle_with_the_prefix_only(case):
    prefix, content = prefix_cases.build(case["case"])
    assert len(prefix) == case["prefix_n"] and hashlib.sha256(prefix).hexdigest() == case["prefix_sha256"]
    assert len(content) == case["n"] and hashlib.sha256(content).hexdigest() == case["sha256"]
    blob = open(os.path.join(GOLDEN, case["file"]), "rb").read()
    assert len(blob) == case["csize"]
    out = oracle_lib.decompress(blob, case["n"], dict_bytes=prefix)
    assert isinstance(out, bytes) and hashlib.sha256(out).hexdigest() == case["sha256"]
    assert oracle_lib.decompress(blob, case["n"]) == -20            # corruption_detected: the matches reach in front of the frame


def test_case_table_is_what_the_issue_names():
    cases = {c["case"]: c for c in manifest()}
    assert set(cases) == set(prefix_cases.CASES)
    assert cases["seam"]["prefix_n"] == 200000 and cases["seam"]["n"] == 200000
    assert cases["small_change"]["prefix_n"] == 70001 and cases["small_change"]["n"] == 70003
    assert cases["cut"]["prefix_n"] == 3 << 20 and cases["cut"]["n"] == 70003 and cases["cut"]["ldm"] == 1
    for name in ("edited_rand", "edited_text"):
        assert cases[name]["prefix_n"] == (1 << 20) + 65536 and cases[name]["n"] >= 1 << 20 and cases[name]["ldm"] == 1 and cases[name]["windowLog"] == 22
    assert all(c["csize"] < 16384 for c in cases.values())
