"""CPU tests of the seekable-stream entry points: the symbols and their types, the host-side answers (parameter checks, the bound,
NULL contexts), the pure-Python table reader on hand-built tables, and the loud failure without a device.  No kernel is launched."""
import ctypes
import struct

import pytest

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

PREFIX_UNKNOWN, CORRUPTION = ZSTD_ErrorCode.ZSTD_error_prefix_unknown, ZSTD_ErrorCode.ZSTD_error_corruption_detected
EMPTY_FRAME = bytes([0x28, 0xB5, 0x2F, 0xFD, 0x20, 0x00, 0x01, 0x00, 0x00])        # content size 0, one empty raw block
ONE_BYTE_FRAME = bytes([0x28, 0xB5, 0x2F, 0xFD, 0x20, 0x01, 0x09, 0x00, 0x00, 0x41])  # content "A": a raw last block of 1 byte


def make_table(entries, checksums=False, descriptor=None, magic=0x8F92EAB1, head_magic=0x184D2A5E, frame_size=None, count=None):
    """the seek table of `entries` = [(cSize, dSize), ...]; every field can be overridden to damage it"""
    body = b"".join(struct.pack("<III", c, d, 0xC0FFEE00 + i) if checksums else struct.pack("<II", c, d) for i, (c, d) in enumerate(entries))
    desc = (0x80 if checksums else 0) if descriptor is None else descriptor
    foot = struct.pack("<IBI", len(entries) if count is None else count, desc, magic)
    return struct.pack("<II", head_magic, len(body) + 9 if frame_size is None else frame_size) + body + foot


def test_symbols_are_exported_and_typed():
    lib = _ffi.load()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("ZSTDMI_CCtx_setSeekTable", "ZSTDMI_seekTableBound", "ZSTDMI_decompressRange", "ZSTDMI_debugLastRangeFrames",
                 "ZSTDMI_debugLastRangeStaged"):
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES, name
    assert lib.ZSTDMI_decompressRange.argtypes[5] is ctypes.c_ulonglong and lib.ZSTDMI_decompressRange.restype is ctypes.c_size_t
    assert lib.ZSTDMI_debugLastRangeStaged.restype is ctypes.c_longlong and lib.ZSTDMI_debugLastRangeFrames.restype is ctypes.c_int
    assert callable(z.read_seek_table) and hasattr(z.Decompressor, "unwrap_range") and isinstance(z.Compressor.seek_table, property)


def test_switch_values_and_null_contexts():
    lib = _ffi.load()
    c = z.Compressor(1)
    assert lib.ZSTDMI_CCtx_setSeekTable(c.cctx, 1) == 0 and lib.ZSTDMI_CCtx_setSeekTable(c.cctx, 0) == 0
    for mode in (2, 3, 0xFFFFFFFF):
        assert get_error_code(lib.ZSTDMI_CCtx_setSeekTable(c.cctx, mode)) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    assert c.seek_table is False
    c.seek_table = True
    assert c.seek_table is True
    c.seek_table = False
    c.Dispose()
    assert get_error_code(lib.ZSTDMI_CCtx_setSeekTable(None, 1)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    buf = ctypes.create_string_buffer(16)
    assert get_error_code(lib.ZSTDMI_decompressRange(None, buf, 16, EMPTY_FRAME, len(EMPTY_FRAME), 0, 1)) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    assert lib.ZSTDMI_debugLastRangeFrames(None) == -1 and lib.ZSTDMI_debugLastRangeStaged(None) == -1
    d = z.Decompressor()
    assert lib.ZSTDMI_debugLastRangeFrames(d.dctx) == 0 and lib.ZSTDMI_debugLastRangeStaged(d.dctx) == 0
    d.Dispose()


def test_bound_is_monotone_and_covers_4k_frames():
    lib = _ffi.load()
    sizes = [0, 1, 4095, 4096, 4097, 65535, 65536, 65537, 300000, 1 << 20, (1 << 20) + 1, 1 << 30, (1 << 32) + 5]
    prev = 0
    for n in sizes:
        b = lib.ZSTDMI_seekTableBound(n)
        assert b >= prev, n
        assert b >= 17 + 8 * (n // 4096), n
        assert b >= 17 + 8, n                     # an empty input still writes one frame
        prev = b
    # dense check of monotonicity around the steps
    vals = [lib.ZSTDMI_seekTableBound(n) for n in range(0, 3 * 4096 + 2)]
    assert all(a <= b for a, b in zip(vals, vals[1:]))


@pytest.mark.parametrize("checksums", [False, True])
def test_read_seek_table_parses_both_strides(checksums):
    entries = [(9, 0), (1000, 65536), (12, 0), (77, 1), (4000, 240 * 1024)]
    front = bytes(sum(c for c, _ in entries))
    table = make_table(entries, checksums=checksums)
    got, nbytes = z.read_seek_table(front + table)
    assert got == entries
    assert nbytes == len(table) == 17 + len(entries) * (12 if checksums else 8)
    # the low descriptor bits are ignored; bytearray and memoryview are accepted
    table2 = make_table(entries, checksums=checksums, descriptor=(0x80 if checksums else 0) | 3)
    assert z.read_seek_table(bytearray(front + table2)) == (entries, len(table2))
    assert z.read_seek_table(memoryview(front + table)) == (entries, len(table))
    # no frames at all
    assert z.read_seek_table(make_table([])) == ([], 17)


def _code(blob):
    with pytest.raises(ZstdException) as e:
        z.read_seek_table(blob)
    return e.value.Code


def test_read_seek_table_error_codes():
    entries = [(100, 5000), (50, 0), (200, 70000)]
    front = bytes(350)
    assert _code(b"") == PREFIX_UNKNOWN
    assert _code(bytes(16)) == PREFIX_UNKNOWN                                                       # srcSize < 17
    assert _code(front + make_table(entries, magic=0x8F92EAB0)) == PREFIX_UNKNOWN                   # footer magic
    assert _code(front + make_table(entries, head_magic=0x184D2A5D)) == PREFIX_UNKNOWN              # header magic not ...5E
    assert _code(front + make_table(entries, head_magic=0x184D2A50)) == PREFIX_UNKNOWN              # (another skippable magic)
    assert _code(front + make_table(entries, frame_size=8 * 3 + 9 + 1)) == PREFIX_UNKNOWN           # header size field
    assert _code(front + make_table(entries, count=2)) == PREFIX_UNKNOWN                            # header missing where the count puts it
    for bit in (0x04, 0x08, 0x10, 0x20, 0x40):
        assert _code(front + make_table(entries, descriptor=bit)) == CORRUPTION                     # reserved bits
    assert _code(front + make_table(entries, count=(1 << 27) + 1)) == CORRUPTION                    # N too large
    assert _code(front + make_table(entries, count=1000)) == CORRUPTION                             # table longer than the stream
    assert _code(front[1:] + make_table(entries)) == CORRUPTION                                     # sum of cSize off by one
    assert _code(front + b"\0" + make_table(entries)) == CORRUPTION
    assert z.read_seek_table(front + make_table(entries))[0] == entries


def test_range_call_fails_loudly_without_a_device():
    lib = _ffi.load()
    if lib.ZSTDMI_deviceCount() > 0:
        pytest.skip("a GPU is visible here")
    blob = ONE_BYTE_FRAME + make_table([(len(ONE_BYTE_FRAME), 1)])
    assert z.read_seek_table(blob) == ([(len(ONE_BYTE_FRAME), 1)], 25)
    room = (ctypes.c_ubyte * 64)(*([0xA5] * 64))
    d = z.Decompressor()
    r = lib.ZSTDMI_decompressRange(d.dctx, ctypes.addressof(room) + 16, 32, blob, len(blob), 0, 1)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_init_missing
    assert bytes(room) == b"\xA5" * 64
    with pytest.raises(ZstdException) as e:
        d.unwrap_range(blob, 0, 1)
    assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_init_missing
    d.Dispose()
    c = z.Compressor(1)
    c.seek_table = True
    with pytest.raises(ZstdException) as e:
        c.Wrap(b"hello")
    assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_init_missing
    c.Dispose()
