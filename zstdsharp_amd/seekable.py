"""The seek table of a seekable stream (the zstd seekable format, include/zstd_mi355x.h), read on the host: pure Python, no device.

    0x184D2A5E (4) | Frame_Size (4) | N entries | Number_Of_Frames (4) | descriptor (1) | 0x8F92EAB1 (4)
    entry: Compressed_Size (4) | Decompressed_Size (4) | [Checksum (4), only if the descriptor's bit 7 is set]
"""
import struct

from .errors import ZstdException, ZSTD_ErrorCode

SEEKABLE_MAGIC = 0x8F92EAB1
SKIPPABLE_MAGIC = 0x184D2A5E
MAX_FRAMES = 1 << 27


def _fail(code, what):
    raise ZstdException(code, f"seek table: {what}")


def read_seek_table(blob, front=0):
    """-> ([(compressed size, content size), ...], the table's byte length): one pair per frame of the stream, in order; the table
    is the last `byte length` bytes of blob.  Checksums, where the table has them, are skipped.  Raises ZstdException with the code
    ZSTDMI_decompressRange gives for the same table.  front: bytes of the stream in front of blob that the caller did not bring
    (blob is then the stream's tail and must hold the whole table)."""
    mv = memoryview(blob).cast("B")
    size = front + len(mv)
    bad_prefix, corrupt = ZSTD_ErrorCode.ZSTD_error_prefix_unknown, ZSTD_ErrorCode.ZSTD_error_corruption_detected
    if size < 17:
        _fail(bad_prefix, "the stream is shorter than an empty table")
    count, descriptor, magic = struct.unpack("<IBI", mv[len(mv) - 9:])
    if magic != SEEKABLE_MAGIC:
        _fail(bad_prefix, "no seekable magic at the end of the stream")
    if descriptor & 0x7C:
        _fail(corrupt, "reserved descriptor bits are set")
    if count > MAX_FRAMES:
        _fail(corrupt, "more than 2^27 frames")
    stride = 12 if descriptor & 0x80 else 8
    table_bytes = 17 + count * stride
    if table_bytes > size:
        _fail(corrupt, "the table is longer than the stream")
    at = size - table_bytes
    if at < front:
        raise ValueError("the tail does not hold the whole table")
    head_magic, frame_size = struct.unpack("<II", mv[at - front:at - front + 8])
    if head_magic != SKIPPABLE_MAGIC or frame_size != table_bytes - 8:
        _fail(bad_prefix, "no skippable header of the table's size in front of it")
    entries = [struct.unpack_from("<II", mv, at - front + 8 + i * stride) for i in range(count)]
    if sum(c for c, _ in entries) != at:
        _fail(corrupt, "the compressed sizes do not add up to the bytes in front of the table")
    return entries, table_bytes
