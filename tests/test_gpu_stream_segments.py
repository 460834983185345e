"""Segmented stream decoding (ZSTDMI_DCtx_setStreamSegment): ZSTD_decompressStream decodes a frame that is still
arriving in runs of whole blocks and carries the window, the live tables' defining blocks, the repcodes and the checksum state from
one run to the next.  The fixtures are libzstd's (tests/golden): 513 blocks behind ONE Huffman table in a 2 KiB window with a
checksum; frames without a content size; a sized single-segment frame; level-19 blocks with FSE tables in repeat mode; a formatted
dictionary.  The oracle compressor supplies one-frame streams of 4 MiB.  What is asserted is the contract of the header: the one-shot
call's bytes, output before the input has ended, a bounded host buffer, the return protocol, and on damaged input an error wherever
the one-shot call has one."""
import ctypes
import hashlib
import json
import os
import random
import struct

import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK = 131075                  # a block with its header
# fixture -> its number of blocks (the table of the issue; checked against the file below)
FIXTURES = {"stream_w11_chk_text_1m_l1.zst": 513, "stream_unsized_mixed_500000_l5.zst": 6, "stream_unsized_text_300000_l1.zst": 3,
            "text_300000_l5.zst": 3, "mixed_150000_l19.zst": 7, "dict_fmt_200000_l3.zst": 2}


# frames behind a dictionary that is LARGER than the frame's window (a single-segment frame's window is its content size): the format
# lets every block reach the whole dictionary until the frame has produced a window's worth, and libzstd's frames do
DICT_FIXTURES = ("dict_fmt_120_l1.zst", "dict_fmt_900_l1.zst", "dict_fmt_5000_l1.zst", "dict_fmt_40000_l1.zst",
                 "dict_raw_500_l1.zst", "dict_raw_30000_l1.zst", "dict_raw_150000_l3.zst")


def _cases():
    out = {}
    for mf in ("manifest.json", "manifest_dict.json"):
        for c in json.load(open(os.path.join(GOLD, mf)))["cases"]:
            if c["file"] in FIXTURES or c["file"] in DICT_FIXTURES:
                out[c["file"]] = c
    return out


CASES = _cases()


def blob_of(name):
    return open(os.path.join(GOLD, name), "rb").read()


def dict_of(name):
    dn = CASES[name].get("dict")
    return open(os.path.join(GOLD, dn), "rb").read() if dn else None


def frame_blocks(blob, at=0):
    """the frame at `at`: [(offset of the block's header, size with the header)], whether it has a checksum, the position behind it"""
    assert blob[at:at + 4] == b"\x28\xb5\x2f\xfd"
    fhd = blob[at + 4]
    single, fcs, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    pos = at + 5 + (0 if single else 1) + (4 if did == 3 else did) + (single if fcs == 0 else 1 << fcs)
    blocks = []
    while True:
        h = blob[pos] | (blob[pos + 1] << 8) | (blob[pos + 2] << 16)
        size = 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)
        blocks.append((pos, size))
        pos += size
        if h & 1:
            break
    chk = (fhd >> 2) & 1
    return blocks, chk, pos + 4 * chk


class Feed:
    """ZSTD_decompressStream over `blob` in input pieces of `piece` bytes and output buffers of `outsz` bytes: the bytes handed out,
    every return value's class, and the stream's state when it stopped (at an error, or when the input ran out)."""

    def __init__(self, lib, dctx, blob, piece, outsz, stop_after=None):
        n = len(blob)
        src = ctypes.create_string_buffer(blob, n) if n else ctypes.create_string_buffer(1)
        base = ctypes.addressof(src)
        dst = ctypes.create_string_buffer(outsz)
        daddr = ctypes.addressof(dst)
        inp, out = ZSTD_inBuffer(), ZSTD_outBuffer(daddr, outsz, 0)
        pin, pout = ctypes.byref(inp), ctypes.byref(out)
        call, string_at = lib.ZSTD_decompressStream, ctypes.string_at
        got = bytearray()
        self.error = 0          # the error code the stream ended with (0 = none)
        self.zero_at = []       # the input positions at which calls returned 0
        self.calls = 0
        self.first_output_at = None     # input bytes fed when the first byte came out
        self.last = None
        fed = 0
        stop = n if stop_after is None else stop_after
        while fed < stop and not self.error:
            k = min(piece, stop - fed)
            inp.src, inp.size, inp.pos = base + fed, k, 0
            fed += k
            while True:
                out.pos = 0
                r = call(dctx, pout, pin)
                self.calls += 1
                if is_error(r):
                    self.error = get_error_code(r)
                    break
                if out.pos:
                    if self.first_output_at is None:
                        self.first_output_at = fed
                    got += string_at(daddr, out.pos)
                self.last = r
                if r == 0 and self.zero_at[-1:] != [fed - (inp.size - inp.pos)]:
                    self.zero_at.append(fed - (inp.size - inp.pos))
                if inp.pos >= inp.size and out.pos < outsz:
                    break
        self.fed = fed
        self.data = bytes(got)


def decompressor(name=None, segment=0):
    d = z.Decompressor()
    if name and dict_of(name):
        d.LoadDictionary(dict_of(name))
    if segment:
        d.stream_segment = segment
    return d


def one_shot(lib, d, blob, cap):
    buf = ctypes.create_string_buffer(max(cap, 1))
    r = lib.ZSTD_decompressDCtx(d.dctx, buf, cap, blob, len(blob))
    return (get_error_code(r), None) if is_error(r) else (0, buf.raw[:r])


# ---------------- round trip ----------------
@pytest.mark.parametrize("piece,outsz", [(1, 1 << 17), (7, 1000), (4096, 1), (1 << 20, 1 << 17)])
@pytest.mark.parametrize("segment", [1, 65536])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_round_trip(gpu_lib, name, segment, piece, outsz):
    """Every input piece size (1, 7, 4096, 1 << 20) and every output buffer size (1, 1000, 1 << 17) appears, deliberately in four
    pairings and not as their cross product: the smallest pieces with a roomy and with a tight output, the one-byte output (a million
    calls on the largest fixture) with a piece that keeps the case at a second, and the piece that holds a whole fixture."""
    blob = blob_of(name)
    blocks, _, end = frame_blocks(blob)
    assert len(blocks) == FIXTURES[name] and end == len(blob)
    d = decompressor(name, segment)
    f = Feed(gpu_lib, d.dctx, blob, piece, outsz)
    assert not f.error, ZSTD_ErrorCode(f.error)
    assert len(f.data) == CASES[name]["n"] and hashlib.sha256(f.data).hexdigest() == CASES[name]["sha256"]
    assert f.zero_at == [len(blob)] and f.last == 0, "0 exactly at the end of the frame"
    segs = gpu_lib.ZSTDMI_debugStreamSegments(d.dctx)
    if segment == 1 and piece < min(s for _, s in blocks):
        assert segs >= len(blocks), (segs, len(blocks))
    else:
        assert segs >= 1
    assert 0 < gpu_lib.ZSTDMI_debugStreamPeakInput(d.dctx) <= len(blob)
    d.Dispose()


@pytest.mark.parametrize("segment,piece", [(1, 1), (1, 7), (65536, 7), (1, 1 << 20)])
@pytest.mark.parametrize("name", DICT_FIXTURES)
def test_dictionary_larger_than_the_window(gpu_lib, name, segment, piece):
    """A formatted 16 KiB dictionary and a raw 6000-byte one in front of frames from 120 bytes up: the whole dictionary stays
    reachable (first history = all of its content), whatever the frame's window says, until the frame has produced a window."""
    blob = blob_of(name)
    blocks, _, end = frame_blocks(blob)
    assert end == len(blob)
    plain = decompressor(name)
    err, want = one_shot(gpu_lib, plain, blob, CASES[name]["n"] + 64)
    plain.Dispose()
    assert not err and hashlib.sha256(want).hexdigest() == CASES[name]["sha256"]
    d = decompressor(name, segment)
    f = Feed(gpu_lib, d.dctx, blob, piece, 1000)
    assert not f.error, ZSTD_ErrorCode(f.error)
    assert f.data == want
    assert f.zero_at == [len(blob)] and f.last == 0
    segs = gpu_lib.ZSTDMI_debugStreamSegments(d.dctx)
    assert segs >= (len(blocks) if segment == 1 and piece < min(s for _, s in blocks) else 1)
    d.Dispose()


def test_checksum_over_segments_of_odd_sizes(gpu_lib, oracle):
    """The frame checksum's carried state: segments whose outputs are no multiples of XXH64's 32-byte stripe, so that a segment begins
    with bytes left over from the one before (1 .. 31 of them), and segments too short to fill a stripe at all.  The frame is made
    here: raw and RLE blocks of the sizes below behind a 128 KiB window, the checksum from the oracle's XXH64."""
    sizes = [1, 33, 1000, 31, 7, 64, 95, 5, 5, 5, 40000, 13, 32, 31, 1, 4097]
    rng = random.Random(7)
    content, body = bytearray(), bytearray(b"\x28\xb5\x2f\xfd\x04\x38")       # checksum flag; window 2^17
    for i, n in enumerate(sizes):
        last = 1 if i == len(sizes) - 1 else 0
        if i % 5 == 4:                  # an RLE block
            b = rng.randrange(256)
            content += bytes([b]) * n
            body += struct.pack("<I", (n << 3) | 2 | last)[:3] + bytes([b])
        else:
            raw = bytes(rng.randrange(256) for _ in range(n))
            content += raw
            body += struct.pack("<I", (n << 3) | last)[:3] + raw
    content = bytes(content)
    digest = oracle.lib().zso_xxh64(content, len(content), 0) & 0xFFFFFFFF
    blob = bytes(body) + struct.pack("<I", digest)
    plain = decompressor()
    err, want = one_shot(gpu_lib, plain, blob, len(content) + 64)
    plain.Dispose()
    assert not err and want == content, "the frame made here is a valid frame with a right checksum"
    for segment, piece in ((1, 1), (64, 50), (1100, 1 << 20)):
        d = decompressor(segment=segment)
        f = Feed(gpu_lib, d.dctx, blob, piece, 1 << 17)
        assert not f.error, (segment, piece, ZSTD_ErrorCode(f.error))
        assert f.data == content and f.zero_at == [len(blob)] and f.last == 0
        if segment == 1:
            assert gpu_lib.ZSTDMI_debugStreamSegments(d.dctx) == len(sizes)
        d.Dispose()
    # and a wrong checksum is still found, at the end
    bad = blob[:-1] + bytes([blob[-1] ^ 0x40])
    d = decompressor(segment=1)
    f = Feed(gpu_lib, d.dctx, bad, 1, 1 << 17)
    assert f.error == ZSTD_ErrorCode.ZSTD_error_checksum_wrong and content.startswith(f.data) and len(f.data) >= len(content) - sizes[-1]
    d.Dispose()


# ---------------- one-frame streams of the oracle's ----------------
@pytest.fixture(scope="module")
def oracle_frames(oracle):
    made = {}

    def get(kind, n, level):
        key = (kind, n, level)
        if key not in made:
            data = datagen.gen(kind, n, 11 + level)
            blob = oracle.compress(data, level, 1, 0)
            assert isinstance(blob, bytes)
            made[key] = (data, blob)
        return made[key]
    return get


@pytest.mark.parametrize("kind,n,level", [("text", 4 << 20, 1), ("text", 4 << 20, 3), ("text", 4 << 20, 5), ("mixed", 1 << 20, 3)])
def test_oracle_one_frame_streams(gpu_lib, oracle_frames, kind, n, level):
    data, blob = oracle_frames(kind, n, level)
    blocks, chk, end = frame_blocks(blob)
    assert chk and end == len(blob) and len(blocks) >= n // (1 << 17)
    d = decompressor(segment=262144)
    f = Feed(gpu_lib, d.dctx, blob, 1 << 16, 1 << 17)
    assert not f.error, ZSTD_ErrorCode(f.error)
    assert f.data == data
    assert f.zero_at == [len(blob)] and f.last == 0
    assert gpu_lib.ZSTDMI_debugStreamSegments(d.dctx) >= 2
    d.Dispose()


def test_early_output_and_bounded_memory(gpu_lib, oracle_frames):
    data, blob = oracle_frames("text", 4 << 20, 3)
    assert len(blob) > 4 * 262144
    d = decompressor(segment=262144)
    half = Feed(gpu_lib, d.dctx, blob, 1 << 16, 1 << 17, stop_after=len(blob) // 2)
    assert not half.error and len(half.data) > 0, "output before the input has ended"
    assert half.zero_at == [] and data.startswith(half.data)
    rest = Feed(gpu_lib, d.dctx, blob[half.fed:], 1 << 16, 1 << 17)
    assert not rest.error and half.data + rest.data == data and rest.last == 0
    peak = gpu_lib.ZSTDMI_debugStreamPeakInput(d.dctx)
    assert 0 < peak <= 262144 + BLOCK + 65536 + 4 * BLOCK, peak
    d.Dispose()
    # the default: the same feeding yields nothing before the last piece
    d = decompressor()
    f = Feed(gpu_lib, d.dctx, blob, 1 << 16, 1 << 17)
    assert not f.error and f.data == data and f.last == 0
    assert f.first_output_at == len(blob), "with the switch off a frame comes out when all of it is there"
    assert gpu_lib.ZSTDMI_debugStreamSegments(d.dctx) == 0
    d.Dispose()


def test_switch_off_and_on_again(gpu_lib):
    name = "mixed_150000_l19.zst"
    blob = blob_of(name)
    plain = decompressor()
    want = Feed(gpu_lib, plain.dctx, blob, 4096, 1 << 17)
    assert not want.error and hashlib.sha256(want.data).hexdigest() == CASES[name]["sha256"]
    d = decompressor()
    for segment, segmented in ((1, True), (0, False), (4096, True), (0, False)):
        d.stream_segment = segment
        f = Feed(gpu_lib, d.dctx, blob, 4096, 1 << 17)
        assert not f.error and f.data == want.data and f.zero_at == want.zero_at and f.last == 0
        assert (gpu_lib.ZSTDMI_debugStreamSegments(d.dctx) > 0) == segmented
        assert (f.first_output_at < len(blob)) == segmented
    plain.Dispose(); d.Dispose()


# ---------------- the shape of a stream ----------------
def test_stream_shapes(gpu_lib, oracle):
    long_name = "stream_unsized_mixed_500000_l5.zst"
    long_blob = blob_of(long_name)
    plain = decompressor()
    err, long_data = one_shot(gpu_lib, plain, long_blob, 600000)
    assert not err and hashlib.sha256(long_data).hexdigest() == CASES[long_name]["sha256"]
    small = [datagen.gen("text", 3000, 1), datagen.gen("zipf", 70000, 2)]
    frames = [oracle.compress(s, 1, 1, 0) for s in small]
    skippable = struct.pack("<II", 0x184D2A53, 300) + bytes(range(256)) + bytes(44)
    for parts, want in (([long_blob, skippable] + frames, long_data + small[0] + small[1]),
                        ([frames[0], long_blob, skippable, frames[1]], small[0] + long_data + small[1])):
        blob = b"".join(parts)
        ends, at = [], 0
        for p in parts:
            at += len(p)
            ends.append(at)
        for piece in (999, 1 << 20):
            d = decompressor(segment=16384)
            f = Feed(gpu_lib, d.dctx, blob, piece, 1 << 16)
            assert not f.error, ZSTD_ErrorCode(f.error)
            assert f.data == want
            assert f.last == 0 and f.zero_at and f.zero_at[-1] == len(blob)
            assert set(f.zero_at) <= set(ends), "0 only on a frame boundary"
            assert gpu_lib.ZSTDMI_debugStreamSegments(d.dctx) >= 2
            d.Dispose()
    plain.Dispose()


# ---------------- damaged input ----------------
@pytest.mark.parametrize("name,segment", [("stream_w11_chk_text_1m_l1.zst", 4096), ("stream_unsized_mixed_500000_l5.zst", 1)])
def test_damage(gpu_lib, name, segment):
    blob = blob_of(name)
    blocks, chk, end = frame_blocks(blob)
    assert chk and end == len(blob)
    n = CASES[name]["n"]
    rng = random.Random(len(blob))
    # the block bodies, as far as they lie past the first 64 KiB
    spans = [(max(off + 3, 65536), off + size) for off, size in blocks if off + size > max(off + 3, 65536)]
    flips = []
    while len(flips) < 15:
        a, b = spans[rng.randrange(len(spans))]
        flips.append((rng.randrange(a, b), 1 << rng.randrange(8)))
    flips.append((len(blob) - 1 - rng.randrange(4), 1 << rng.randrange(8)))           # one in the trailing checksum
    plain = decompressor()
    err0, content = one_shot(gpu_lib, plain, blob, n + (1 << 17))
    assert not err0 and hashlib.sha256(content).hexdigest() == CASES[name]["sha256"]
    for i, (pos, bit) in enumerate(flips):
        bad = bytearray(blob)
        bad[pos] ^= bit
        bad = bytes(bad)
        err1, data1 = one_shot(gpu_lib, plain, bad, n + (1 << 17))
        d = decompressor(segment=segment)
        f = Feed(gpu_lib, d.dctx, bad, 1 << 15, 1 << 17)
        d.Dispose()
        what = f"flip {i} at {pos} (bit {bit}): one-shot {err1}, stream {f.error}"
        if i == 15:
            assert err1 == ZSTD_ErrorCode.ZSTD_error_checksum_wrong and f.error == ZSTD_ErrorCode.ZSTD_error_checksum_wrong, what
        if err1:
            assert f.error, what + ": an error no later than the end of the frame"
            assert not f.zero_at, what
        elif f.error:
            assert f.error == ZSTD_ErrorCode.ZSTD_error_corruption_detected, what
            assert data1.startswith(f.data), what
        else:
            assert f.data == data1 and f.last == 0, what
    # a stream that stops early never ends in 0, and nothing is an error before the input ends
    for cut in sorted(rng.randrange(1, len(blob)) for _ in range(5)):
        d = decompressor(segment=segment)
        f = Feed(gpu_lib, d.dctx, blob[:cut], 1 << 15, 1 << 17)
        d.Dispose()
        assert not f.error, (cut, f.error)
        assert not f.zero_at and f.last != 0, cut
        assert content.startswith(f.data) and len(f.data) < n
    plain.Dispose()


def test_several_workers_are_refused(gpu_lib):
    blob = blob_of("text_300000_l5.zst")
    d = decompressor(segment=1)
    assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, (ctypes.c_int * 2)(0, 0), 2) == 0
    f = Feed(gpu_lib, d.dctx, blob, 4096, 1 << 17)
    assert f.error == ZSTD_ErrorCode.ZSTD_error_parameter_unsupported and f.data == b""
    d.Dispose()
