"""GPU tests of seekable streams: ZSTDMI_CCtx_setSeekTable appends a seek table to exactly the bytes the context writes without it, and
ZSTDMI_decompressRange returns any byte range of such a stream (this library's framings at their smallest, and foreign streams with a
hand-built table) while decoding only the frames that meet the range.

Layout of every range call: dst starts HEAD (an odd number of) bytes into a buffer filled with 0xA5 and everything outside
[dst, dst + returned) must still be 0xA5 afterwards; a device source lies 3 bytes into its tensor."""
import ctypes
import functools
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD, TAIL, CANARY = 37, 64, 0xA5
ZSTD_c_windowLog, ZSTD_c_enableLongDistanceMatching = 101, 160
PREFIX_UNKNOWN, CORRUPTION = ZSTD_ErrorCode.ZSTD_error_prefix_unknown, ZSTD_ErrorCode.ZSTD_error_corruption_detected
TOO_SMALL, UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall, ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
COMBOS = [(False, False), (True, True), (False, True), (True, False)]       # (source on the device, destination on the device)


def make_table(entries, checksums=False, descriptor=None, magic=0x8F92EAB1, head_magic=0x184D2A5E, frame_size=None, count=None):
    """the seek table of `entries` = [(cSize, dSize), ...]; every field can be overridden to damage it"""
    body = b"".join(struct.pack("<III", c, d, 0xC0FFEE00 + i) if checksums else struct.pack("<II", c, d) for i, (c, d) in enumerate(entries))
    desc = (0x80 if checksums else 0) if descriptor is None else descriptor
    foot = struct.pack("<IBI", len(entries) if count is None else count, desc, magic)
    return struct.pack("<II", head_magic, len(body) + 9 if frame_size is None else frame_size) + body + foot


class Stream:
    """a seekable stream, its content and its table as the test reads it"""

    def __init__(self, blob, content, dict_bytes=None, entries=None, table_bytes=None):
        self.blob, self.content, self.dict_bytes = blob, content, dict_bytes
        if entries is None:
            entries, table_bytes = z.read_seek_table(blob)
        self.entries, self.table_bytes = entries, table_bytes
        self._dev = None

    def dev(self):
        if self._dev is None:
            import torch
            self._dev = torch.from_numpy(np.frombuffer(bytes(3) + self.blob, dtype=np.uint8).copy()).cuda()
        return self._dev

    def bounds(self):
        """content offsets of the entries with content, plus the total"""
        out, at = [], 0
        for _, d in self.entries:
            if d:
                out.append(at)
            at += d
        return out + [at]

    def selection(self, offset, length):
        """-> (entries with content that meet the range, compressed bytes from the first to the last of them)"""
        c_at = d_at = 0
        meet, c_lo, c_hi = 0, None, 0
        for c, d in self.entries:
            if d > 0 and d_at < offset + length and d_at + d > offset and length > 0:
                meet += 1
                c_lo = c_at if c_lo is None else c_lo
                c_hi = c_at + c
            c_at += c
            d_at += d
        return meet, (c_hi - c_lo if meet else 0)


def wrap(data, level, seek, params=(), history=None, pass_chunks=None, dict_bytes=None):
    lib = z._ffi.load()
    with z.Compressor(level) as c:
        for p, v in params:
            c.SetParameter(p, v)
        if history is not None:
            assert lib.ZSTDMI_CCtx_setHistory(c.cctx, history[0], history[1]) == 0
        if pass_chunks is not None:
            assert lib.ZSTDMI_CCtx_setPassChunks(c.cctx, pass_chunks) == 0
        if dict_bytes is not None:
            c.LoadDictionary(dict_bytes)
        c.seek_table = seek
        return c.Wrap(data)


@functools.lru_cache(maxsize=None)
def data_of(kind, n, seed):
    return datagen.gen(kind, n, seed)


def golden_file(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


# name -> (data, level, keyword arguments of wrap)
FRAMINGS = {
    "single-block-64k": lambda: (data_of("text", 300000, 31), 1, dict(history=(0, 0))),
    "four-16k-blocks": lambda: (data_of("text", 300000, 32), 1, {}),
    "multi-block-240k": lambda: (data_of("text", 1 << 20, 33), 3, {}),
    "windowlog12": lambda: (data_of("text", 300000, 34), 1, dict(params=((ZSTD_c_windowLog, 12),))),
    "several-passes": lambda: (data_of("mixed", 1 << 20, 35), 3, dict(pass_chunks=4)),
    "two-range-plan": lambda: (data_of("text", 8 << 20, 36) + data_of("rand", 16 << 20, 37), 5, {}),
    "raw-dictionary": lambda: (data_of("text", 300000, 38), 1, dict(dict_bytes=golden_file("rawcontent_6000.dict"))),
    "formatted-dictionary": lambda: (data_of("text", 300000, 39), 3, dict(dict_bytes=golden_file("trained_16k.dict"))),
    "empty": lambda: (b"", 1, {}),
    "one-byte": lambda: (b"Z", 3, {}),
}


@functools.lru_cache(maxsize=None)
def framing(name):
    data, level, kw = FRAMINGS[name]()
    return Stream(wrap(data, level, True, **kw), data, kw.get("dict_bytes")), wrap(data, level, False, **kw)


def make_decompressor(stream):
    d = z.Decompressor()
    if stream.dict_bytes is not None:
        d.LoadDictionary(stream.dict_bytes)
    return d


def call_range(lib, dctx, stream, offset, length, src_dev, dst_dev, cap=None, blob=None):
    """-> (return value, the whole destination buffer as a numpy array: HEAD guard bytes, cap bytes of dst, TAIL guard bytes)"""
    import torch
    blob = stream.blob if blob is None else blob
    if cap is None:
        cap = len(stream.content[offset:offset + length])
    if dst_dev:
        buf = torch.full((HEAD + cap + TAIL,), CANARY, dtype=torch.uint8, device="cuda")
        dptr = buf.data_ptr() + HEAD
    else:
        buf = np.full(HEAD + cap + TAIL, CANARY, dtype=np.uint8)
        dptr = buf.ctypes.data + HEAD
    if src_dev:
        if blob is stream.blob:
            src = stream.dev()
        else:
            src = torch.from_numpy(np.frombuffer(bytes(3) + blob, dtype=np.uint8).copy()).cuda()
        sptr = src.data_ptr() + 3
    else:
        src = blob
        sptr = ctypes.cast(ctypes.c_char_p(src), ctypes.c_void_p).value
    torch.cuda.synchronize()
    r = lib.ZSTDMI_decompressRange(dctx, dptr, cap, sptr, len(blob), offset, length)
    host = buf.cpu().numpy() if dst_dev else buf
    del src
    return r, host


def check_range(lib, dctx, stream, offset, length, src_dev, dst_dev, what=""):
    want = stream.content[offset:offset + length]
    r, host = call_range(lib, dctx, stream, offset, length, src_dev, dst_dev)
    tag = (what, offset, length, src_dev, dst_dev)
    assert not is_error(r), (tag, get_error_code(r))
    assert r == len(want), tag
    assert host[HEAD:HEAD + r].tobytes() == want, tag
    assert (host[:HEAD] == CANARY).all() and (host[HEAD + r:] == CANARY).all(), tag
    meet, span = stream.selection(offset, length)
    if r:
        assert lib.ZSTDMI_debugLastRangeFrames(dctx) == meet, tag
    else:
        assert lib.ZSTDMI_debugLastRangeFrames(dctx) == 0, tag
    staged = lib.ZSTDMI_debugLastRangeStaged(dctx)
    if src_dev:
        assert staged == 0, tag
    else:
        assert 0 < staged <= stream.table_bytes + span, (tag, staged)
    return staged


def ranges_of(stream, seed):
    """-> [(what, offset, length)]: the fixed cases that exist for this stream's frames, and 32 seeded random ranges"""
    b = stream.bounds()
    total, nf = b[-1], len(b) - 1
    out = [("length 0", 0, 0), ("length 0 inside", total // 2, 0), ("offset == total", total, 10), ("offset > total", total + 1, 10),
           ("offset far beyond", total + (1 << 40), 1), ("whole content", 0, total), ("whole content and more", 0, total + 1000)]
    if total:
        out += [("first byte", 0, 1), ("last byte", total - 1, 1), ("past the end", max(total - 10, 0), 1000),
                ("short last frame", b[nf - 1], total - b[nf - 1]), ("inside the last frame", b[nf - 1] + (total - b[nf - 1]) // 2, 1 << 30)]
    for k in sorted({0, nf // 2, nf - 1} if nf else ()):
        size = b[k + 1] - b[k]
        if size >= 8:
            out.append((f"inside frame {k}", b[k] + 3, size - 6))
            out.append((f"one byte inside frame {k}", b[k] + size // 2, 1))
        out.append((f"frame {k} exactly", b[k], size))
    if nf >= 2:
        out += [("across one boundary", b[1] - 5, 10), ("across the last boundary", b[nf - 1] - 1, 2), ("two frames exactly", b[0], b[2] - b[0])]
    if nf >= 4:
        out += [("aligned at both ends", b[1], b[3] - b[1]), ("aligned start, cut end", b[1], b[3] - b[1] - 1), ("cut start, aligned end", b[1] + 1, b[3] - b[1] - 1)]
    rng = np.random.default_rng(seed)
    for i in range(32 if total else 0):
        off = int(rng.integers(0, total))
        most = total - off if i % 8 == 0 else min(total - off, 700000)
        out.append((f"random {i}", off, int(rng.integers(1, most + 1))))
    return out


# ---------------------------------------------------------------- identity
@pytest.mark.parametrize("level", [1, 3, 5])
@pytest.mark.parametrize("kind", ["text", "zipf", "mixed"])
def test_table_is_appended_to_the_same_bytes(gpu_lib, oracle, kind, level):
    data = data_of(kind, 700001, 50 + level)
    off, on = wrap(data, level, False), wrap(data, level, True)
    entries, table_bytes = z.read_seek_table(on)
    assert on[:len(on) - table_bytes] == off
    assert table_bytes == 17 + 8 * len(entries) and on[-5] == 0            # 8-byte entries, descriptor 0
    assert len(on) <= gpu_lib.ZSTD_compressBound(len(data)) + gpu_lib.ZSTDMI_seekTableBound(len(data))
    # the table against a host walk of the frames
    walk, at = [], 0
    while at < len(off):
        rest = off[at:]
        c = gpu_lib.ZSTD_findFrameCompressedSize(rest, len(rest))
        assert not is_error(c)
        walk.append((c, gpu_lib.ZSTD_getFrameContentSize(rest, len(rest))))
        at += c
    assert entries == walk and len(entries) > 1
    with z.Decompressor() as d:
        assert d.Unwrap(on) == data
    assert oracle.decompress(on, len(data)) == data


def test_device_call_writes_the_same_stream(gpu_lib):
    import torch
    data = data_of("text", 300000, 32)
    on = framing("four-16k-blocks")[0].blob
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    cap = gpu_lib.ZSTD_compressBound(len(data)) + gpu_lib.ZSTDMI_seekTableBound(len(data))
    dst = torch.full((cap + 65,), CANARY, dtype=torch.uint8, device="cuda")
    with z.Compressor(1) as c:
        c.seek_table = True
        torch.cuda.synchronize()
        r = gpu_lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr() + 1, cap, src.data_ptr(), len(data))
        assert not is_error(r), get_error_code(r)
        host = dst.cpu().numpy()
        assert host[1:1 + r].tobytes() == on and host[0] == CANARY and (host[1 + r:] == CANARY).all()
        # the frames fit, the table does not: dstSize_tooSmall (one byte short, and no room at all behind the frames)
        for short in (1, z.read_seek_table(on)[1]):
            r = gpu_lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr() + 1, len(on) - short, src.data_ptr(), len(data))
            assert get_error_code(r) == TOO_SMALL
        room = bytearray(len(on) - 1)
        ok, _ = c.TryWrap(data, room)
        assert not ok


# ---------------------------------------------------------------- framings and ranges
@pytest.mark.parametrize("name", list(FRAMINGS))
def test_ranges_of_every_framing(gpu_lib, oracle, name):
    stream, plain = framing(name)
    data = stream.content
    assert stream.blob[:len(stream.blob) - stream.table_bytes] == plain
    assert sum(d for _, d in stream.entries) == len(data) and sum(c for c, _ in stream.entries) == len(plain)
    sizes = [d for _, d in stream.entries]
    if name == "single-block-64k":
        assert sizes == [65536] * 4 + [300000 - 4 * 65536]
    elif name == "four-16k-blocks":
        assert sizes == [65536] * 4 + [300000 - 4 * 65536]
    elif name == "multi-block-240k":
        assert sizes == [240 << 10] * 4 + [(1 << 20) - 4 * (240 << 10)]
    elif name == "windowlog12":
        assert sizes == [65536] * 4 + [300000 - 4 * 65536]
    elif name == "several-passes":
        assert sizes == [240 << 10] * 4 + [(1 << 20) - 4 * (240 << 10)]
    elif name == "two-range-plan":
        assert 65536 in sizes and max(sizes) > 65536
        assert sizes[0] > 65536 and sizes[-1] == 65536            # text first, random bytes behind it: the table is in input order
    elif name in ("empty", "one-byte"):
        assert stream.entries == [(len(plain), len(data))]
    else:
        assert len(sizes) > 4 and max(sizes) <= 65536
    with make_decompressor(stream) as d:
        assert d.Unwrap(stream.blob, maxDecompressedSize=1 << 30) == data
        if stream.dict_bytes is None or stream.dict_bytes[:4] != bytes([0x37, 0xA4, 0x30, 0xEC]):
            assert oracle.decompress(stream.blob, len(data), stream.dict_bytes) == data
        seen = set()
        for i, (what, offset, length) in enumerate(ranges_of(stream, 1000 + len(name))):
            combo = COMBOS[i % 4]
            seen.add(combo)
            staged = check_range(gpu_lib, d.dctx, stream, offset, length, *combo, what=what)
            meet, _ = stream.selection(offset, length)
            if not combo[0] and meet == 1 and len(sizes) >= 4:
                assert staged < len(stream.blob), (what, staged)          # one frame of several: not the whole stream
        if len(data):
            assert seen == set(COMBOS)
        # the whole content and a cut range through every pointer combination
        b = stream.bounds()
        for combo in COMBOS:
            check_range(gpu_lib, d.dctx, stream, 0, len(data), *combo, what="whole")
            if len(b) > 2:
                check_range(gpu_lib, d.dctx, stream, b[1] - 7, 20, *combo, what="cut")
        # the Python surface: bytes in, bytes out; tensor in, tensor out
        assert d.unwrap_range(stream.blob, len(data) // 3, 1000) == data[len(data) // 3:len(data) // 3 + 1000]
        got = d.unwrap_range(stream.dev()[3:], len(data) // 2, 70000)
        assert got.is_cuda and got.cpu().numpy().tobytes() == data[len(data) // 2:len(data) // 2 + 70000]


@pytest.mark.parametrize("name", ["four-16k-blocks", "multi-block-240k", "formatted-dictionary", "one-byte"])
def test_capacity_one_byte_short(gpu_lib, name):
    stream, _ = framing(name)
    total = len(stream.content)
    with make_decompressor(stream) as d:
        for i, (offset, length) in enumerate([(0, total), (total // 3, total // 2 + 1), (total - 1, 5), (0, 1)]):
            want = len(stream.content[offset:offset + length])
            for combo in (COMBOS[i % 4], COMBOS[(i + 1) % 4]):
                r, host = call_range(gpu_lib, d.dctx, stream, offset, length, *combo, cap=want - 1)
                assert get_error_code(r) == TOO_SMALL, (offset, length, combo)
                assert (host == CANARY).all(), (offset, length, combo)
                r, host = call_range(gpu_lib, d.dctx, stream, offset, length, *combo, cap=want + 9)      # more room than needed: fine
                assert r == want and host[HEAD:HEAD + r].tobytes() == stream.content[offset:offset + length]
                assert (host[HEAD + r:] == CANARY).all() and (host[:HEAD] == CANARY).all()


# ---------------------------------------------------------------- the single-call path for large frames
def test_frame_above_the_batch_limit_is_decoded_alone(gpu_lib):
    data = data_of("rand", 5 << 20, 61)
    blob = wrap(data, 1, True, params=((ZSTD_c_enableLongDistanceMatching, 1), (ZSTD_c_windowLog, 23)))
    stream = Stream(blob, data)
    assert [d for _, d in stream.entries if d] == [5 << 20] and stream.entries[0][0] > (4 << 20)
    with z.Decompressor() as d:
        for combo in COMBOS:
            check_range(gpu_lib, d.dctx, stream, (5 << 19) + 12345, 100000, *combo, what="middle of the one frame")
            assert gpu_lib.ZSTDMI_debugLastRangeFrames(d.dctx) == 1
        check_range(gpu_lib, d.dctx, stream, 0, 5 << 20, True, True, what="the whole frame, in place")


# ---------------------------------------------------------------- foreign streams
@functools.lru_cache(maxsize=None)
def foreign_parts():
    """[(compressed bytes, content, dSize for the table)]: golden frames made by libzstd, a skippable frame between them, one frame
    without a content size (its size comes from the manifest)"""
    import oracle_lib
    cases = {c["file"]: c for c in json.load(open(os.path.join(GOLDEN, "manifest.json")))["cases"]}
    cases.update({c["file"]: c for c in json.load(open(os.path.join(GOLDEN, "manifest_dict.json")))["cases"]})
    parts = []
    for name in ("text_20000_l1.zst", "zipf_40000_l5_chk.zst", None, "mixed_150000_l5.zst", "stream_unsized_zipf_70000_l3.zst", "bytei_0_l1.zst",
                 "text_5000_x2_multiframe.zst", "runs_50000_l1.zst", "text_300000_l5.zst"):
        if name is None:
            parts.append((struct.pack("<II", 0x184D2A53, 11) + b"hello world", b"", 0))
            continue
        blob, c = golden_file(name), cases[name]
        n = c["n"] * c.get("copies", 1)
        content = oracle_lib.decompress(blob, n)
        assert isinstance(content, bytes) and len(content) == n
        if c.get("copies", 1) == 1:
            assert hashlib.sha256(content).hexdigest() == c["sha256"]
        parts.append((blob, content, n))          # (the two-frame golden is ONE entry: its two frames decode one behind the other)
    return parts


@pytest.mark.parametrize("checksums", [False, True])
def test_foreign_stream_with_a_hand_built_table(gpu_lib, checksums):
    parts = foreign_parts()
    entries = [(len(b), n) for b, _, n in parts]
    front = b"".join(b for b, _, _ in parts)
    table = make_table(entries, checksums=checksums)
    stream = Stream(front + table, b"".join(c for _, c, _ in parts))
    assert stream.entries == entries and stream.table_bytes == len(table) == 17 + len(entries) * (12 if checksums else 8)
    b = stream.bounds()
    with z.Decompressor() as d:
        i = 0
        for k in range(1, len(b) - 1):            # every junction: a few bytes on both sides, and frame-aligned pairs
            for offset, length in ((b[k] - 3, 6), (b[k] - 1, 1), (b[k], 1), (b[k - 1], b[k + 1] - b[k - 1]), (b[k] - 1000, 2000)):
                check_range(gpu_lib, d.dctx, stream, max(offset, 0), length, *COMBOS[i % 4], what=f"junction {k}")
                i += 1
        for combo in COMBOS:
            check_range(gpu_lib, d.dctx, stream, 0, b[-1], *combo, what="whole")
        for what, offset, length in ranges_of(stream, 77)[-32:]:
            check_range(gpu_lib, d.dctx, stream, offset, length, *COMBOS[i % 4], what=what)
            i += 1


# ---------------------------------------------------------------- damaged tables
def test_damaged_tables_give_their_codes(gpu_lib):
    stream, plain = framing("four-16k-blocks")
    e = stream.entries
    total = len(stream.content)
    bump = lambda k, dc, dd: [(c + (dc if i == k else 0), d + (dd if i == k else 0)) for i, (c, d) in enumerate(e)]
    cases = [
        ("footer magic", make_table(e, magic=0x8F92EAB0), PREFIX_UNKNOWN, True),
        ("header magic", make_table(e, head_magic=0x184D2A5D), PREFIX_UNKNOWN, True),
        ("header magic (another skippable)", make_table(e, head_magic=0x184D2A50), PREFIX_UNKNOWN, True),
        ("header size", make_table(e, frame_size=8 * len(e) + 10), PREFIX_UNKNOWN, True),
        ("count one less: no header there", make_table(e, count=len(e) - 1), PREFIX_UNKNOWN, True),
        ("reserved bits", make_table(e, descriptor=0x20), CORRUPTION, True),
        ("reserved bit 2", make_table(e, descriptor=0x04), CORRUPTION, True),
        ("N too large", make_table(e, count=(1 << 27) + 1), CORRUPTION, True),
        ("table longer than the stream", make_table(e, count=1 << 20), CORRUPTION, True),
        ("cSize sum + 1", make_table(bump(2, 1, 0)), CORRUPTION, True),
        ("cSize sum - 1", make_table(bump(0, -1, 0)), CORRUPTION, True),
        ("dSize larger", make_table(bump(1, 0, 1)), CORRUPTION, False),
        ("dSize smaller", make_table(bump(1, 0, -1)), CORRUPTION, False),
        ("dSize much larger", make_table(bump(3, 0, 100000)), CORRUPTION, False),
        ("dSize of a frame 0", make_table(bump(4, 0, 3 - e[4][1])), CORRUPTION, False),
    ]
    with z.Decompressor() as d:
        i = 0
        for what, table, code, reader_too in cases:
            blob = plain + table
            if reader_too:
                with pytest.raises(ZstdException) as err:
                    z.read_seek_table(blob)
                assert err.value.Code == code, what
            # the whole content (frames in place), and ranges that cut the damaged frames (the edge path)
            for offset, length in ((0, total), (65536 + 100, 10), (3 * 65536 - 5, 65536 + 10), (4 * 65536 + 1, 2)):
                for combo in (COMBOS[i % 4], COMBOS[(i + 2) % 4]):
                    r, host = call_range(gpu_lib, d.dctx, stream, offset, length, *combo, cap=length, blob=blob)
                    if reader_too or offset == 0:
                        assert get_error_code(r) == code, (what, offset, length, combo, r)
                    else:               # a range the damaged entry may not touch: the content or the entry's error, nothing else
                        assert get_error_code(r) in (0, code), (what, offset, length, combo, r)
                    assert (host[:HEAD] == CANARY).all() and (host[HEAD + length:] == CANARY).all(), (what, offset, length, combo)
                    if is_error(r) and reader_too:
                        assert (host == CANARY).all(), (what, offset, length, combo)
                i += 1
        # ranges through a damaged entry itself
        for what, table in (("dSize larger", make_table(bump(1, 0, 1))), ("dSize smaller", make_table(bump(1, 0, -1)))):
            for offset, length in ((65536 + 100, 10), (65536, 65536), (65530, 20)):
                for combo in COMBOS:
                    r, host = call_range(gpu_lib, d.dctx, stream, offset, length, *combo, cap=length, blob=plain + table)
                    assert get_error_code(r) == CORRUPTION, (what, offset, length, combo)
                    assert (host[:HEAD] == CANARY).all() and (host[HEAD + length:] == CANARY).all()
        # a boundary moved into a payload (the sizes still add up): an error, never a fault
        for k, shift in ((1, 7), (1, -7), (2, 1000), (0, -4), (3, e[4][0])):
            moved = [(c + (shift if i == k else -shift if i == k + 1 else 0), dd) for i, (c, dd) in enumerate(e)]
            blob = plain + make_table(moved)
            assert z.read_seek_table(blob)[0] == moved
            for offset, length in ((0, total), (k * 65536 + 50, 65536), ((k + 1) * 65536 + 5, 10)):
                for combo in COMBOS:
                    r, host = call_range(gpu_lib, d.dctx, stream, offset, length, *combo, cap=length, blob=blob)
                    assert is_error(r), (k, shift, offset, length, combo)
                    assert (host[:HEAD] == CANARY).all() and (host[HEAD + length:] == CANARY).all()
        # the context still works
        check_range(gpu_lib, d.dctx, stream, 1000, 200000, False, True)


# ---------------------------------------------------------------- refusals
def test_calls_that_cannot_write_a_table_refuse(gpu_lib):
    import torch
    data = data_of("text", 300000, 32)
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    dst = torch.empty(400000, dtype=torch.uint8, device="cuda")
    with z.Compressor(1) as c:
        c.seek_table = True
        got = (ctypes.c_size_t * 1)()
        r = gpu_lib.ZSTDMI_compressBatch(c.cctx, (ctypes.c_void_p * 1)(src.data_ptr()), (ctypes.c_size_t * 1)(1000), 1,
                                         (ctypes.c_void_p * 1)(dst.data_ptr()), (ctypes.c_size_t * 1)(2000), got)
        assert get_error_code(r) == UNSUPPORTED
        with pytest.raises(ZstdException) as err:
            z.compress_batch(c, [data[:1000]])
        assert err.value.Code == UNSUPPORTED
        out = ctypes.create_string_buffer(1 << 17)
        ob, ib = ZSTD_outBuffer(ctypes.cast(out, ctypes.c_void_p).value, len(out), 0), ZSTD_inBuffer(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value, 1000, 0)
        for end_op in (0, 1, 2):
            assert get_error_code(gpu_lib.ZSTD_compressStream2(c.cctx, ctypes.byref(ob), ctypes.byref(ib), end_op)) == UNSUPPORTED
        assert ib.pos == 0 and ob.pos == 0
        # ZSTD_compressCCtx runs with the level alone: no table, the bytes of a context that never had the switch
        cap = gpu_lib.ZSTD_compressBound(len(data)) + gpu_lib.ZSTDMI_seekTableBound(len(data))
        a, b = ctypes.create_string_buffer(cap), ctypes.create_string_buffer(cap)
        ra = gpu_lib.ZSTD_compressCCtx(c.cctx, a, cap, data, len(data), 1)
        with z.Compressor(1) as plain:
            rb = gpu_lib.ZSTD_compressCCtx(plain.cctx, b, cap, data, len(data), 1)
        assert not is_error(ra) and a.raw[:ra] == b.raw[:rb]
        with pytest.raises(ZstdException):
            z.read_seek_table(a.raw[:ra])
        # switched off again: the batch call runs
        c.seek_table = False
        assert z.compress_batch(c, [data[:1000]])[0] == wrap(data[:1000], 1, False)
    with z.Compressor(1) as c:
        c.seek_table = True
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        with pytest.raises(ZstdException) as err:
            c.Wrap(data)
        assert err.value.Code == UNSUPPORTED
        torch.cuda.synchronize()
        assert get_error_code(gpu_lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), 400000, src.data_ptr(), len(data))) == UNSUPPORTED
        c.seek_table = False
        assert c.Wrap(data) == framing("four-16k-blocks")[1]
    stream, _ = framing("four-16k-blocks")
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        r, host = call_range(gpu_lib, d.dctx, stream, 10, 100, False, False)
        assert get_error_code(r) == UNSUPPORTED and (host == CANARY).all()
        assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, None, 0) == 0
        check_range(gpu_lib, d.dctx, stream, 10, 100, False, False)
