"""GPU tests of gather reads: ZSTDMI_decompressRanges serves many ranges of one seekable stream in one call, decodes every frame that
some range meets once, and answers each range exactly as ZSTDMI_decompressRange answers it alone.

The model throughout is content[o : o + l] and the table from read_seek_table.  Layout of every call: all destinations lie in ONE
device buffer filled with 0xA5, each HEAD (an odd number of) bytes behind its predecessor's end and in shuffled order, and the WHOLE
buffer is compared afterwards with what the model puts there — so a byte written anywhere outside [dsts[i], dsts[i] + dstSizes[i])
fails the call's check.  A device source lies 3 bytes into its tensor."""
import ctypes
import functools
import os
import struct

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD, CANARY = 37, 0xA5
ALONE_ABOVE = 4 << 20
ZSTD_c_windowLog, ZSTD_c_enableLongDistanceMatching, ZSTD_c_checksumFlag = 101, 160, 201
PREFIX_UNKNOWN, CORRUPTION = ZSTD_ErrorCode.ZSTD_error_prefix_unknown, ZSTD_ErrorCode.ZSTD_error_corruption_detected
TOO_SMALL, UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall, ZSTD_ErrorCode.ZSTD_error_parameter_unsupported


def make_table(entries, checksums=False, descriptor=None, magic=0x8F92EAB1, head_magic=0x184D2A5E, frame_size=None, count=None):
    """the seek table of `entries` = [(cSize, dSize), ...]; every field can be overridden to damage it"""
    body = b"".join(struct.pack("<III", c, d, 0xC0FFEE00 + i) if checksums else struct.pack("<II", c, d) for i, (c, d) in enumerate(entries))
    desc = (0x80 if checksums else 0) if descriptor is None else descriptor
    foot = struct.pack("<IBI", len(entries) if count is None else count, desc, magic)
    return struct.pack("<II", head_magic, len(body) + 9 if frame_size is None else frame_size) + body + foot


def to_device(blob):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(3) + blob, dtype=np.uint8).copy()).cuda()


class Stream:
    """a seekable stream, its content and its table as the test reads it"""

    def __init__(self, blob, content, dict_bytes=None):
        self.blob, self.content, self.dict_bytes = blob, content, dict_bytes
        self.entries, self.table_bytes = z.read_seek_table(blob)
        self._dev = None
        self.d_at = np.concatenate([[0], np.cumsum([d for _, d in self.entries], dtype=np.int64)]).astype(np.int64)
        self.total = int(self.d_at[-1])
        assert self.total == len(content)

    def dev(self):
        if self._dev is None:
            self._dev = to_device(self.blob)
        return self._dev

    def bounds(self):
        """content offsets of the entries with content, plus the total"""
        return [int(self.d_at[i]) for i, (_, d) in enumerate(self.entries) if d] + [self.total]

    def want(self, offset, length):
        return self.content[offset:offset + length]

    def met(self, offset, length):
        """indices of the entries with content that meet the range"""
        if length <= 0 or offset >= self.total:
            return range(0)
        end = min(offset + length, self.total)
        first = int(np.searchsorted(self.d_at, offset, side="right")) - 1
        last = int(np.searchsorted(self.d_at, end - 1, side="right")) - 1
        return [i for i in range(first, last + 1) if self.entries[i][1]]


def wrap(data, level, seek=True, params=(), history=None, dict_bytes=None):
    lib = z._ffi.load()
    with z.Compressor(level) as c:
        for p, v in params:
            c.SetParameter(p, v)
        if history is not None:
            assert lib.ZSTDMI_CCtx_setHistory(c.cctx, history[0], history[1]) == 0
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
    "formatted-dictionary": lambda: (data_of("text", 300000, 39), 3, dict(dict_bytes=golden_file("trained_16k.dict"))),
    "windowlog12": lambda: (data_of("text", 300000, 34), 1, dict(params=((ZSTD_c_windowLog, 12),))),
    "empty": lambda: (b"", 1, {}),
    "one-byte": lambda: (b"Z", 3, {}),
}


@functools.lru_cache(maxsize=None)
def framing(name):
    data, level, kw = FRAMINGS[name]()
    return Stream(wrap(data, level, **kw), data, kw.get("dict_bytes"))


def make_decompressor(stream):
    d = z.Decompressor()
    if stream.dict_bytes is not None:
        d.LoadDictionary(stream.dict_bytes)
    return d


class Call:
    """one ZSTDMI_decompressRanges call: .ret, .sizes, the whole destination buffer afterwards (.host; destination i starts at .pos[i])
    and the three debug counters"""


def call_ranges(lib, dctx, blob, ranges, src_dev, caps, seed=5, dev_src=None, null_empty=False):
    """ranges = [(offset, length)], caps[i] = room of destination i -> Call.  Destinations in shuffled order with guard bytes between."""
    import torch
    n = len(ranges)
    order = np.random.default_rng(seed).permutation(n).tolist()          # (plain ints: ctypes takes no numpy integers as pointers)
    pos, at = [0] * n, HEAD
    for i in order:
        pos[i] = at
        at += caps[i] + HEAD + (i % 3)             # (every alignment comes up)
    buf = torch.full((at + 64,), CANARY, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    if src_dev:
        src = dev_src if dev_src is not None else to_device(blob)
        sptr = src.data_ptr() + 3
    else:
        src = blob
        sptr = ctypes.cast(ctypes.c_char_p(src), ctypes.c_void_p).value
    offs = (ctypes.c_ulonglong * max(n, 1))(*[o for o, _ in ranges])
    lens = (ctypes.c_size_t * max(n, 1))(*[l for _, l in ranges])
    dsts = (ctypes.c_void_p * max(n, 1))(*[None if (null_empty and caps[i] == 0) else base + pos[i] for i in range(n)])
    cps = (ctypes.c_size_t * max(n, 1))(*caps)
    got = (ctypes.c_size_t * max(n, 1))(*([0xDEAD] * n))
    torch.cuda.synchronize()
    c = Call()
    c.ret = lib.ZSTDMI_decompressRanges(dctx, sptr, len(blob), offs, lens, n, dsts, cps, got)
    c.sizes, c.pos, c.host = list(got)[:n], pos, buf.cpu().numpy()
    c.frames, c.alone, c.staged = lib.ZSTDMI_debugLastRangesFrames(dctx), lib.ZSTDMI_debugLastRangesAlone(dctx), lib.ZSTDMI_debugLastRangesStaged(dctx)
    del src
    return c


def expect_buffer(call, payloads):
    """the whole destination buffer must be CANARY except payloads[i] at destination i (None / b'' = untouched)"""
    want = np.full(len(call.host), CANARY, dtype=np.uint8)
    for i, p in enumerate(payloads):
        if p:
            want[call.pos[i]:call.pos[i] + len(p)] = np.frombuffer(p, dtype=np.uint8)
    if not np.array_equal(call.host, want):
        where = int(np.flatnonzero(call.host != want)[0])
        owner = max((i for i in range(len(payloads)) if call.pos[i] <= where), key=lambda i: call.pos[i], default=None)
        raise AssertionError(f"buffer differs at byte {where} (destination {owner} starts at {call.pos[owner] if owner is not None else None})")


def single_call(lib, dctx, blob_ptr, blob_len, offset, length, cap):
    """ZSTDMI_decompressRange for the same arguments -> (return value, the destination's bytes behind a guard)"""
    import torch
    buf = torch.full((HEAD + cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = lib.ZSTDMI_decompressRange(dctx, buf.data_ptr() + HEAD, cap, blob_ptr, blob_len, offset, length)
    return r, buf.cpu().numpy()


def check_stream(lib, dctx, stream, ranges, caps=None, compare_single=True, expect_alone=0):
    """the checks of the issue's test 1 for one stream and one list of ranges, host and device source -> the two Calls"""
    wants = [stream.want(o, l) for o, l in ranges]
    caps = [len(w) for w in wants] if caps is None else caps
    served = [i for i, w in enumerate(wants) if 0 < len(w) <= caps[i] and len(w) <= ALONE_ABOVE]
    alone = [i for i, w in enumerate(wants) if len(w) <= caps[i] and len(w) > ALONE_ABOVE]
    touched = set()
    for i in served:
        touched.update(stream.met(*ranges[i]))
    payloads = [w if len(w) <= caps[i] else None for i, w in enumerate(wants)]
    calls = []
    for src_dev in (True, False):
        c = call_ranges(lib, dctx, stream.blob, ranges, src_dev, caps, dev_src=stream.dev() if src_dev else None, null_empty=True)
        assert c.ret == 0, (src_dev, get_error_code(c.ret))
        for i, w in enumerate(wants):
            if len(w) > caps[i]:
                assert get_error_code(c.sizes[i]) == TOO_SMALL, (i, ranges[i], src_dev)
            else:
                assert c.sizes[i] == len(w), (i, ranges[i], src_dev, get_error_code(c.sizes[i]))
        expect_buffer(c, payloads)
        assert c.frames == len(touched), (src_dev, c.frames, len(touched))
        assert c.alone == len(alone) == expect_alone, (src_dev, c.alone)
        if src_dev:
            assert c.staged == 0
        elif not alone:
            assert 0 < c.staged <= stream.table_bytes + sum(stream.entries[k][0] for k in touched), (c.staged, len(touched))
        calls.append(c)
    assert calls[0].sizes == calls[1].sizes and np.array_equal(calls[0].host, calls[1].host)
    if compare_single:
        sptr = stream.dev().data_ptr() + 3
        for i, (o, l) in enumerate(ranges):
            r, _ = single_call(lib, dctx, sptr, len(stream.blob), o, l, caps[i])
            assert r == calls[0].sizes[i], (i, o, l, r, calls[0].sizes[i])
    return calls


def ranges_of(stream, seed):
    """about 80 ranges: the fixed cases that exist for this stream's frames, and 32 seeded random ranges"""
    b = stream.bounds()
    total, nf = b[-1], len(b) - 1
    out = [(0, 0), (total // 2, 0), (total, 10), (total + 1, 10), (total + (1 << 40), 1), (0, total), (0, total + 1000)]
    if total:
        out += [(0, 1), (total - 1, 1), (max(total - 10, 0), 1000), (b[nf - 1], total - b[nf - 1]), (b[nf - 1] + (total - b[nf - 1]) // 2, 1 << 30)]
    for k in range(nf):
        size = b[k + 1] - b[k]
        out.append((b[k], size))                                        # each frame exactly
        if size >= 8:
            out += [(b[k] + 3, size - 6), (b[k] + size // 2, 1)]        # inside it; one byte inside it
    if nf >= 2:
        out += [(b[1] - 5, 10), (b[nf - 1] - 1, 2), (b[0], b[2] - b[0])]           # across a boundary; two frames exactly
        out += [(b[1] - 5, 10), (b[1] - 5, 10)]                          # the same range again, twice
        out += [(b[1] + 100, 5000), (b[1] + 1000, 50), (b[1] + 1010, 7)]            # nested in one frame
    if nf >= 4:
        out += [(b[1], b[3] - b[1]), (b[1], b[3] - b[1] - 1), (b[1] + 1, b[3] - b[1] - 1)]     # aligned both; cut end; cut start
    rng = np.random.default_rng(seed)
    for _ in range(32 if total else 0):
        off = int(rng.integers(0, total))
        out.append((off, int(rng.integers(1, min(total - off, 700000) + 1))))
    return out


# ---------------------------------------------------------------- 1. against the content and against the single call
@pytest.mark.parametrize("name", list(FRAMINGS))
def test_ranges_of_every_framing(gpu_lib, name):
    stream = framing(name)
    ranges = ranges_of(stream, 2000 + len(name))
    with make_decompressor(stream) as d:
        check_stream(gpu_lib, d.dctx, stream, ranges)
        # nothing to serve at all: every range empty
        check_stream(gpu_lib, d.dctx, stream, [(stream.total, 5), (0, 0)], compare_single=False)


# ---------------------------------------------------------------- 2. a frame decoded once
def test_many_ranges_in_one_frame_decode_it_once(gpu_lib):
    stream = framing("multi-block-240k")
    b = stream.bounds()
    k = 2
    rng = np.random.default_rng(12)
    ranges = [(int(rng.integers(b[k], b[k + 1] - 100)), 100) for _ in range(64)]
    with make_decompressor(stream) as d:
        dev, host = check_stream(gpu_lib, d.dctx, stream, ranges, compare_single=False)
        assert dev.frames == 1 and host.frames == 1
        entry = stream.met(*ranges[0])
        assert len(entry) == 1
        assert host.staged == stream.table_bytes + stream.entries[entry[0]][0]


# ---------------------------------------------------------------- 3. a table longer than a scan tile, with every entry shape
@functools.lru_cache(maxsize=None)
def long_table_parts():
    """3000 one-frame pieces of 40-400 bytes, a skippable frame of 8-40 bytes behind every 7th -> [(bytes, content)], 3428 entries"""
    rng = np.random.default_rng(77)
    text = data_of("text", 1 << 20, 78)
    pieces = []
    for i in range(3000):
        n = int(rng.integers(40, 401))
        at = int(rng.integers(0, len(text) - n))
        pieces.append(text[at:at + n] if i % 2 else rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    with z.Compressor(1) as c:
        frames = z.compress_batch(c, pieces)
    parts = []
    for i, (f, p) in enumerate(zip(frames, pieces)):
        parts.append((f, p))
        if i % 7 == 6:
            pay = int(rng.integers(0, 33))
            parts.append((struct.pack("<II", 0x184D2A50 + (i % 16), pay) + bytes(rng.integers(0, 256, pay, dtype=np.uint8)), b""))
    return parts


@pytest.mark.parametrize("checksums", [False, True])
def test_long_table_with_skippable_frames(gpu_lib, checksums):
    parts = long_table_parts()
    entries = [(len(f), len(p)) for f, p in parts]
    assert len(entries) == 3428 and sum(1 for _, d in entries if d == 0) == 428
    stream = Stream(b"".join(f for f, _ in parts) + make_table(entries, checksums=checksums), b"".join(p for _, p in parts))
    assert stream.entries == entries and stream.table_bytes == 17 + 3428 * (12 if checksums else 8)
    skips = [int(stream.d_at[i]) for i, (_, d) in enumerate(entries) if d == 0]          # content positions of the skippable frames
    rng = np.random.default_rng(79)
    ranges = []
    for i in range(2000):
        length = int(rng.integers(1, 5001))
        if i % 10 == 0:
            offset = skips[int(rng.integers(0, len(skips)))]                                # begins exactly there
        elif i % 10 == 1:
            offset = max(skips[int(rng.integers(0, len(skips)))] - length, 0)               # ends exactly there
        else:
            offset = int(rng.integers(0, stream.total))
        ranges.append((offset, length))
    with z.Decompressor() as d:
        check_stream(gpu_lib, d.dctx, stream, ranges)           # (every range against the single call too)


# ---------------------------------------------------------------- 4. capacity
@pytest.mark.parametrize("name", ["four-16k-blocks", "multi-block-240k", "formatted-dictionary"])
def test_capacity_one_byte_short(gpu_lib, name):
    stream = framing(name)
    ranges = ranges_of(stream, 3000 + len(name))
    caps = [len(stream.want(o, l)) for o, l in ranges]
    short = [i for i in range(len(ranges)) if i % 3 == 0 and caps[i] > 0]
    assert len(short) > 10
    for i in short:
        caps[i] -= 1
    with make_decompressor(stream) as d:
        dev, host = check_stream(gpu_lib, d.dctx, stream, ranges, caps=caps)
        for i in short:
            assert get_error_code(dev.sizes[i]) == TOO_SMALL and get_error_code(host.sizes[i]) == TOO_SMALL


# ---------------------------------------------------------------- 5. isolation of a damaged frame
def test_a_damaged_frame_fails_only_the_ranges_that_meet_it(gpu_lib):
    data = data_of("text", 300000, 31)
    blob = bytearray(wrap(data, 1, params=((ZSTD_c_checksumFlag, 1),), history=(0, 0)))
    good = Stream(bytes(blob), data)
    assert [d for _, d in good.entries] == [65536] * 4 + [300000 - 4 * 65536]
    end2 = sum(c for c, _ in good.entries[:3])
    blob[end2 - 2] ^= 0x10                          # inside frame 2's checksum: the last four bytes of the frame
    blob = bytes(blob)
    b = good.bounds()
    ranges = [(b[1] + 500, 3000), (b[2] - 100, 200), (b[2] + 7000, 100), (b[3] - 50, 100), (b[3] + 10, 40000)]
    meets = [False, True, True, True, False]
    caps = [l for _, l in ranges]
    with z.Decompressor() as d:
        dev_src = to_device(blob)
        codes = []
        for (o, l), bad in zip(ranges, meets):
            r, host = single_call(gpu_lib, d.dctx, dev_src.data_ptr() + 3, len(blob), o, l, l)
            assert is_error(r) == bad, (o, l, r)
            codes.append(r)
        for src_dev in (True, False):
            c = call_ranges(gpu_lib, d.dctx, blob, ranges, src_dev, caps, dev_src=dev_src if src_dev else None)
            assert c.ret == 0
            assert c.sizes == codes, (src_dev, [get_error_code(s) for s in c.sizes])
            expect_buffer(c, [None if bad else good.want(o, l) for (o, l), bad in zip(ranges, meets)])
            assert c.frames == 3 and c.alone == 0            # entries 1, 2 and 3 were decoded, once each


# ---------------------------------------------------------------- 6. damaged tables
def test_damaged_tables_fail_the_call_with_the_single_calls_code(gpu_lib):
    stream = framing("four-16k-blocks")
    e = stream.entries
    plain = stream.blob[:len(stream.blob) - stream.table_bytes]
    bump = lambda k, dc, dd: [(c + (dc if i == k else 0), d + (dd if i == k else 0)) for i, (c, d) in enumerate(e)]
    cases = [
        ("footer magic", plain + make_table(e, magic=0x8F92EAB0), PREFIX_UNKNOWN),
        ("header magic", plain + make_table(e, head_magic=0x184D2A5D), PREFIX_UNKNOWN),
        ("header size", plain + make_table(e, frame_size=8 * len(e) + 10), PREFIX_UNKNOWN),
        ("count one less: no header there", plain + make_table(e, count=len(e) - 1), PREFIX_UNKNOWN),
        ("reserved bits", plain + make_table(e, descriptor=0x20), CORRUPTION),
        ("a count above 2^27", plain + make_table(e, count=(1 << 27) + 1), CORRUPTION),
        ("table longer than the stream", plain + make_table(e, count=1 << 20), CORRUPTION),
        ("cSize sum + 1", plain + make_table(bump(2, 1, 0)), CORRUPTION),
        ("cSize sum - 1", plain + make_table(bump(0, -1, 0)), CORRUPTION),
        ("a stream of 16 bytes", make_table([])[1:], PREFIX_UNKNOWN),
    ]
    ranges = [(0, 100), (65536 + 100, 10), (3 * 65536 - 5, 65536 + 10), (299990, 100), (0, 0)]
    caps = [l for _, l in ranges]
    with z.Decompressor() as d:
        for what, blob, code in cases:
            dev_src = to_device(blob)
            r, host = single_call(gpu_lib, d.dctx, dev_src.data_ptr() + 3, len(blob), 65536 + 100, 10, 10)
            assert get_error_code(r) == code, what
            for src_dev in (True, False):
                c = call_ranges(gpu_lib, d.dctx, blob, ranges, src_dev, caps, dev_src=dev_src if src_dev else None)
                assert c.ret == r, (what, src_dev, get_error_code(c.ret))
                expect_buffer(c, [None] * len(ranges))
                assert c.sizes == [0xDEAD] * len(ranges), what           # (a call that failed as a whole reports no sizes)
        # a content size that is not the frame's, the compressed column still adding up: only the ranges that meet the entry fail
        for what, table in (("dSize larger", make_table(bump(1, 0, 1))), ("dSize smaller", make_table(bump(1, 0, -1)))):
            bent = Stream(plain + table, stream.content[:len(stream.content) - 1] if "smaller" in what else stream.content + b"?")
            # (the model's content is shifted by one byte behind entry 1; ranges in entry 0 and ranges inside later entries that the
            # shift does not move out of their entry are compared after mapping them back)
            shift = 1 if "larger" in what else -1
            probes = [(100, 2000, False), (65536 - 10, 20, True), (65536 + 500, 100, True), (65536, 65536 + shift, True), (2 * 65536 + shift + 100, 3000, False),
                      (4 * 65536 + shift + 5, 1000, False)]
            rs = [(o, l) for o, l, _ in probes]
            for src_dev in (True, False):
                c = call_ranges(gpu_lib, d.dctx, bent.blob, rs, src_dev, [l for _, l in rs])
                assert c.ret == 0, what
                payloads = []
                for (o, l, bad), size in zip(probes, c.sizes):
                    if bad:
                        assert get_error_code(size) == CORRUPTION, (what, o, l, size)
                        payloads.append(None)
                    else:
                        assert size == l, (what, o, l, get_error_code(size))
                        real = o if o < 65536 else o - shift            # where these bytes lie in the true content
                        payloads.append(stream.content[real:real + l])
                expect_buffer(c, payloads)
        check_stream(gpu_lib, d.dctx, stream, [(1000, 200000), (5, 5)])           # the context still works


# ---------------------------------------------------------------- 7. what goes alone
def test_a_long_range_goes_alone(gpu_lib):
    data = data_of("text", 8 << 20, 36)
    stream = Stream(wrap(data, 1), data)
    ranges = [(1000, 100), (3 << 20, 5 << 20), ((7 << 20) + 13, 100), (65536 * 40 - 50, 100)]
    with z.Decompressor() as d:
        dev, host = check_stream(gpu_lib, d.dctx, stream, ranges, expect_alone=1)
        small = set()
        for i in (0, 2, 3):
            small.update(stream.met(*ranges[i]))
        assert dev.frames == len(small) >= 3 and dev.alone == 1 and host.alone == 1
        # the stage times are the gathered pass's, also when a range went alone behind it
        assert gpu_lib.ZSTDMI_DCtx_setProfiling(d.dctx, 1) == 0
        c = call_ranges(gpu_lib, d.dctx, stream.blob, ranges, True, [l for _, l in ranges], dev_src=stream.dev())
        assert c.ret == 0 and c.alone == 1
        ms, names = (ctypes.c_float * 24)(), (ctypes.c_char_p * 24)()
        k = gpu_lib.ZSTDMI_DCtx_getStageTimes(d.dctx, ms, names, 24)
        stages = [names[i].decode() for i in range(k)]
        assert stages[:3] == ["seek_index", "ranges_select", "ranges_plan"] and stages[3] == "batch_walk" and stages[-1] == "ranges_gather", stages
        assert all(ms[i] >= 0 for i in range(k))
        gpu_lib.ZSTDMI_DCtx_setProfiling(d.dctx, 0)


def test_a_frame_above_the_batch_limit_does_not_make_its_range_alone(gpu_lib):
    data = data_of("rand", 6 << 20, 61)
    stream = Stream(wrap(data, 1, params=((ZSTD_c_enableLongDistanceMatching, 1), (ZSTD_c_windowLog, 23))), data)
    assert [dd for _, dd in stream.entries if dd] == [6 << 20] and stream.entries[0][0] > (4 << 20)
    with z.Decompressor() as d:
        dev, host = check_stream(gpu_lib, d.dctx, stream, [((3 << 20) + 12345, 100), (17, 3)])
        assert dev.alone == 0 and host.alone == 0 and dev.frames == 1


# ---------------------------------------------------------------- 8. refusals and the context afterwards
def test_refusals_leave_the_context_usable(gpu_lib):
    stream = framing("four-16k-blocks")
    plain = stream.blob[:len(stream.blob) - stream.table_bytes]
    ranges, caps = [(10, 100), (70000, 50)], [100, 50]
    out = ctypes.create_string_buffer(len(stream.content))
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        for src_dev in (True, False):
            c = call_ranges(gpu_lib, d.dctx, stream.blob, ranges, src_dev, caps)
            assert get_error_code(c.ret) == UNSUPPORTED
            expect_buffer(c, [None, None])
        assert gpu_lib.ZSTD_decompressDCtx(d.dctx, out, len(out), plain, len(plain)) == len(stream.content) and out.raw == stream.content
        assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, None, 0) == 0
        check_stream(gpu_lib, d.dctx, stream, ranges)
    with z.Decompressor() as d:
        prefix = ctypes.create_string_buffer(data_of("text", 5000, 3), 5000)
        assert gpu_lib.ZSTD_DCtx_refPrefix(d.dctx, prefix, 5000) == 0
        c = call_ranges(gpu_lib, d.dctx, stream.blob, ranges, True, caps)
        assert get_error_code(c.ret) == UNSUPPORTED
        expect_buffer(c, [None, None])
        ctypes.memset(out, 0, len(out))
        assert gpu_lib.ZSTD_decompressDCtx(d.dctx, out, len(out), plain, len(plain)) == len(stream.content) and out.raw == stream.content
        check_stream(gpu_lib, d.dctx, stream, ranges)                # (the prefix was consumed by that call)


# ---------------------------------------------------------------- 9. the mirror
def test_unwrap_ranges_bytes_and_tensor(gpu_lib):
    stream = framing("single-block-64k")
    ranges = ranges_of(stream, 9)[:8] + ranges_of(stream, 9)[-8:]
    assert len(ranges) == 16
    with z.Decompressor() as d:
        from_bytes = d.unwrap_ranges(stream.blob, ranges)
        from_tensor = d.unwrap_ranges(stream.dev()[3:], ranges)
        assert all(isinstance(x, bytes) for x in from_bytes) and all(t.is_cuda for t in from_tensor)
        assert from_bytes == [stream.want(o, l) for o, l in ranges]
        assert [t.cpu().numpy().tobytes() for t in from_tensor] == from_bytes
        assert d.unwrap_ranges(stream.blob, []) == []
        # a damaged frame (its checksum, so the failure is certain): the exception names the first failing range
        data = data_of("text", 300000, 31)
        blob = bytearray(wrap(data, 1, params=((ZSTD_c_checksumFlag, 1),), history=(0, 0)))
        entries, _ = z.read_seek_table(bytes(blob))
        blob[entries[0][0] + entries[1][0] - 2] ^= 0x10
        probes = [(10, 10), (200000, 10), (65536 + 5, 10), (65536 + 50, 10)]
        for src in (bytes(blob), to_device(bytes(blob))[3:]):
            with pytest.raises(ZstdException) as err:
                d.unwrap_ranges(src, probes)
            assert "range 2" in str(err.value) and int(err.value.Code) != 0, str(err.value)
            got = d.unwrap_ranges(src, probes[:2])              # the ranges that do not meet the frame, on their own
            assert [bytes(g) if isinstance(g, bytes) else g.cpu().numpy().tobytes() for g in got] == [data[10:20], data[200000:200010]]
        with pytest.raises(ZstdException) as err:
            d.unwrap_ranges(bytes(blob[:-1]) + b"\0", probes)
        assert err.value.Code == PREFIX_UNKNOWN
