"""GPU tests of ZSTDMI_DCtx_prepareRangesAsync / ZSTDMI_decompressRangesAsync (include/zstd_mi355x.h "gather reads enqueued from the
device") through Decompressor.PrepareRangesAsync and batch.decompress_ranges_async: the stream is prepared once, the five arrays are
CUDA tensors, the call only enqueues, and what arrives is — per range, size or error code and bytes — what ZSTDMI_decompressRanges
gives on a SECOND context with the same setup, but for the header's exceptions (maxRangeBytes, the limits, no single-call path).

Layout of every call (Lay): the destinations lie in one tensor filled with 0xA5, at odd offsets, in shuffled order, with 64 guard bytes
or more between them; the yardstick call gets a tensor of the same layout, so the two WHOLE buffers are compared, and every byte
outside what a range reports as written must still be 0xA5.  A device source lies 3 bytes into its tensor.  (Nothing here is meant to
fault: the decoder bounds every read and write itself.)"""
import ctypes
import functools
import os
import struct
import sys

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.batch import decompress_batch_async, decompress_ranges_async
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_train as mgt  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = 0xA5
ZSTD_c_checksumFlag = 201
WS_TOO_SMALL, TOO_SMALL, DST_NULL = -66, -70, -74
PREFIX_UNKNOWN, CORRUPTION = ZSTD_ErrorCode.ZSTD_error_prefix_unknown, ZSTD_ErrorCode.ZSTD_error_corruption_detected
STAGE_WRONG = ZSTD_ErrorCode.ZSTD_error_stage_wrong


def make_table(entries, checksums=False, descriptor=None, magic=0x8F92EAB1, head_magic=0x184D2A5E, frame_size=None, count=None):
    """the seek table of `entries` = [(cSize, dSize), ...]; every field can be overridden to damage it"""
    body = b"".join(struct.pack("<III", c, d, 0xC0FFEE00 + i) if checksums else struct.pack("<II", c, d) for i, (c, d) in enumerate(entries))
    desc = (0x80 if checksums else 0) if descriptor is None else descriptor
    foot = struct.pack("<IBI", len(entries) if count is None else count, desc, magic)
    return struct.pack("<II", head_magic, len(body) + 9 if frame_size is None else frame_size) + body + foot


def golden_bytes(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


@functools.lru_cache(maxsize=None)
def data_of(kind, n, seed):
    return datagen.gen(kind, n, seed)


def to_device(blob):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(3) + blob, dtype=np.uint8).copy()).cuda()


class Stream:
    """a seekable stream on the device, its table as the test reads it, and the sizes of the records its ranges are made from"""

    def __init__(self, blob, records, dict_bytes=None):
        self.blob, self.records, self.dict_bytes = blob, [int(r) for r in records], dict_bytes
        self.entries, self.table_bytes = z.read_seek_table(blob)
        self.d_at = np.concatenate([[0], np.cumsum([d for _, d in self.entries], dtype=np.int64)]).astype(np.int64)
        self.total = int(self.d_at[-1])
        assert self.total == sum(self.records)
        self._dev = None

    def dev(self):
        """the stream as a tensor (a view 3 bytes into its storage)"""
        if self._dev is None:
            self._dev = to_device(self.blob)
        return self._dev[3:]

    def setup(self, d):
        if self.dict_bytes is not None:
            d.LoadDictionary(self.dict_bytes)

    def met(self, offset, length):
        """indices of the entries with content that meet the range"""
        if length <= 0 or offset >= self.total:
            return []
        end = min(offset + length, self.total)
        first = int(np.searchsorted(self.d_at, offset, side="right")) - 1
        last = int(np.searchsorted(self.d_at, end - 1, side="right")) - 1
        return [i for i in range(first, last + 1) if self.entries[i][1]]


def _records(sizes, seed):
    """one record per size, text and zipf bytes in turn"""
    text, zipf = data_of("text", 1 << 20, seed), data_of("zipf", 1 << 20, seed + 1)
    out, at = [], 0
    for i, n in enumerate(sizes):
        src = zipf if i % 2 else text
        at = (at + 4099) % (len(src) - 70001)
        out.append(src[at:at + n])
    return out


@functools.lru_cache(maxsize=None)
def stream_of(name):
    if name in ("pack-l1", "pack-l3"):
        sizes = np.random.default_rng(len(name)).integers(0, 70001, 200)
        sizes[3] = sizes[17] = sizes[199] = 0
        sizes[5] = 70000
        with z.Compressor(1 if name == "pack-l1" else 3) as c:
            s = Stream(z.compress_pack(c, _records(sizes.tolist(), 50)), sizes)
        assert any(d == 0 for _, d in s.entries) or len(s.entries) < 200         # (empty records)
        if name == "pack-l1":
            assert len(s.entries) > 200                                            # (records of two frames)
        return s
    if name == "wrap":
        data = data_of("text", 3 << 20, 52)
        with z.Compressor(3) as c:
            c.seek_table = True
            return Stream(c.Wrap(data), [30000] * 100 + [(3 << 20) - 3000000])
    if name == "dict-pack":
        recs, dic = mgt.json_records(2000, 77)[1000:], golden_bytes("train_default_json.dict")
        with z.Compressor(1) as c:
            c.LoadDictionary(dic)
            c.dict_index = True
            return Stream(z.compress_pack(c, recs), [len(r) for r in recs], dic)
    if name == "checksummed":
        data = data_of("text", 300000, 31)
        with z.Compressor(1) as c:
            c.SetParameter(ZSTD_c_checksumFlag, 1)
            assert z._ffi.load().ZSTDMI_CCtx_setHistory(c.cctx, 0, 0) == 0
            c.seek_table = True
            return Stream(c.Wrap(data), [65536] * 4 + [300000 - 4 * 65536])
    raise KeyError(name)


class Result:
    """.sizes: per range the bytes returned or the error code as a negative number; .host: the whole destination buffer"""

    def __init__(self, sizes, host):
        self.sizes, self.host = sizes, host


class Lay:
    """n ranges (offsets and lengths: CUDA int64 tensors, computed by the caller on the device) and where their destinations lie.
    short: ranges whose capacity is one byte less than they return; null: ranges without a destination"""

    def __init__(self, stream, offsets, lengths, short=(), null=(), seed=1):
        self.stream, self.offsets, self.lengths = stream, offsets.contiguous(), lengths.contiguous()
        self.offs, self.lens = self.offsets.cpu().tolist(), self.lengths.cpu().tolist()     # (the test's business, not the call's)
        self.n = len(self.offs)
        self.want = [min(l, max(stream.total - o, 0)) for o, l in zip(self.offs, self.lens)]
        short, self.null = set(short), set(null)
        self.caps = [w - 1 if (i in short and w) else w for i, w in enumerate(self.want)]
        self.pos, at = [0] * self.n, 1
        for i in np.random.default_rng(seed).permutation(self.n).tolist():
            self.pos[i] = at
            at = (at + self.caps[i] + 64) | 1
        self.size = at + 64

    def buffer(self):
        import torch
        dst = torch.full((self.size,), CANARY, dtype=torch.uint8, device="cuda")
        return dst, [0 if i in self.null else dst.data_ptr() + self.pos[i] for i in range(self.n)]

    def enqueue(self, d, n=None):
        """-> (the sizes tensor, the destination tensor): nothing is waited for"""
        import torch
        n = self.n if n is None else n
        dst, ptrs = self.buffer()
        cols = [torch.tensor(c[:n], dtype=torch.int64, device="cuda") for c in (ptrs, self.caps)]
        return decompress_ranges_async(d, self.offsets[:n], self.lengths[:n], cols[0], cols[1]), dst

    def fetch(self, out, dst):
        import torch
        torch.cuda.synchronize()
        return Result([int(x) for x in out.cpu().tolist()], dst.cpu().numpy())

    def run_async(self, d, n=None):
        return self.fetch(*self.enqueue(d, n))

    def run_sync(self, d, n=None):
        """the yardstick: ZSTDMI_decompressRanges with the same arguments as host arrays"""
        import torch
        n = self.n if n is None else n
        dst, ptrs = self.buffer()
        got = (ctypes.c_size_t * n)()
        src = self.stream.dev()
        torch.cuda.synchronize()
        r = d._lib.ZSTDMI_decompressRanges(d.dctx, src.data_ptr(), src.numel(), (ctypes.c_ulonglong * n)(*self.offs[:n]), (ctypes.c_size_t * n)(*self.lens[:n]), n,
                                           (ctypes.c_void_p * n)(*[p or None for p in ptrs[:n]]), (ctypes.c_size_t * n)(*self.caps[:n]), got)
        assert r == 0, get_error_code(r)
        return Result([-get_error_code(g) if is_error(g) else int(g) for g in got], dst.cpu().numpy())

    def assert_canaries(self, res):
        """nothing outside the bytes the ranges report (a failed range: not a byte)"""
        rest = res.host.copy()
        for i, g in enumerate(res.sizes):
            if g > 0:
                assert g <= self.caps[i] and i not in self.null, i
                rest[self.pos[i]:self.pos[i] + g] = CANARY
        bad = np.flatnonzero(rest != CANARY)
        assert bad.size == 0, f"bytes outside the reported results were written, first at {bad[:4]}"

    def refuse(self, res, which):
        """the yardstick's result with the ranges `which` answering workSpace_tooSmall and nothing of them written"""
        sizes, host = list(res.sizes), res.host.copy()
        for i in which:
            sizes[i] = WS_TOO_SMALL
            host[self.pos[i]:self.pos[i] + self.caps[i]] = CANARY
        return Result(sizes, host)


def assert_same(got, want):
    diff = [i for i in range(len(want.sizes)) if got.sizes[i] != want.sizes[i]]
    assert len(got.sizes) == len(want.sizes) and not diff, f"ranges {diff[:8]} answer otherwise than the synchronous call ({len(diff)}): {[(got.sizes[i], want.sizes[i]) for i in diff[:6]]}"
    if not np.array_equal(got.host, want.host):
        raise AssertionError(f"the destination buffers differ, first at byte {int(np.flatnonzero(got.host != want.host)[0])}")


def prepared(stream, max_ranges, max_range_bytes, max_content=None, **limits):
    d = z.Decompressor()
    stream.setup(d)
    d.PrepareRangesAsync(stream.dev(), max_ranges, max_range_bytes, stream.total + 1 if max_content is None else max_content, **limits)
    return d


def sync_context(stream):
    d = z.Decompressor()
    stream.setup(d)
    return d


def seeded_ranges(stream, n, seed):
    """n ranges of the stream's records, computed ON THE DEVICE from a seeded index tensor -> (offsets, lengths, short, null): whole
    records, parts of them (overlapping), runs of three records, repeats, empty ranges, ranges beyond and across the end"""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    sizes = torch.tensor(stream.records, dtype=torch.int64, device="cuda")
    ends = torch.cumsum(sizes, 0)
    starts = ends - sizes
    nrec, total = sizes.numel(), int(stream.total)
    idx = torch.randint(0, nrec, (n,), generator=gen, device="cuda")
    kind = torch.arange(n, device="cuda") % 10
    idx[5::10] = idx[0::10][:idx[5::10].numel()]                     # kind 5 repeats kind 0's record
    offsets, lengths = starts[idx].clone(), sizes[idx].clone()
    part = kind == 1
    offsets[part] += sizes[idx][part] // 3
    lengths[part] = sizes[idx][part] // 2 + 1
    lengths[kind == 2] = 0
    beyond = kind == 3
    offsets[beyond] = total + idx[beyond]
    run = kind == 4
    lengths[run] = ends[torch.clamp(idx[run] + 2, max=nrec - 1)] - starts[idx[run]]
    across = kind == 6
    offsets[across] = total - 100 - idx[across]
    lengths[across] = 1000 + idx[across]
    k = kind.cpu().tolist()
    return offsets, lengths, [i for i in range(n) if k[i] == 7], [i for i in range(n) if k[i] == 8 or (k[i] == 2 and i % 20 == 2)]


def check_parity(stream, lay, d, d_sync, n=None):
    got, want = lay.run_async(d, n), lay.run_sync(d_sync, n)
    assert_same(got, want)
    lay.assert_canaries(got)
    return got


# ---- 1. parity over framings ----
@pytest.mark.parametrize("name", ["pack-l1", "pack-l3", "wrap", "dict-pack"])
def test_parity_over_framings(gpu_lib, name):
    stream = stream_of(name)
    offsets, lengths, short, null = seeded_ranges(stream, 300, 1000 + len(name))
    lay = Lay(stream, offsets, lengths, short, null)
    assert max(lay.want) <= 1 << 20
    with prepared(stream, 300, 1 << 20) as d, sync_context(stream) as ref:
        assert d.ranges_async_plan == (len(stream.entries), stream.total)
        got = check_parity(stream, lay, d, ref)
    # every kind of answer came up
    assert TOO_SMALL in got.sizes and DST_NULL in got.sizes and 0 in got.sizes and max(got.sizes) > 0
    assert any(g == 0 and i in lay.null for i, g in enumerate(got.sizes))              # an empty range without a destination
    assert any(0 < g < l for g, l in zip(got.sizes, lay.lens))                          # clipped at the end


# ---- 2. two calls on one prepare ----
def test_two_calls_on_one_prepare(gpu_lib):
    import torch
    lib, stream = gpu_lib, stream_of("pack-l1")
    offsets, lengths, short, null = seeded_ranges(stream, 60, 7)
    first = Lay(stream, offsets, lengths, short, null)
    # fewer and other frames: twelve short ranges inside entries the index tensor picks from the table's second half
    at = torch.tensor(stream.d_at[:-1], dtype=torch.int64, device="cuda")
    pick = torch.arange(12, device="cuda") * 7 + len(stream.entries) // 2
    second = Lay(stream, at[pick] + 3, torch.full((12,), 50, dtype=torch.int64, device="cuda"), seed=2)
    touched = lambda lay: {j for o, l, w, c, i in zip(lay.offs, lay.lens, lay.want, lay.caps, range(lay.n)) if 0 < w <= c and i not in lay.null for j in stream.met(o, l)}
    t1, t2 = touched(first), touched(second)
    assert len(t2) < len(t1) and t2 - t1
    # limits that hold exactly what the larger call touches: marks left over from the first call would push the second beyond them
    content = max(sum(stream.entries[j][1] for j in t) for t in (t1, t2))
    with prepared(stream, 60, 1 << 20, content, max_frames=len(t1)) as d, sync_context(stream) as ref:
        waits, allocs = lib.ZSTDMI_debugHostWaitsD(d.dctx), lib.ZSTDMI_debugDeviceAllocsD(d.dctx)
        assert allocs > 0
        a = first.enqueue(d)
        b = second.enqueue(d)
        assert lib.ZSTDMI_debugHostWaitsD(d.dctx) == waits and lib.ZSTDMI_debugDeviceAllocsD(d.dctx) == allocs
        got_a, got_b = first.fetch(*a), second.fetch(*b)
        assert_same(got_a, first.run_sync(ref))
        assert_same(got_b, second.run_sync(ref))
        first.assert_canaries(got_a); second.assert_canaries(got_b)
        assert got_b.sizes == [50] * 12


# ---- 3. tile borders of the grid-wide scans ----
@functools.lru_cache(maxsize=None)
def tiny_pack(n):
    """n records of 1 to 40 bytes -> (the pack, the record sizes): one table entry per record"""
    rng = np.random.default_rng(n)
    sizes = rng.integers(1, 41, n).tolist()
    with z.Compressor(1) as c:
        blob = z.compress_pack(c, _records(sizes, 60))
    assert len(z.read_seek_table(blob)[0]) == n
    return blob, sizes


@pytest.mark.parametrize("checksums", [False, True])
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2500])
def test_tile_borders(gpu_lib, n, checksums):
    import torch
    blob, sizes = tiny_pack(n)
    if checksums:                                                     # the same frames behind a hand-made table of 12-byte entries
        entries, table_bytes = z.read_seek_table(blob)
        blob = blob[:len(blob) - table_bytes] + make_table(entries, checksums=True)
    stream = Stream(blob, sizes)
    assert len(stream.entries) == n and stream.table_bytes == 17 + n * (12 if checksums else 8)
    # the first and the last entry of every tile of 1024, alone and across the border, and seeded ones
    edge = sorted({j for j in (0, 1, 1022, 1023, 1024, 1025, 2047, 2048, n - 2, n - 1) if 0 <= j < n})
    at = torch.tensor(stream.d_at, dtype=torch.int64, device="cuda")
    j = torch.tensor(edge, dtype=torch.int64, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n)
    r = torch.randint(0, n - 3, (40,), generator=gen, device="cuda")
    offsets = torch.cat([at[j], torch.clamp(at[j] - 1, min=0), at[r] + 1])
    lengths = torch.cat([at[j + 1] - at[j], torch.full_like(j, 3), at[r + 3] - at[r] - 1])
    lay = Lay(stream, offsets, lengths)
    with prepared(stream, 64, 4096) as d, sync_context(stream) as ref:
        assert d.ranges_async_plan == (n, stream.total)
        got = check_parity(stream, lay, d, ref)
        assert got.sizes == lay.want
        whole = Lay(stream, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), stream.total, dtype=torch.int64, device="cuda"))
    with prepared(stream, 1, 1 << 20) as d, sync_context(stream) as ref:     # every entry touched: the plan's table is full
        assert check_parity(stream, whole, d, ref).sizes == [stream.total]


# ---- 4. the limits ----
def refused_ranges(stream, lay, max_frames=None, max_content=None, max_range_bytes=4 << 20):
    """the header's rule, from the table: -> (ranges above max_range_bytes, ranges that meet a refused entry)"""
    served = [i for i in range(lay.n) if 0 < lay.want[i] <= lay.caps[i] and i not in lay.null]
    long = [i for i in served if lay.want[i] > max_range_bytes]
    served = [i for i in served if i not in long]
    touched = sorted({j for i in served for j in stream.met(lay.offs[i], lay.lens[i])})
    refused, content = set(), 0
    for k, j in enumerate(touched):
        content += stream.entries[j][1]
        if (max_frames is not None and k + 1 > max_frames) or (max_content is not None and content > max_content):
            refused.add(j)
    return long, [i for i in served if refused & set(stream.met(lay.offs[i], lay.lens[i]))], touched


@pytest.mark.parametrize("limit", ["frames", "content", "content-exact", "range-bytes"])
def test_the_limits(gpu_lib, limit):
    stream = stream_of("pack-l1")
    offsets, lengths, short, null = seeded_ranges(stream, 120, 33)
    lay = Lay(stream, offsets, lengths, short, null)
    _, _, touched = refused_ranges(stream, lay)
    half = sum(stream.entries[j][1] for j in touched[:len(touched) // 2])
    kw = {"frames": dict(max_frames=len(touched) // 2), "content": dict(max_content=half - 1), "content-exact": dict(max_content=half),
          "range-bytes": dict(max_range_bytes=5000)}[limit]
    long, cut, _ = refused_ranges(stream, lay, **kw)
    assert (len(long) > 5 and not cut) if limit == "range-bytes" else (len(cut) > 5 and not long)
    with prepared(stream, 120, kw.get("max_range_bytes", 1 << 20), kw.get("max_content"), max_frames=kw.get("max_frames", 0)) as d, sync_context(stream) as ref:
        got = lay.run_async(d)
        assert_same(got, lay.refuse(lay.run_sync(ref), long + cut))
        lay.assert_canaries(got)
        assert sum(1 for g in got.sizes if g > 0) > 5
        # (a call inside the limits, on the same prepare, is served as before)
        inside = sorted((i for i in range(lay.n) if got.sizes[i] > 0), key=lambda i: got.sizes[i])[:4]
        import torch
        pick = torch.tensor(inside, dtype=torch.int64, device="cuda")
        small = Lay(stream, lay.offsets[pick], lay.lengths[pick])
        check_parity(stream, small, d, ref)


# ---- 5. a damaged frame ----
def test_a_damaged_frame_fails_only_the_ranges_that_meet_it(gpu_lib):
    import torch
    good = stream_of("checksummed")
    assert [d for _, d in good.entries] == [65536] * 4 + [300000 - 4 * 65536]
    blob = bytearray(good.blob)
    blob[sum(c for c, _ in good.entries[:3]) - 2] ^= 0x10           # inside frame 2's checksum: the last four bytes of the frame
    stream = Stream(bytes(blob), good.records)
    b = [int(x) for x in stream.d_at]
    ranges = [(b[1] + 500, 3000), (b[2] - 100, 200), (b[2] + 7000, 100), (b[3] - 50, 100), (b[3] + 10, 40000), (b[0], 10)]
    meets = [False, True, True, True, False, False]
    dev = torch.tensor(ranges, dtype=torch.int64, device="cuda")
    lay = Lay(stream, dev[:, 0], dev[:, 1])
    with prepared(stream, 8, 1 << 16) as d, sync_context(stream) as ref:
        want = lay.run_sync(ref)
        assert [s < 0 for s in want.sizes] == meets and len({s for s in want.sizes if s < 0}) == 1
        got = lay.run_async(d)
        assert_same(got, want)
        lay.assert_canaries(got)


# ---- 6. damaged tables ----
def test_damaged_tables_fail_the_prepare_with_the_synchronous_code(gpu_lib):
    import torch
    stream = stream_of("checksummed")
    e = stream.entries
    plain = stream.blob[:len(stream.blob) - stream.table_bytes]
    bump = lambda k, dc: [(c + (dc if i == k else 0), d) for i, (c, d) in enumerate(e)]
    cases = [
        ("footer magic", plain + make_table(e, magic=0x8F92EAB0), PREFIX_UNKNOWN),
        ("header magic", plain + make_table(e, head_magic=0x184D2A5D), PREFIX_UNKNOWN),
        ("header size", plain + make_table(e, frame_size=8 * len(e) + 10), PREFIX_UNKNOWN),
        ("count one less: no header there", plain + make_table(e, count=len(e) - 1), PREFIX_UNKNOWN),
        ("reserved bits", plain + make_table(e, descriptor=0x20), CORRUPTION),
        ("a count above 2^27", plain + make_table(e, count=(1 << 27) + 1), CORRUPTION),
        ("table longer than the stream", plain + make_table(e, count=1 << 20), CORRUPTION),
        ("cSize sum + 1", plain + make_table(bump(2, 1)), CORRUPTION),
        ("cSize sum - 1", plain + make_table(bump(0, -1)), CORRUPTION),
        ("a stream of 16 bytes", make_table([])[1:], PREFIX_UNKNOWN),
    ]
    offsets = torch.tensor([100, 65536 + 100], dtype=torch.int64, device="cuda")
    lengths = torch.tensor([50, 10], dtype=torch.int64, device="cuda")
    lay = Lay(stream, offsets, lengths)
    with z.Decompressor() as d, z.Decompressor() as ref:
        for what, blob, code in cases:
            src = to_device(blob)
            got = (ctypes.c_size_t * 2)()
            torch.cuda.synchronize()
            r = gpu_lib.ZSTDMI_decompressRanges(ref.dctx, src.data_ptr() + 3, len(blob), (ctypes.c_ulonglong * 2)(100, 65636), (ctypes.c_size_t * 2)(50, 10), 2,
                                                (ctypes.c_void_p * 2)(None, None), (ctypes.c_size_t * 2)(0, 0), got)
            assert get_error_code(r) == code, what
            with pytest.raises(ZstdException) as err:
                d.PrepareRangesAsync(src[3:], 8, 4096, 1 << 20)
            assert err.value.code == code, (what, err.value.code)
            with pytest.raises(ZstdException) as err:                 # (a failed prepare leaves none)
                lay.enqueue(d)
            assert err.value.code == STAGE_WRONG, what
        d.PrepareRangesAsync(stream.dev(), 8, 4096, 1 << 20)          # the context still works
        check_parity(stream, lay, d, ref)


# ---- 7. stage_wrong ----
def _raises(code, fn, *args):
    with pytest.raises(ZstdException) as e:
        fn(*args)
    assert e.value.code == code, e.value.code


def test_stage_wrong(gpu_lib):
    import torch
    lib, stream = gpu_lib, stream_of("checksummed")
    offsets = torch.arange(6, dtype=torch.int64, device="cuda") * 50000
    lay = Lay(stream, offsets, torch.full((6,), 2000, dtype=torch.int64, device="cuda"))
    with z.Compressor(1) as c:
        frame = c.Wrap(b"some bytes for the batch call" * 20)
    src = to_device(frame)
    cols = [torch.tensor([v], dtype=torch.int64, device="cuda") for v in (src.data_ptr() + 3, len(frame))]
    out = torch.full((1024,), CANARY, dtype=torch.uint8, device="cuda")
    cols += [torch.tensor([v], dtype=torch.int64, device="cuda") for v in (out.data_ptr(), 1024)]
    with z.Decompressor() as d, sync_context(stream) as ref:
        want = lay.run_sync(ref)
        prepare = lambda n=6: d.PrepareRangesAsync(stream.dev(), n, 4096, 1 << 20)
        _raises(STAGE_WRONG, lay.enqueue, d)                          # no prepare
        prepare(4)
        _raises(STAGE_WRONG, lay.enqueue, d)                          # n > maxRanges
        assert lay.run_async(d, 4).sizes == want.sizes[:4]
        prepare()
        setters = [lambda: d.SetParameter(z.ZSTD_d_windowLogMax, 27), lambda: setattr(d, "batch_unsized", False),
                   lambda: lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, 0), lambda: lib.ZSTDMI_DCtx_setExecWaves(d.dctx, 0),
                   lambda: lib.ZSTDMI_DCtx_setProfiling(d.dctx, 0), lambda: d.LoadDictionary(golden_bytes("rawcontent_6000.dict")),
                   lambda: d.LoadDictionary(None)]
        for s in setters:                                             # (the value it had: any setter invalidates)
            s()
            _raises(STAGE_WRONG, lay.enqueue, d)
            with pytest.raises(ZstdException):
                d.ranges_async_plan
            prepare()
            assert d.ranges_async_plan == (len(stream.entries), stream.total)
        assert_same(lay.run_async(d), want)
        d.PrepareBatchAsync(4, 4096, 1 << 16)                         # the other kind replaces this one ...
        _raises(STAGE_WRONG, lay.enqueue, d)
        decompress_batch_async(d, *cols)
        prepare()                                                     # ... and is replaced by it
        _raises(STAGE_WRONG, decompress_batch_async, d, *cols)
        assert_same(lay.run_async(d), want)
        torch.cuda.synchronize()
        assert bytes(out[:len(b"some bytes for the batch call" * 20)].cpu().numpy()) == b"some bytes for the batch call" * 20


# ---- 8. a synchronous call in between ----
def test_a_synchronous_call_in_between(gpu_lib):
    stream, other = stream_of("pack-l3"), stream_of("checksummed")
    offsets, lengths, short, null = seeded_ranges(stream, 100, 21)
    lay = Lay(stream, offsets, lengths, short, null)
    with prepared(stream, 100, 1 << 20) as d, sync_context(stream) as ref:
        want = lay.run_sync(ref)
        a = lay.enqueue(d)
        # (another stream, a table of another length, on the SAME context: its own index and marks, the shared decode buffers)
        back = d.unwrap_ranges(other.dev(), [(10, 100000), (200000, 5000)])
        b = lay.enqueue(d)
        assert_same(lay.fetch(*a), want)
        assert_same(lay.fetch(*b), want)
        assert [t.numel() for t in back] == [100000, 5000]
        assert bytes(back[1].cpu().numpy()) == data_of("text", 300000, 31)[200000:205000]
        assert d.ranges_async_plan == (len(stream.entries), stream.total)


# ---- 9. a stream of its own ----
def test_on_a_stream_of_its_own(gpu_lib):
    import torch
    stream = stream_of("pack-l3")
    sizes_host = stream.records
    with prepared(stream, 256, 1 << 17) as d, sync_context(stream) as ref:
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            sizes = torch.tensor(sizes_host, dtype=torch.int64, device="cuda")
            starts = torch.cumsum(sizes, 0) - sizes
            gen = torch.Generator(device="cuda")
            gen.manual_seed(9)
            idx = torch.randint(0, sizes.numel(), (256,), generator=gen, device="cuda")      # the sampler
            offsets, lengths = starts[idx], sizes[idx]
            slot = 70000 + 65
            dst = torch.full((256 * slot + 64,), CANARY, dtype=torch.uint8, device="cuda")
            dsts = dst.data_ptr() + 1 + torch.arange(256, device="cuda", dtype=torch.int64) * slot
            out = decompress_ranges_async(d, offsets, lengths, dsts, lengths.clone())
            total = out.clamp(min=0).sum()                                                    # a torch op behind it, same stream
        torch.cuda.synchronize()                # the one wait, at the very end
        lay = Lay(stream, offsets, lengths)
        want = lay.run_sync(ref)
    idx_h, out_h, dst_h = idx.cpu().tolist(), out.cpu().tolist(), dst.cpu().numpy()
    assert out_h == [sizes_host[i] for i in idx_h] == want.sizes and int(total) == sum(out_h)
    for i in range(256):
        mine = dst_h[1 + i * slot:1 + (i + 1) * slot]
        assert np.array_equal(mine[:out_h[i]], want.host[lay.pos[i]:lay.pos[i] + out_h[i]]), i
        assert (mine[out_h[i]:] == CANARY).all(), i


# ---- 10. dispose while in flight ----
def test_dispose_straight_after_a_call(gpu_lib):
    stream = stream_of("pack-l1")
    offsets, lengths, short, null = seeded_ranges(stream, 200, 5)
    lay = Lay(stream, offsets, lengths, short, null)
    with sync_context(stream) as ref:
        want = lay.run_sync(ref)
    d = prepared(stream, 200, 1 << 20)
    out, dst = lay.enqueue(d)
    d.Dispose()                                  # (nothing synchronised first: the context waits for its own work)
    got = lay.fetch(out, dst)
    assert_same(got, want)
    lay.assert_canaries(got)
