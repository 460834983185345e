"""GPU tests of ZSTDMI_compressPackAsync / ZSTDMI_CCtx_packAsyncBound (include/zstd_mi355x.h "a pack enqueued from the device") through
batch.compress_pack_async: sources and sizes are CUDA tensors, the call only enqueues, and what arrives at d_dst is ONE seekable stream —
every entry's frames as ZSTDMI_compressBatchAsync writes them under the same prepare, one behind the other, and one seek table.

Two yardsticks, neither of them the call under test: for entries in the tier of the prepared bound the whole stream is byte for byte what
ZSTDMI_compressPack writes on a second context with the same setup; for every tier it is the concatenation of what compress_batch_async
returns for the same entries on the same prepare + make_table(rows).

Layout of every call: d_dst sits HEAD = 37 bytes into a tensor filled with 0xA5, with 64 guard bytes behind the capacity; sources are
carved from one tensor in shuffled order at odd places (test_gpu_batch_async.Layout); after every call every byte outside the reported
stream must still be 0xA5."""
import functools

import numpy as np
import pytest

import oracle_lib
import test_gpu_batch_async as base
import test_gpu_batch_async_frames as frames
import test_gpu_pack as tpack
import zstdsharp_amd as z
from test_gpu_batch_async import Layout, make_compressor
from test_gpu_pack import HEAD, TAIL, first_difference, make_table
from zstdsharp_amd.batch import compress_batch_async, compress_pack_async, decompress_batch_async, decompress_ranges_async, pack_ranges
from zstdsharp_amd.errors import ZSTD_ErrorCode

pytestmark = pytest.mark.gpu

ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 200, 201
TOO_SMALL, SRC_WRONG, WS_TOO_SMALL = -70, -72, -66
CANARY = 0xA5


def run_pack(c, lay, cap=None, n=None, with_ends=True):
    """one async pack of lay's first n entries into a canary-filled destination of `cap` bytes (default: pack_async_bound(n)); waits,
    checks the canary around the reported stream -> (the stream's bytes or the error as a negative number, entry_ends or None)"""
    import torch
    n = lay.n if n is None else n
    cap = c.pack_async_bound(n) if cap is None else cap
    buf = torch.full((HEAD + cap + TAIL,), CANARY, dtype=torch.uint8, device="cuda")
    srcs = torch.tensor(lay.src_ptr[:n], dtype=torch.int64, device="cuda")
    sizes = torch.tensor(lay.sizes[:n], dtype=torch.int64, device="cuda")
    ends = torch.full((n,), -1, dtype=torch.int64, device="cuda") if with_ends else None
    out = compress_pack_async(c, srcs, sizes, buf[HEAD:HEAD + cap], entry_ends=ends)
    torch.cuda.synchronize()
    return collect(out, buf, cap, ends)


def collect(out, buf, cap, ends=None):
    r, host = int(out.item()), buf.cpu().numpy()
    assert r <= cap
    assert (host[:HEAD] == CANARY).all(), "bytes in front of d_dst were written"
    bad = np.flatnonzero(host[HEAD + max(r, 0):] != CANARY)
    assert bad.size == 0, f"bytes outside the reported stream ({r}) were written, first at {bad[:4] + max(r, 0)}"
    ends_h = None if ends is None else [int(x) for x in ends.cpu().tolist()]
    if r < 0:
        assert ends_h is None or all(e == -1 for e in ends_h), "entry_ends was written by a failed pack"
        return r, None
    return host[HEAD:HEAD + r].tobytes(), ends_h


def sync_pack(entries, **config):
    """ZSTDMI_compressPack of the entries on a context of its own"""
    with tpack.make_compressor(**config) as ref:
        want = tpack.Pack(z._ffi.load(), entries, seed=9).run(ref.cctx)
    assert isinstance(want, bytes), want
    return want


def batch_stream(c, lay, n=None):
    """the yardstick of every tier: compress_batch_async of the same entries on the same prepare -> (frames side by side, sizes)"""
    got = lay.run_async(c, n)
    lay.assert_nothing_else_written()
    assert all(isinstance(g, bytes) for g in got), [g for g in got if not isinstance(g, bytes)][:4]
    return b"".join(got), [len(g) for g in got]


def assert_stream(stream, ends, frames_bytes, frame_sizes, sizes):
    """stream == frames + make_table(its own rows); the rows add up per entry; entry_ends is the running sum of the batch's sizes"""
    rows, table_bytes = z.read_seek_table(stream)
    assert stream == frames_bytes + make_table(rows), first_difference(stream, frames_bytes + make_table(rows))
    assert table_bytes == 17 + 8 * len(rows) and sum(r[0] for r in rows) == len(frames_bytes)
    assert ends == [int(x) for x in np.cumsum(frame_sizes)]
    at = 0
    for i, (S, F) in enumerate(zip(sizes, frame_sizes)):
        c_sum = d_sum = 0
        while c_sum < F:
            c_sum += rows[at][0]; d_sum += rows[at][1]; at += 1
        assert c_sum == F and d_sum == S, (i, c_sum, F, d_sum, S)
    assert at == len(rows)
    return rows


# ---- 1. in tier: the whole stream equals ZSTDMI_compressPack on a second context ----
@pytest.mark.parametrize("level", [1, 3, 5])
def test_one_block_bound_equals_sync_pack(gpu_lib, level):
    entries = base.large_entries()[:12]
    assert {16385, 65536} <= {len(e) for e in entries} and all(16385 <= len(e) <= 65536 for e in entries)
    want = sync_pack(entries, level=level)
    with make_compressor(level) as c:
        c.PrepareBatchAsync(len(entries), 65536)
        assert c.pack_async_bound(12) == 17 + 12 * (gpu_lib.ZSTD_compressBound(65536) + 8)
        got, ends = run_pack(c, Layout(gpu_lib, entries))
    assert got == want, first_difference(got, want)
    assert ends[-1] + 17 + 8 * len(z.read_seek_table(got)[0]) == len(got)


def tier_256k():
    entries = frames.tier_entries(131073, 262144, 8, 11)
    assert {131073, 262144, 196607, 196608, 196609} <= {len(e) for e in entries} and len(entries) == 8
    return entries


@pytest.mark.parametrize("level", [1, 3, 5])
def test_limits_bound_equals_sync_pack(gpu_lib, level):
    entries = tier_256k()
    want = sync_pack(entries, level=level)
    with make_compressor(level) as c:
        c.PrepareBatchAsyncLimits(len(entries), 262144)
        cb, fb, _ = c.batch_async_plan
        per = frames.chunks(frames.chunks(262144, cb), fb)
        assert c.pack_async_bound(8) == 17 + 8 * (gpu_lib.ZSTD_compressBound(262144) + 8 * per)
        got, _ = run_pack(c, Layout(gpu_lib, entries))
    assert got == want, first_difference(got, want)


@functools.lru_cache(maxsize=None)
def json_tier(lo, hi, count):
    flat = b"".join(base.mgt.json_records(1500, 78))
    sizes = [hi, lo] + [int(x) for x in np.random.default_rng(62).integers(lo, hi + 1, count - 2)]
    assert len(flat) > hi + count * 9973
    return tuple(flat[i * 9973:i * 9973 + n] for i, n in enumerate(sizes))


# name -> (configuration of test_gpu_pack.make_compressor, prepare, bound, entries)
SETUPS = {
    "checksum": (dict(level=3, params=((ZSTD_c_checksumFlag, 1),)), "limits", 262144, tier_256k),
    "no-content-size": (dict(level=3, params=((ZSTD_c_contentSizeFlag, 0),)), "limits", 262144, tier_256k),
    "raw-dictionary": (dict(level=1, dic="rawcontent_6000.dict"), "limits", 200000, lambda: json_tier(131073, 200000, 8)),
    "dict-index-entropy": (dict(level=1, dic="trained_16k.dict", index=True, entropy=True), "one-block", 4096, lambda: json_tier(1500, 4096, 8)),
}


@pytest.mark.parametrize("name", list(SETUPS))
def test_setups_equal_sync_pack(gpu_lib, name):
    config, prepare, bound, make = SETUPS[name]
    entries = make()
    want = sync_pack(entries, **config)
    with tpack.make_compressor(**config) as c:
        if prepare == "limits":
            c.PrepareBatchAsyncLimits(len(entries), bound)
        else:
            c.PrepareBatchAsync(len(entries), bound)
        got, _ = run_pack(c, Layout(gpu_lib, entries))
    assert got == want, first_difference(got, want)
    rows = z.read_seek_table(got)[0]
    assert sum(r[1] for r in rows) == sum(map(len, entries))        # (true content sizes in the table, whatever the frames state)


# ---- 2. every tier: equal to the async batch, a valid seekable stream under every reader ----
def test_every_tier_equals_the_async_batch(gpu_lib):
    rng = np.random.default_rng(23)
    sizes = [1, 0, 16384, 16385, 65536, 65537, 0, 131072, 131073, 262144]
    for lo, hi in ((1, 16384), (16385, 65536), (65537, 131072), (131073, 262144)):
        sizes += [int(x) for x in rng.integers(lo, hi + 1, 13)]
    sizes += [0, 0]
    entries = tuple(frames.piece(i, n) for i, n in enumerate(sizes))
    assert len(entries) == 64
    whole = b"".join(entries)
    with make_compressor(3) as c, z.Decompressor() as d:
        c.PrepareBatchAsyncLimits(len(entries), 262144)
        lay = Layout(gpu_lib, entries)
        want_frames, frame_sizes = batch_stream(c, lay)
        got, ends = run_pack(c, lay)
        assert isinstance(got, bytes), got
        assert_stream(got, ends, want_frames, frame_sizes, sizes)
        assert d.Unwrap(got) == whole
        assert oracle_lib.decompress(got, len(whole)) == whole
        assert d.unwrap_ranges(got, pack_ranges(sizes)) == list(entries)


# ---- 3. empties and small n, against ZSTDMI_compressPack ----
@pytest.mark.parametrize("shape", ["one", "all-empty", "empties-around", "none"])
def test_empties_and_small_n(gpu_lib, shape):
    e = [frames.piece(i, 2000 + 300 * i) for i in range(4)]
    entries = {"one": e[:1], "all-empty": [b""] * 5, "empties-around": [b"", b"", e[0], b"", e[1], e[2], b""], "none": []}[shape]
    want = sync_pack(entries, level=3)
    with make_compressor(3) as c:
        c.PrepareBatchAsync(8, 4096)
        assert c.pack_async_bound(0) == 17
        got, ends = run_pack(c, Layout(gpu_lib, entries))
    assert got == want, first_difference(got, want)
    if shape == "none":
        assert got == make_table([]) and len(got) == 17 and ends == []


# ---- 4. the scan's edges ----
def test_entry_counts_at_the_scan_edges_one_block(gpu_lib):
    counts = (1, 15, 16, 17, 1023, 1024, 1025, 4097)
    rng = np.random.default_rng(41)
    sizes = [3000, 1] + [int(x) for x in rng.integers(1, 3001, max(counts) - 2)]
    entries = tuple(frames.piece(i, n) for i, n in enumerate(sizes))
    with make_compressor(1) as c:
        c.PrepareBatchAsync(max(counts), 4096)
        lay = Layout(gpu_lib, entries)
        got_all = lay.run_async(c)
        lay.assert_nothing_else_written()
        for n in counts:
            got, ends = run_pack(c, lay, n=n)
            assert isinstance(got, bytes), (n, got)
            assert_stream(got, ends, b"".join(got_all[:n]), [len(g) for g in got_all[:n]], sizes[:n])


def test_entry_counts_at_the_scan_edges_limits(gpu_lib):
    counts = (1, 255, 256, 257)
    rng = np.random.default_rng(43)
    sizes = [80000, 1, 49152, 49153] + [int(x) for x in rng.integers(1, 80001, max(counts) - 4)]
    entries = tuple(frames.piece(i, n) for i, n in enumerate(sizes))
    with make_compressor(3) as c:
        c.PrepareBatchAsyncLimits(max(counts), 80000)
        lay = Layout(gpu_lib, entries)
        for n in counts:
            want_frames, frame_sizes = batch_stream(c, lay, n)
            got, ends = run_pack(c, lay, n=n)
            assert isinstance(got, bytes), (n, got)
            assert_stream(got, ends, want_frames, frame_sizes, sizes[:n])


# ---- 5. the capacity is compared on the device ----
def test_capacity_on_the_device(gpu_lib):
    entries = tier_256k()[:5]
    with make_compressor(3) as c:
        c.PrepareBatchAsyncLimits(8, 262144)
        lay = Layout(gpu_lib, entries)
        full, ends = run_pack(c, lay)                   # (pack_async_bound as the capacity never fails)
        assert isinstance(full, bytes)
        size, table = len(full), z.read_seek_table(full)[1]
        assert run_pack(c, lay, cap=size)[0] == full
        assert run_pack(c, lay, cap=size - 1)[0] == TOO_SMALL
        assert run_pack(c, lay, cap=size - table)[0] == TOO_SMALL          # the frames fit, the table does not
        assert run_pack(c, lay, cap=size - table + 16)[0] == TOO_SMALL
        assert run_pack(c, lay, cap=1)[0] == TOO_SMALL
        assert run_pack(c, lay, n=0, cap=16)[0] == TOO_SMALL
        assert run_pack(c, lay, n=0, cap=17)[0] == make_table([])
        assert run_pack(c, lay)[0] == full


# ---- 6. one answer for the whole pack: the lowest failing entry's ----
def test_the_one_answer(gpu_lib):
    sizes = [60000, 49152, 100000, 1, 98305, 120000, 60000, 49153, 131072, 90000, 70000, 0]
    entries = tuple(frames.piece(i, n) for i, n in enumerate(sizes))
    cb = frames.FRAMING[3][0]
    per = [frames.chunks(s, cb) for s in sizes]

    def run(max_chunks, oversize=(), null_src=()):
        with make_compressor(3) as c:
            c.PrepareBatchAsyncLimits(len(entries), 131072, max_chunks)
            lay = Layout(gpu_lib, entries)
            if max_chunks == 0:
                good_frames, good_sizes = batch_stream(c, lay)
            for i in oversize:
                lay.sizes[i] = 131073
            for i in null_src:
                lay.src_ptr[i] = 0
            got = run_pack(c, lay)[0]
            lay.sizes, lay.src_ptr = [len(e) for e in entries], [lay.src.data_ptr() + a for a in lay.src_at]
            again, ends = run_pack(c, lay)              # a following good call on the same prepare
            if max_chunks == 0:
                assert_stream(again, ends, good_frames, good_sizes, sizes)
            return got, again

    got, good = run(0, oversize=(3,), null_src=(9,))
    assert got == SRC_WRONG and isinstance(good, bytes)
    assert run(0, null_src=(9,))[0] == SRC_WRONG
    cut = sum(per[:6]) - 1                              # room for the entries 0 .. 4 and all but one chunk of entry 5
    got, again = run(cut, oversize=(8,))
    assert got == WS_TOO_SMALL and again == WS_TOO_SMALL
    assert run(cut, oversize=(2,))[0] == SRC_WRONG


# ---- 7. no host involvement ----
def test_no_host_wait_and_no_allocation(gpu_lib):
    import torch
    lib = gpu_lib
    entries = tier_256k()
    want = sync_pack(entries, level=3)
    with make_compressor(3) as c:
        c.PrepareBatchAsyncLimits(len(entries), 262144)
        lay = Layout(lib, entries)
        cols = lay.columns()
        cap = c.pack_async_bound(lay.n)
        bufs = [torch.full((HEAD + cap + TAIL,), CANARY, dtype=torch.uint8, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        waits, allocs = lib.ZSTDMI_debugHostWaits(c.cctx), lib.ZSTDMI_debugDeviceAllocs(c.cctx)
        frames_before = lib.ZSTDMI_debugLastPackFrames(c.cctx)
        outs = [compress_pack_async(c, cols[0], cols[1], b[HEAD:HEAD + cap]) for b in bufs]
        assert lib.ZSTDMI_debugHostWaits(c.cctx) == waits and lib.ZSTDMI_debugDeviceAllocs(c.cctx) == allocs
        assert lib.ZSTDMI_debugLastPackFrames(c.cctx) == frames_before
        torch.cuda.synchronize()
        for out, b in zip(outs, bufs):
            got = collect(out, b, cap)[0]
            assert got == want, first_difference(got, want)


def test_staleness_alternation_and_dispose(gpu_lib):
    import torch
    lib = gpu_lib
    raises, stage_wrong = base._raises, ZSTD_ErrorCode.ZSTD_error_stage_wrong
    entries = tier_256k()
    want = sync_pack(entries, level=3)
    lay = Layout(lib, entries)
    cols = lay.columns()
    cap_all = 17 + 8 * (lib.ZSTD_compressBound(262144) + 8 * 2)
    dst = torch.full((cap_all,), CANARY, dtype=torch.uint8, device="cuda")
    with make_compressor(3) as c:
        raises(stage_wrong, c.pack_async_bound, 1)
        c.PrepareBatchAsyncLimits(4, 262144)
        raises(stage_wrong, compress_pack_async, c, cols[0], cols[1], dst)             # n > maxEntries
        c.PrepareBatchAsyncLimits(8, 262144)
        assert c.pack_async_bound(8) == cap_all
        c.SetParameter(ZSTD_c_checksumFlag, 0)                                          # (the value it had: any setter invalidates)
        raises(stage_wrong, compress_pack_async, c, cols[0], cols[1], dst)
        raises(stage_wrong, c.pack_async_bound, 8)
        assert (dst.cpu().numpy() == CANARY).all()
        # a batch and a pack alternate on one prepare
        c.PrepareBatchAsyncLimits(8, 262144)
        frames_1, sizes_1 = batch_stream(c, lay)
        got_1, ends_1 = run_pack(c, lay)
        frames_2, _ = batch_stream(c, lay)
        got_2, _ = run_pack(c, lay)
        assert got_1 == want and got_2 == want and frames_1 == frames_2 == want[:ends_1[-1]]
    # the context freed straight behind an enqueued pack
    c = make_compressor(3)
    c.PrepareBatchAsyncLimits(8, 262144)
    buf = torch.full((HEAD + cap_all + TAIL,), CANARY, dtype=torch.uint8, device="cuda")
    out = compress_pack_async(c, cols[0], cols[1], buf[HEAD:HEAD + cap_all])
    c.Dispose()                              # (nothing synchronised first: the context waits for its own work)
    torch.cuda.synchronize()
    assert collect(out, buf, cap_all)[0] == want


# ---- 8. on the device end to end: pack, then both readers, the host holding one length at the very end of the first leg ----
def test_on_the_device_end_to_end(gpu_lib):
    import torch
    lib = gpu_lib
    n, bound = 40, 200000
    text = frames.pool("text")
    pool_host = text * (n * bound // len(text) + 1)
    with make_compressor(1) as c, z.Decompressor() as d, z.Decompressor() as dr:
        c.PrepareBatchAsyncLimits(n, bound)
        cap = c.pack_async_bound(n)
        d.PrepareBatchAsync(n, lib.ZSTD_compressBound(bound), n * bound, max_frames=n * frames.chunks(bound, 65536))
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            data = torch.from_numpy(np.frombuffer(pool_host[:n * bound], dtype=np.uint8).copy()).cuda()
            gen = torch.Generator(device="cuda"); gen.manual_seed(9)
            lengths = torch.randint(1, bound + 1, (n,), device="cuda", generator=gen, dtype=torch.int64)
            at = torch.cumsum(lengths, 0) - lengths
            buf = torch.full((HEAD + cap + TAIL,), CANARY, dtype=torch.uint8, device="cuda")
            dst = buf[HEAD:HEAD + cap]
            ends = torch.empty(n, dtype=torch.int64, device="cuda")
            size = compress_pack_async(c, data.data_ptr() + at, lengths, dst, entry_ends=ends)
            begins = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), ends[:-1]])
            back = torch.full((n * (bound + 3),), CANARY, dtype=torch.uint8, device="cuda")
            back_at = back.data_ptr() + torch.arange(n, device="cuda", dtype=torch.int64) * (bound + 3)
            caps = torch.full((n,), bound, dtype=torch.int64, device="cuda")
            dsizes = decompress_batch_async(d, dst.data_ptr() + begins, ends - begins, back_at, caps)
            same = torch.equal(dsizes, lengths)
        torch.cuda.synchronize()
        assert same, (dsizes.cpu().tolist(), lengths.cpu().tolist())
        lengths_h, at_h = lengths.cpu().numpy(), at.cpu().numpy()

        def check(back_t):
            back_h = back_t.cpu().numpy()
            for i in range(n):
                row = back_h[i * (bound + 3):(i + 1) * (bound + 3)]
                assert row[:lengths_h[i]].tobytes() == pool_host[at_h[i]:at_h[i] + lengths_h[i]], i
                assert (row[lengths_h[i]:] == CANARY).all(), i

        check(back)
        total = int(size.item())                # the one length the host reads
        assert collect(size, buf, cap)[0][-4:] == (0x8F92EAB1).to_bytes(4, "little")
        with torch.cuda.stream(stream):
            dr.PrepareRangesAsync(dst[:total], n, bound, n * bound)
            back2 = torch.full((n * (bound + 3),), CANARY, dtype=torch.uint8, device="cuda")
            back2_at = back2.data_ptr() + torch.arange(n, device="cuda", dtype=torch.int64) * (bound + 3)
            rsizes = decompress_ranges_async(dr, at, lengths, back2_at, caps)
            same = torch.equal(rsizes, lengths)
        torch.cuda.synchronize()
        assert same, rsizes.cpu().tolist()
        check(back2)
