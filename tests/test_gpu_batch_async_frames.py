"""GPU tests of ZSTDMI_CCtx_prepareBatchAsyncLimits (include/zstd_mi355x.h "entries of several blocks: the second prepare"): entries of
up to 4 MiB - 1 through ZSTDMI_compressBatchAsync, cut into blocks on the device.  What arrives is — for entries in the tier of the
prepared bound — byte for byte what ZSTDMI_compressBatch writes on a second context with the same setup.

Layout, canaries and helpers are those of test_gpu_batch_async.py: sources carved from one tensor in shuffled order, destinations from
one tensor filled with 0xA5 at odd offsets with guard bytes between them; everything outside the reported results must still be 0xA5."""
import functools

import numpy as np
import pytest

import oracle_lib
import test_gpu_batch_async as base
import zstdsharp_amd as z
from test_gpu_batch_async import KINDS, Layout, assert_same, data_of, expected_sync, golden_bytes, make_compressor
from zstdsharp_amd.batch import compress_batch_async, decompress_batch_async
from zstdsharp_amd.errors import ZSTD_ErrorCode

pytestmark = pytest.mark.gpu

ZSTD_c_windowLog, ZSTD_c_checksumFlag, ZSTD_c_enableLongDistanceMatching = 101, 201, 160
TOO_SMALL, SRC_WRONG, DST_NULL, WS_TOO_SMALL = -70, -72, -74, -66
FRAMING = {1: (16384, 4), 3: (49152, 5), 5: (32768, 8)}         # level -> (chunk bytes, blocks per frame) above 64 KiB without a dictionary


def chunks(size, cb):
    return (size + cb - 1) // cb


@functools.lru_cache(maxsize=None)
def pool(kind):
    return data_of(kind, 1 << 20, 4242) if kind != "pysrc" else base.python_source()


def piece(i, n):
    """entry i: n bytes of kind i % 5, a slice of that kind's pool (generated once)"""
    p = pool(KINDS[i % len(KINDS)])
    if n > len(p):
        p = p * (n // len(p) + 1)
    at = (i * 7919) % (len(p) - n + 1)
    return p[at:at + n]


@functools.lru_cache(maxsize=None)
def tier_entries(lo, hi, count, seed):
    """`count` entries of lo .. hi bytes: both ends, a size that is a multiple of 16, 32 and 48 KiB and its neighbours, then seeded sizes"""
    rng = np.random.default_rng(seed)
    mult = ((lo + hi) // 2 // 98304) * 98304 or 98304
    sizes = [hi, lo] + [s for s in (mult, mult - 1, mult + 1) if lo <= s <= hi]
    sizes += [int(x) for x in rng.integers(lo, hi + 1, count - len(sizes))]
    return tuple(piece(i, n) for i, n in enumerate(sizes))


# ---- 1. same tier: bytes equal to the synchronous batch on a second context ----
@pytest.mark.parametrize("level", [1, 3, 5])
def test_same_tier_256k_bytes_equal_sync_batch(gpu_lib, level):
    lib = gpu_lib
    entries = tier_entries(131073, 262144, 24, 11)
    assert {262144, 131073, 196608, 196607, 196609} <= {len(e) for e in entries}
    want = expected_sync("frames256k", entries, level)
    assert all(isinstance(w, bytes) for w in want)
    with make_compressor(level) as c:
        c.PrepareBatchAsyncLimits(len(entries), 262144)
        cb, fb = FRAMING[level]
        assert c.batch_async_plan == (cb, fb, len(entries) * chunks(262144, cb))
        lay = Layout(lib, entries)
        assert_same(lay.run_async(c), want)
        lay.assert_nothing_else_written()


def test_same_tier_1m_bytes_equal_sync_batch(gpu_lib):
    lib = gpu_lib
    entries = tier_entries(262145, 1048576, 6, 12)
    want = expected_sync("frames1m", entries, 3)
    assert all(isinstance(w, bytes) for w in want)
    with make_compressor(3) as c:
        c.PrepareBatchAsyncLimits(len(entries), 1048576)
        lay = Layout(lib, entries)
        assert_same(lay.run_async(c), want)
        lay.assert_nothing_else_written()


# ---- 2. every tier under one bound: valid streams, no byte identity claimed ----
def test_every_tier_decodes_under_both_decoders(gpu_lib, capsys):
    lib = gpu_lib
    rng = np.random.default_rng(21)
    sizes = [1, 16384, 16385, 65536, 65537, 131072, 131073, 262144]
    for lo, hi in ((1, 16384), (16385, 65536), (65537, 131072), (131073, 262144)):
        sizes += [int(x) for x in rng.integers(lo, hi + 1, 14)]
    entries = tuple(piece(i, n) for i, n in enumerate(sizes))
    assert len(entries) == 64
    with make_compressor(3) as c, z.Decompressor() as d:
        c.PrepareBatchAsyncLimits(len(entries), 262144)
        lay = Layout(lib, entries)
        got = lay.run_async(c)
        lay.assert_nothing_else_written()
        for i, (g, e) in enumerate(zip(got, entries)):
            assert isinstance(g, bytes), (i, g)
            assert len(g) <= lib.ZSTD_compressBound(len(e)), i
            assert d.Unwrap(g) == e, i
            assert oracle_lib.decompress(g, len(e)) == e, i
    sync_total = sum(len(x) for x in expected_sync("frames-every-tier", entries, 3))
    with capsys.disabled():
        print(f"\n[every tier, level 3, bound 256 KiB, 64 entries] async {sum(len(g) for g in got)} B, synchronous batch {sync_total} B, input {sum(map(len, entries))} B")


# ---- 3. the scan's edges: entry counts around the wave, the workgroup's 16 entries per lane, and beyond one entry per lane ----
def _one_at_a_time(c, lay):
    """every entry through a call of n = 1 on the same prepare; one fetch at the end"""
    import torch
    cols = lay.columns()
    out = torch.empty(lay.n, dtype=torch.int64, device="cuda")
    for i in range(lay.n):
        compress_batch_async(c, *[col[i:i + 1] for col in cols], out_sizes=out[i:i + 1])
    return lay.fetch(out)


@pytest.mark.parametrize("level,counts", [(3, (1, 255, 256, 257, 1025)), (1, (1, 256, 257))])
def test_entry_counts_at_the_scan_edges(gpu_lib, level, counts):
    """bound 80 000: at level 3 an entry is 1 or 2 blocks of 48 KiB; the level 1 row has the same sizes in 1 .. 5 blocks of 16 KiB"""
    lib = gpu_lib
    rng = np.random.default_rng(33)
    sizes = [80000, 1, 49152, 49153, 16384, 16385] + [int(x) for x in rng.integers(1, 80001, max(counts) - 6)]
    entries = tuple(piece(i, n) for i, n in enumerate(sizes))
    with make_compressor(level) as c, z.Decompressor() as d:
        c.PrepareBatchAsyncLimits(max(counts), 80000)
        cb = c.batch_async_plan[0]
        assert cb == FRAMING[level][0] and {chunks(s, cb) for s in sizes} == set(range(1, chunks(80000, cb) + 1))
        single = Layout(lib, entries, seed=5)
        want = _one_at_a_time(c, single)
        single.assert_nothing_else_written()
        for w, e in zip(want, entries):
            assert isinstance(w, bytes) and d.Unwrap(w) == e
        for n in counts:
            lay = Layout(lib, entries[:n], seed=n)
            assert_same(lay.run_async(c), want[:n])
            lay.assert_nothing_else_written()


# ---- 4. the chunk limit ----
def test_chunk_limit_refuses_from_the_cut_on(gpu_lib):
    lib = gpu_lib
    sizes = [150000, 49152, 262144, 1, 98305, 200000, 60000, 49153, 131072, 250000]
    good = [piece(i, n) for i, n in enumerate(sizes)]
    # an empty entry (index 3) and a NULL source (index 7) between them: they count for nothing and keep their answers
    entries = good[:3] + [b""] + good[3:6] + [good[0]] + good[6:]
    null_src, empty_at = 7, 3
    is_good = [i not in (null_src, empty_at) for i in range(len(entries))]
    with make_compressor(3) as ref:
        empty = ref.Wrap(b"")

    def run(max_chunks):
        with make_compressor(3) as c:
            c.PrepareBatchAsyncLimits(len(entries), 262144, max_chunks)
            assert c.batch_async_plan[2] == max_chunks
            lay = Layout(lib, entries)
            lay.src_ptr[null_src] = 0
            got = lay.run_async(c)
            lay.assert_nothing_else_written()       # (a refused entry's whole destination is still canary)
            return got

    cb = FRAMING[3][0]
    per = [chunks(len(e), cb) if ok else 0 for e, ok in zip(entries, is_good)]
    total = sum(per)
    full = run(total)
    assert all(isinstance(g, bytes) for i, g in enumerate(full) if is_good[i])
    assert full[null_src] == SRC_WRONG and full[empty_at] == empty
    last_good = max(i for i, ok in enumerate(is_good) if ok)
    less = run(total - 1)
    assert less[last_good] == WS_TOO_SMALL
    assert less[:last_good] == full[:last_good] and less[last_good + 1:] == full[last_good + 1:]
    # a cut in the middle: room for the first four good entries and all but one chunk of the fifth
    fifth = [i for i, ok in enumerate(is_good) if ok][4]
    cut = run(sum(per[:fifth + 1]) - 1)
    for i in range(len(entries)):
        if i < fifth or not is_good[i]:
            assert cut[i] == full[i], i
        else:
            assert cut[i] == WS_TOO_SMALL, (i, cut[i])
    assert cut[null_src] == SRC_WRONG and cut[empty_at] == empty and null_src > fifth
    # the smallest limit the bound allows, one entry's six chunks: the first two entries (four chunks and one), then the cut
    few = run(chunks(262144, cb))
    assert few[:2] == full[:2] and all(few[i] == WS_TOO_SMALL for i in range(2, len(entries)) if is_good[i])


def test_chunk_limit_below_the_entries_of_a_one_block_bound(gpu_lib):
    """a bound of one block keeps the one-block prepare's state unless maxChunks is below maxEntries: then the limit holds there too"""
    lib = gpu_lib
    entries = base.small_entries()[:20]
    want = expected_sync(4096, base.small_entries(), 3)[:20]
    with make_compressor(3) as c:
        c.PrepareBatchAsyncLimits(20, 4096)
        assert c.batch_async_plan == (65536, 0, 20)
        lay = Layout(lib, entries)
        assert_same(lay.run_async(c), want)
        c.PrepareBatchAsyncLimits(20, 4096, 30)
        assert c.batch_async_plan == (65536, 0, 20)     # (room for every entry: the same state)
        c.PrepareBatchAsyncLimits(20, 4096, 12)
        assert c.batch_async_plan == (65536, 0, 12)
        lay = Layout(lib, entries)
        got = lay.run_async(c)
        assert_same(got[:12], want[:12])
        assert got[12:] == [WS_TOO_SMALL] * 8
        lay.assert_nothing_else_written()


# ---- 5. per-entry verdicts between entries of several chunks ----
@pytest.mark.parametrize("checksum", [0, 1])
def test_per_entry_verdicts_between_multi_chunk_entries(gpu_lib, checksum):
    lib = gpu_lib
    bound = 150000
    params = ((ZSTD_c_checksumFlag, checksum),)
    good = tier_entries(131073, bound, 10, 51)          # three or four blocks of 48 KiB each, all in the bound's tier
    want_good = expected_sync(("frames-verdicts", checksum), good, 3, params)
    victim = piece(77, 140000)
    want_victim = expected_sync(("frames-victim", checksum), (victim,), 3, params)[0]
    with make_compressor(3, params) as ref:
        empty = ref.Wrap(b"")
    # between the good ones: 0 = one byte short, 1 = size bound + 1, 2 = size 0, 3 = capacity 0, 4 = NULL destination, 5 = NULL source
    entries, kind = [], []
    bad_at = {1: 0, 3: 1, 4: 2, 6: 3, 7: 4, 9: 5}
    for i, e in enumerate(good):
        if i in bad_at:
            entries.append(victim if bad_at[i] != 2 else b""); kind.append(bad_at[i])
        entries.append(e); kind.append(None)
    caps = [lib.ZSTD_compressBound(len(e)) for e in entries]
    for i, k in enumerate(kind):
        if k == 0:
            caps[i] = len(want_victim) - 1
        elif k == 3:
            caps[i] = 0
        elif k == 2:
            caps[i] = len(empty)            # (exactly the room the empty frame needs)
    with make_compressor(3, params) as c:
        c.PrepareBatchAsyncLimits(len(entries), bound)
        lay = Layout(lib, entries, caps=caps)
        for i, k in enumerate(kind):
            if k == 1:
                lay.sizes[i] = bound + 1
            elif k == 4:
                lay.dst_ptr[i] = 0
            elif k == 5:
                lay.src_ptr[i] = 0
        got = lay.run_async(c)
    answers = {0: TOO_SMALL, 1: SRC_WRONG, 2: empty, 3: TOO_SMALL, 4: DST_NULL, 5: SRC_WRONG}
    for i, k in enumerate(kind):
        if k is not None:
            assert got[i] == answers[k], (i, k, got[i])
    assert_same([g for g, k in zip(got, kind) if k is None], want_good)
    lay.assert_nothing_else_written()


# ---- 6. the largest entry: 4 MiB - 1 at level 1, 256 blocks ----
def test_one_entry_of_4mib_minus_1(gpu_lib):
    lib = gpu_lib
    n = (4 << 20) - 1
    entries = (piece(0, n),)
    want = expected_sync("frames4m", entries, 1)
    with make_compressor(1) as c, z.Decompressor() as d:
        c.PrepareBatchAsyncLimits(1, n)
        assert c.batch_async_plan == (16384, 4, 256)
        lay = Layout(lib, entries)
        got = lay.run_async(c)
        assert_same(got, want)
        lay.assert_nothing_else_written()
        assert d.Unwrap(got[0]) == entries[0]


# ---- 7. dictionaries: independent frames behind a staged tail, an index, an index with entropy tables, a CDict ----
@functools.lru_cache(maxsize=None)
def json_entries():
    flat = b"".join(base.mgt.json_records(1500, 78))
    rng = np.random.default_rng(61)
    sizes = [200000, 70000, 131072, 131073] + [int(x) for x in rng.integers(70000, 200001, 8)]
    assert len(flat) > 200000 + 12 * 9973
    return tuple(flat[i * 9973:i * 9973 + n] for i, n in enumerate(sizes))


@pytest.mark.parametrize("setup", base.DICT_SETUPS)
def test_dictionaries(gpu_lib, setup, capsys):
    lib = gpu_lib
    dic = golden_bytes("train_default_json.dict")
    entries = json_entries()
    keep = []
    with base._dict_compressor(setup, dic, keep) as ref:
        want = Layout(lib, entries, seed=7).run_sync(ref)
        assert lib.ZSTDMI_debugLastBatchAlone(ref.cctx) == 0
    with base._dict_compressor(setup, dic, keep) as c, z.Decompressor() as d:
        c.PrepareBatchAsyncLimits(len(entries), 200000)
        cb, fb, _ = c.batch_async_plan
        assert fb == 0 and cb == (65536 if setup.startswith("dict-index") else 32768)
        lay = Layout(lib, entries)
        got = lay.run_async(c)
        lay.assert_nothing_else_written()
        d.LoadDictionary(dic)
        same_tier = [i for i, e in enumerate(entries) if len(e) > 131072]           # the bound's tier: (128 KiB, 256 KiB]
        assert len(same_tier) >= 4
        assert_same([got[i] for i in same_tier], [want[i] for i in same_tier])
        for g, e in zip(got, entries):
            assert isinstance(g, bytes)
            assert d.Unwrap(g) == e
            assert oracle_lib.decompress(g, len(e), dic) == e
    with capsys.disabled():
        print(f"\n[{setup}] {sum(g == w for g, w in zip(got, want))} of {len(got)} entries equal the synchronous batch's ({len(same_tier)} in the bound's tier)")
    for k in keep:
        k.Dispose()


# ---- 8. no host round trip ----
def test_no_host_wait_and_no_allocation_across_calls(gpu_lib):
    lib = gpu_lib
    entries = tier_entries(131073, 262144, 24, 11)[:8]
    with make_compressor(3) as c:
        c.PrepareBatchAsyncLimits(len(entries), 262144)
        lay = Layout(lib, entries)
        cols = lay.columns()
        waits, allocs = lib.ZSTDMI_debugHostWaits(c.cctx), lib.ZSTDMI_debugDeviceAllocs(c.cctx)
        assert allocs > 0                    # (the prepare sized the workspaces: the counter counts)
        outs = [compress_batch_async(c, *cols) for _ in range(3)]
        assert lib.ZSTDMI_debugHostWaits(c.cctx) == waits
        assert lib.ZSTDMI_debugDeviceAllocs(c.cctx) == allocs
        assert_same(lay.fetch(outs[-1]), expected_sync("frames256k", tier_entries(131073, 262144, 24, 11), 3)[:8])


# ---- 9. the device-only loop: lengths drawn on the device, sizes straight into the decoder ----
@pytest.mark.parametrize("side_stream", [False, True])
def test_device_only_loop(gpu_lib, side_stream):
    import torch
    lib = gpu_lib
    n, bound = 40, 200000
    pool_host = pool("text") * (n * bound // len(pool("text")) + 1)
    cap = lib.ZSTD_compressBound(bound)
    with make_compressor(1) as c, z.Decompressor() as d:
        c.PrepareBatchAsyncLimits(n, bound)
        # (level 1 writes 64 KiB frames of four 16 KiB blocks: four frames an entry at most)
        d.PrepareBatchAsync(n, cap, n * bound, max_frames=n * chunks(bound, 65536))
        stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            data = torch.from_numpy(np.frombuffer(pool_host[:n * bound], dtype=np.uint8).copy()).cuda()
            gen = torch.Generator(device="cuda"); gen.manual_seed(9)
            lengths = torch.randint(1, bound + 1, (n,), device="cuda", generator=gen, dtype=torch.int64)
            at = torch.cumsum(lengths, 0) - lengths
            slot = torch.arange(n, device="cuda", dtype=torch.int64)
            comp = torch.full((n * (cap + 3),), 0xA5, dtype=torch.uint8, device="cuda")
            back = torch.full((n * (bound + 3),), 0xA5, dtype=torch.uint8, device="cuda")
            comp_at, back_at = comp.data_ptr() + slot * (cap + 3), back.data_ptr() + slot * (bound + 3)
            csizes = compress_batch_async(c, data.data_ptr() + at, lengths, comp_at, torch.full((n,), cap, dtype=torch.int64, device="cuda"))
            dsizes = decompress_batch_async(d, comp_at, csizes, back_at, torch.full((n,), bound, dtype=torch.int64, device="cuda"))
            same = torch.equal(dsizes, lengths)
        torch.cuda.synchronize()            # the one wait, at the very end
        assert same, (dsizes.cpu().tolist(), lengths.cpu().tolist())
        lengths_h, at_h, back_h = lengths.cpu().numpy(), at.cpu().numpy(), back.cpu().numpy()
        for i in range(n):
            row = back_h[i * (bound + 3):(i + 1) * (bound + 3)]
            assert row[:lengths_h[i]].tobytes() == pool_host[at_h[i]:at_h[i] + lengths_h[i]], i
            assert (row[lengths_h[i]:] == 0xA5).all(), i


# ---- 10. refusals that need the device, staleness, the two prepares replacing each other, a context freed with work in flight ----
def test_refusals_staleness_and_replacement(gpu_lib):
    lib = gpu_lib
    unsupported, stage_wrong, out_of_bound = (ZSTD_ErrorCode.ZSTD_error_parameter_unsupported, ZSTD_ErrorCode.ZSTD_error_stage_wrong,
                                              ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound)
    raises = base._raises
    with make_compressor(3, ((ZSTD_c_enableLongDistanceMatching, 1),)) as c:
        raises(unsupported, c.PrepareBatchAsyncLimits, 4, 262144)
    with make_compressor(3) as c:
        c.single_frame = True
        raises(unsupported, c.PrepareBatchAsyncLimits, 4, 262144)
    with make_compressor(3, ((ZSTD_c_windowLog, 12),)) as c:
        raises(unsupported, c.PrepareBatchAsyncLimits, 4, 8192)
        c.PrepareBatchAsyncLimits(4, 4096)              # (one window: the one-block state)
        assert c.batch_async_plan == (4096, 0, 4)
    with make_compressor(3) as c:
        c.entropy_carry = True
        raises(unsupported, c.PrepareBatchAsyncLimits, 4, 262144)
        c.PrepareBatchAsyncLimits(4, 65536)             # (one block: the switch takes no effect there)
    with make_compressor(1) as c:
        assert lib.ZSTDMI_CCtx_setHistory(c.cctx, 16384, 0) == 0
        raises(unsupported, c.PrepareBatchAsyncLimits, 4, 262144)
    with make_compressor(3) as c:
        raises(out_of_bound, c.PrepareBatchAsyncLimits, 4, 262144, 5)          # (one entry of the bound needs six blocks of 48 KiB)
        raises(stage_wrong, lambda: c.batch_async_plan)
    entries = tier_entries(131073, 262144, 24, 11)[:4]
    small = tuple(piece(i, 3000 + i) for i in range(4))
    want, want_small = expected_sync("frames256k", tier_entries(131073, 262144, 24, 11), 3)[:4], expected_sync("frames-small", small, 3)
    lay, lay_small = Layout(lib, entries), Layout(lib, small)
    with make_compressor(3) as c:
        c.PrepareBatchAsyncLimits(2, 262144)
        raises(stage_wrong, compress_batch_async, c, *lay.columns())             # n > maxEntries
        compress_batch_async(c, *lay.columns(2))
        c.SetParameter(ZSTD_c_checksumFlag, 0)                                    # (the value it had: any setter invalidates)
        raises(stage_wrong, compress_batch_async, c, *lay.columns(2))
        raises(stage_wrong, lambda: c.batch_async_plan)
        c.PrepareBatchAsyncLimits(4, 262144)
        assert_same(lay.fetch(compress_batch_async(c, *lay.columns())), want)
        c.PrepareBatchAsync(4, 4096)                                              # the first prepare replaces the second ...
        assert c.batch_async_plan == (65536, 0, 4)
        assert_same(lay_small.fetch(compress_batch_async(c, *lay_small.columns())), want_small)
        assert lay.fetch(compress_batch_async(c, *lay.columns())) == [SRC_WRONG] * 4     # (... and its bound holds)
        c.PrepareBatchAsyncLimits(4, 262144)                                      # and back
        assert_same(lay.fetch(compress_batch_async(c, *lay.columns())), want)
        raises(unsupported, c.PrepareBatchAsync, 4, 65537)                        # a refused prepare of either kind leaves none
        raises(stage_wrong, compress_batch_async, c, *lay.columns())
        lay.assert_nothing_else_written()


def test_dispose_straight_after_a_call(gpu_lib):
    lib = gpu_lib
    entries = tier_entries(131073, 262144, 24, 11)
    lay = Layout(lib, entries)
    cols = lay.columns()
    c = make_compressor(5)
    c.PrepareBatchAsyncLimits(len(entries), 262144)
    out = compress_batch_async(c, *cols)
    c.Dispose()                              # (nothing synchronised first: the context waits for its own work)
    assert_same(lay.fetch(out), expected_sync("frames256k", entries, 5))
