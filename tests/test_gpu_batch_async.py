"""GPU tests of ZSTDMI_CCtx_prepareBatchAsync / ZSTDMI_compressBatchAsync (include/zstd_mi355x.h "a batch enqueued from the device")
through the C ABI and batch.compress_batch_async: the five arrays are CUDA tensors, the call only enqueues, and what arrives is —
for entries in the tier of the prepared bound — byte for byte what ZSTDMI_compressBatch writes on a second context with the same setup.

Layout as in test_gpu_batch.py: sources carved from one tensor in shuffled order at whatever alignment that gives, destinations from one
tensor filled with 0xA5 at odd offsets with 64 guard bytes or more between them; everything outside the reported results must still
be 0xA5 afterwards."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import datagen
import oracle_lib
import zstdsharp_amd as z
from zstdsharp_amd.batch import compress_batch, compress_batch_async
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_train as mgt  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ZSTD_c_windowLog, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 101, 200, 201
TOO_SMALL, SRC_WRONG, DST_NULL = -70, -72, -74
KINDS = ["text", "zipf", "rand", "zeros", "pysrc"]
EDGE_SIZES = [1, 2, 255, 256, 257, 4095, 4096]
MAX_ENTRIES = 300


@functools.lru_cache(maxsize=None)
def python_source():
    """Python source text: this suite's own helper modules, one behind the other"""
    return b"".join(open(os.path.join(HERE, name), "rb").read() for name in ("datagen.py", "oracle_lib.py", "forge_cases.py", "zstd_forge.py"))


@functools.lru_cache(maxsize=None)
def data_of(kind, n, seed):
    if kind == "pysrc":
        src = python_source()
        at = (seed * 977) % (len(src) - n)
        return src[at:at + n]
    return datagen.gen(kind, n, seed)


@functools.lru_cache(maxsize=None)
def small_entries():
    """300 entries of at most 4096 bytes (all in the tier up to 16 KiB): every edge size of every kind, then seeded sizes"""
    out = [data_of(kind, n, n + 5) for n in EDGE_SIZES for kind in KINDS]
    rng = np.random.default_rng(2024)
    while len(out) < MAX_ENTRIES:
        out.append(data_of(KINDS[len(out) % len(KINDS)], int(rng.integers(1, 4097)), len(out)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def large_entries():
    """24 entries of 16 385 .. 65 536 bytes (the tier above 16 KiB)"""
    rng = np.random.default_rng(77)
    sizes = [16385, 65536, 65535, 32768] + [int(x) for x in rng.integers(16385, 65537, 20)]
    return tuple(data_of(KINDS[i % len(KINDS)], n, 300 + i) for i, n in enumerate(sizes))


@functools.lru_cache(maxsize=None)
def mixed_entries():
    """64 entries of 1 .. 65 536 bytes on both sides of the 16 KiB line"""
    rng = np.random.default_rng(99)
    sizes = [1, 16384, 16385, 65536] + [int(x) for x in rng.integers(1, 16385, 30)] + [int(x) for x in rng.integers(16385, 65537, 30)]
    return tuple(data_of(KINDS[i % len(KINDS)], n, 500 + i) for i, n in enumerate(sizes))


def golden_bytes(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def make_compressor(level, params=()):
    c = z.Compressor(level)
    for p, v in params:
        c.SetParameter(p, v)
    return c


class Layout:
    """Sources and destinations on the device; the four input columns as CUDA int64 tensors."""

    def __init__(self, lib, entries, caps=None, seed=1):
        import torch
        self.torch, self.lib, self.entries, self.n = torch, lib, entries, len(entries)
        self.caps = list(caps) if caps is not None else [lib.ZSTD_compressBound(len(e)) for e in entries]
        order = np.random.default_rng(seed).permutation(self.n)
        self.src_at = [0] * self.n
        at, parts = 3, [bytes(3)]
        for i in order:
            self.src_at[i] = at
            parts.append(entries[i]); parts.append(bytes(5))
            at += len(entries[i]) + 5
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).cuda()
        self.dst_at, at = [], 1
        for cap in self.caps:
            self.dst_at.append(at)
            at = (at + cap + 64) | 1
        self.dst = torch.full((at + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.src_ptr = [self.src.data_ptr() + a for a in self.src_at]
        self.dst_ptr = [self.dst.data_ptr() + a for a in self.dst_at]
        self.sizes = [len(e) for e in entries]

    def columns(self, n=None):
        t = self.torch
        n = self.n if n is None else n
        return [t.tensor(col[:n], dtype=t.int64, device="cuda") for col in (self.src_ptr, self.sizes, self.dst_ptr, self.caps)]

    def run_async(self, compressor, n=None):
        """enqueue, then — the test's business, not the call's — wait and fetch -> [bytes, or the error code as a negative number]"""
        cols = self.columns(n)
        out = compress_batch_async(compressor, *cols)
        return self.fetch(out)

    def fetch(self, out):
        self.torch.cuda.synchronize()
        self.got = [int(x) for x in out.cpu().tolist()]
        self.host = self.dst.cpu().numpy()
        return [self.host[self.dst_at[i]:self.dst_at[i] + g].tobytes() if g >= 0 else g for i, g in enumerate(self.got)]

    def run_sync(self, compressor, n=None):
        n = self.n if n is None else n
        got = (ctypes.c_size_t * n)()
        self.torch.cuda.synchronize()
        r = self.lib.ZSTDMI_compressBatch(compressor.cctx, (ctypes.c_void_p * n)(*self.src_ptr[:n]), (ctypes.c_size_t * n)(*self.sizes[:n]), n,
                                          (ctypes.c_void_p * n)(*self.dst_ptr[:n]), (ctypes.c_size_t * n)(*self.caps[:n]), got)
        assert r == 0, r
        host = self.dst.cpu().numpy()
        return [-get_error_code(g) if is_error(g) else host[self.dst_at[i]:self.dst_at[i] + g].tobytes() for i, g in enumerate(got)]

    def assert_nothing_else_written(self):
        rest = self.host.copy()
        for i, g in enumerate(self.got):
            if g >= 0:
                assert g <= self.caps[i], i
                rest[self.dst_at[i]:self.dst_at[i] + g] = 0xA5
        bad = np.flatnonzero(rest != 0xA5)
        assert bad.size == 0, f"bytes outside the reported results were written, first at {bad[:4]}"


_expected = {}


def expected_sync(key, entries, level, params=()):
    """the synchronous batch's bytes on a context of its own, computed once per (key, level, params)"""
    k = (key, level, params)
    if k not in _expected:
        lib = z._ffi.load()
        with make_compressor(level, params) as c:
            _expected[k] = Layout(lib, entries, seed=7).run_sync(c)
            assert lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
    return _expected[k]


def assert_same(got, want):
    assert len(got) == len(want)
    diff = [i for i in range(len(want)) if got[i] != want[i]]
    assert not diff, f"entries {diff[:8]} differ from the synchronous batch ({len(diff)} of {len(want)})"


# ---- 1. same tier: bytes equal to the synchronous batch ----
@pytest.mark.parametrize("level", [1, 3, 5])
@pytest.mark.parametrize("bound", [4096, 65536])
def test_same_tier_bytes_equal_sync_batch(gpu_lib, level, bound):
    lib = gpu_lib
    entries = small_entries() if bound == 4096 else large_entries()
    want = expected_sync(bound, entries, level)
    assert all(isinstance(w, bytes) for w in want)
    with make_compressor(level) as c:
        c.PrepareBatchAsync(len(entries), bound)
        lay = Layout(lib, entries)
        got = lay.run_async(c)
        assert_same(got, want)
        lay.assert_nothing_else_written()


# ---- 2. n at the kernel edges ----
def test_entry_counts_at_the_kernel_edges(gpu_lib):
    lib = gpu_lib
    entries = small_entries()
    want = expected_sync(4096, entries, 3)
    with make_compressor(3) as c:
        c.PrepareBatchAsync(MAX_ENTRIES, 4096)
        for n in (1, 255, 256, 257, MAX_ENTRIES):
            lay = Layout(lib, entries[:n], seed=n)
            assert_same(lay.run_async(c), want[:n])
            lay.assert_nothing_else_written()


# ---- 3. mixed tiers: valid streams, no byte identity claimed ----
def test_mixed_tiers_decode_under_both_decoders(gpu_lib, capsys):
    lib = gpu_lib
    entries = mixed_entries()
    with make_compressor(3) as c, z.Decompressor() as d:
        c.PrepareBatchAsync(len(entries), 65536)
        lay = Layout(lib, entries)
        got = lay.run_async(c)
        lay.assert_nothing_else_written()
        for i, (g, e) in enumerate(zip(got, entries)):
            assert isinstance(g, bytes), (i, g)
            assert len(g) <= lib.ZSTD_compressBound(len(e)), i
            assert d.Unwrap(g) == e, i
            assert oracle_lib.decompress(g, len(e)) == e, i
    sync_total = sum(len(x) for x in expected_sync("mixed", entries, 3))
    with capsys.disabled():
        print(f"\n[mixed tiers, level 3, 64 entries] async {sum(len(g) for g in got)} B, synchronous batch {sync_total} B, input {sum(map(len, entries))} B")


# ---- 4. per-entry verdicts ----
@pytest.mark.parametrize("checksum", [0, 1])
def test_per_entry_verdicts(gpu_lib, checksum):
    lib = gpu_lib
    params = ((ZSTD_c_checksumFlag, checksum),)
    good = small_entries()[:40:3]           # 14 good entries
    want_good = expected_sync(("verdicts", checksum), good, 3, params)
    with make_compressor(3, params) as ref:
        empty = ref.Wrap(b"")
    # between the good ones: 0 = one byte short, 1 = size bound + 1, 2 = size 0, 3 = capacity 0, 4 = NULL destination, 5 = NULL source
    entries, kind = [], []
    bad_at = {2: 0, 5: 1, 6: 2, 9: 3, 11: 4, 13: 5}
    victim = small_entries()[50]
    want_victim = expected_sync(("victim", checksum), (victim,), 3, params)[0]
    for i, e in enumerate(good):
        if i in bad_at:
            entries.append(victim if bad_at[i] != 2 else b""); kind.append(bad_at[i])
        entries.append(e); kind.append(None)
    caps = [lib.ZSTD_compressBound(len(e)) for e in entries]
    with make_compressor(3, params) as c:
        c.PrepareBatchAsync(len(entries), 4096)
        for i, k in enumerate(kind):
            if k == 0:
                caps[i] = len(want_victim) - 1
            elif k == 3:
                caps[i] = 0
            elif k == 2:
                caps[i] = len(empty)            # (exactly the room the empty frame needs)
        lay = Layout(lib, entries, caps=caps)
        for i, k in enumerate(kind):
            if k == 1:
                lay.sizes[i] = 4097
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
    lay.assert_nothing_else_written()       # (every canary: behind each destination, and the whole of each failed entry's)


# ---- 5. no host round trip ----
def test_no_host_wait_and_no_allocation_across_async_calls(gpu_lib):
    lib = gpu_lib
    entries = small_entries()[:64]
    with make_compressor(3) as c:
        c.PrepareBatchAsync(64, 4096)
        lay = Layout(lib, entries)
        cols = lay.columns()
        waits, allocs = lib.ZSTDMI_debugHostWaits(c.cctx), lib.ZSTDMI_debugDeviceAllocs(c.cctx)
        assert allocs > 0                    # (the prepare sized the workspaces: the counter counts)
        outs = [compress_batch_async(c, *cols) for _ in range(3)]
        assert lib.ZSTDMI_debugHostWaits(c.cctx) == waits
        assert lib.ZSTDMI_debugDeviceAllocs(c.cctx) == allocs
        got = lay.fetch(outs[-1])
        assert_same(got, expected_sync(4096, small_entries(), 3)[:64])
        lay.run_sync(c)
        assert lib.ZSTDMI_debugHostWaits(c.cctx) > waits
        assert lib.ZSTDMI_debugDeviceAllocs(c.cctx) == allocs       # (64 entries of one block again: nothing grows)


# ---- 6. in-stream use: the host never holds a length ----
@pytest.mark.parametrize("side_stream", [False, True])
def test_in_stream_use(gpu_lib, side_stream):
    import torch
    n, bound = 200, 4096
    pool_host = data_of("text", n * bound, 31)
    with make_compressor(1) as c, z.Decompressor() as d:
        c.PrepareBatchAsync(n, bound)
        cap = c.GetCompressBound(bound)
        stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            pool = torch.from_numpy(np.frombuffer(pool_host, dtype=np.uint8).copy()).cuda()
            gen = torch.Generator(device="cuda"); gen.manual_seed(5)
            lengths = torch.randint(1, bound + 1, (n,), device="cuda", generator=gen, dtype=torch.int64)
            srcs = pool.data_ptr() + torch.cumsum(lengths, 0) - lengths
            dst = torch.full((n * (cap + 3),), 0xA5, dtype=torch.uint8, device="cuda")
            dsts = dst.data_ptr() + torch.arange(n, device="cuda", dtype=torch.int64) * (cap + 3)
            caps = torch.full((n,), cap, dtype=torch.int64, device="cuda")
            out = compress_batch_async(c, srcs, lengths, dsts, caps)
            total = out.clamp(min=0).sum()
        torch.cuda.synchronize()            # the one wait, at the very end
        lengths_h, out_h, dst_h = lengths.cpu().numpy(), out.cpu().numpy(), dst.cpu().numpy()
        assert int(total) == int(out_h.sum()) and (out_h > 0).all()
        at = 0
        for i in range(n):
            frame = dst_h[i * (cap + 3):i * (cap + 3) + out_h[i]].tobytes()
            assert d.Unwrap(frame) == pool_host[at:at + lengths_h[i]], i
            assert (dst_h[i * (cap + 3) + out_h[i]:(i + 1) * (cap + 3)] == 0xA5).all(), i
            at += int(lengths_h[i])


# ---- 7. back to back, then a synchronous call on the same context ----
def test_back_to_back_then_synchronous(gpu_lib):
    lib = gpu_lib
    want = expected_sync(4096, small_entries(), 3)
    first, second, third = small_entries()[:100], small_entries()[100:200], small_entries()[200:300]
    with make_compressor(3) as c:
        c.PrepareBatchAsync(100, 4096)
        a, b = Layout(lib, first, seed=3), Layout(lib, second, seed=4)
        out_a = compress_batch_async(c, *a.columns())
        out_b = compress_batch_async(c, *b.columns())       # (no synchronisation in between)
        items = compress_batch(c, list(third))              # the synchronous wrapper, same context
        assert_same(a.fetch(out_a), want[:100])
        assert_same(b.fetch(out_b), want[100:200])
        a.assert_nothing_else_written(); b.assert_nothing_else_written()
    with make_compressor(3) as fresh:
        assert items == compress_batch(fresh, list(third))
    assert_same(items, want[200:300])


# ---- 8. dictionaries ----
DICT_SETUPS = ["staged-tail", "dict-index", "dict-index-entropy", "cdict"]


def _dict_compressor(setup, dic, keep):
    if setup == "cdict":
        c = z.Compressor(3)
        keep.append(z.CDict(dic, 3))
        c.RefCDict(keep[-1])
        return c
    c = z.Compressor(3 if setup == "staged-tail" else 1)
    if setup != "staged-tail":
        c.dict_index = True
    if setup == "dict-index-entropy":
        c.dict_entropy = True
    c.LoadDictionary(dic)
    return c


@pytest.mark.parametrize("setup", DICT_SETUPS)
def test_dictionaries(gpu_lib, setup):
    lib = gpu_lib
    dic = golden_bytes("train_default_json.dict")
    recs = tuple(r for r in mgt.json_records(1200, 77)[1000:] if len(r) <= 2048)[:120]
    assert len(recs) == 120
    keep = []
    with _dict_compressor(setup, dic, keep) as ref:
        want = Layout(lib, recs, seed=7).run_sync(ref)
    with _dict_compressor(setup, dic, keep) as c, z.Decompressor() as d:
        c.PrepareBatchAsync(len(recs), 2048)
        lay = Layout(lib, recs)
        got = lay.run_async(c)
        assert_same(got, want)
        lay.assert_nothing_else_written()
        d.LoadDictionary(dic)
        for g, r in zip(got[::7], recs[::7]):
            assert d.Unwrap(g) == r
            assert oracle_lib.decompress(g, len(r), dic) == r
    for k in keep:
        k.Dispose()


# ---- 9. checksum, no content size, a window of one block ----
def test_frame_parameters(gpu_lib):
    lib = gpu_lib
    params = ((ZSTD_c_checksumFlag, 1), (ZSTD_c_contentSizeFlag, 0), (ZSTD_c_windowLog, 12))
    entries = small_entries()[:120]
    want = expected_sync("params", entries, 3, params)
    with make_compressor(3, params) as c, z.Decompressor() as d:
        c.PrepareBatchAsync(len(entries), 4096)
        lay = Layout(lib, entries)
        got = lay.run_async(c)
        assert_same(got, want)
        lay.assert_nothing_else_written()
        assert d.Unwrap(got[-1]) == entries[-1]


# ---- 10. refusals, staleness, and a context freed with work in flight ----
def _raises(code, fn, *args):
    with pytest.raises(ZstdException) as e:
        fn(*args)
    assert e.value.code == code, e.value.code


def test_refusals_and_staleness(gpu_lib):
    lib = gpu_lib
    stage_wrong, unsupported = ZSTD_ErrorCode.ZSTD_error_stage_wrong, ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
    entries = small_entries()[:20]
    lay = Layout(lib, entries)
    with make_compressor(3) as c:
        _raises(stage_wrong, compress_batch_async, c, *lay.columns())           # no prepare
        c.PrepareBatchAsync(10, 4096)
        _raises(stage_wrong, compress_batch_async, c, *lay.columns())           # n > maxEntries
        compress_batch_async(c, *lay.columns(10))
        c.SetParameter(ZSTD_c_checksumFlag, 0)                                   # (the value it had: any setter invalidates)
        _raises(stage_wrong, compress_batch_async, c, *lay.columns(10))
        c.PrepareBatchAsync(10, 4096)
        compress_batch_async(c, *lay.columns(10))
        c.LoadDictionary(golden_bytes("rawcontent_6000.dict"))
        _raises(stage_wrong, compress_batch_async, c, *lay.columns(10))
        c.PrepareBatchAsync(20, 4096)
        out = compress_batch_async(c, *lay.columns())
        assert all(isinstance(g, bytes) for g in lay.fetch(out))
        _raises(unsupported, c.PrepareBatchAsync, 10, 65537)
        _raises(stage_wrong, compress_batch_async, c, *lay.columns(10))         # (a refused prepare leaves none)
        _raises(unsupported, c.PrepareBatchAsync, 10, 0)
        c.seek_table = True
        _raises(unsupported, c.PrepareBatchAsync, 10, 4096)
        c.seek_table = False
        c.RefPrefix(b"some prefix of more than eight bytes")
        _raises(unsupported, c.PrepareBatchAsync, 10, 4096)


def test_dispose_straight_after_an_async_call(gpu_lib):
    lib = gpu_lib
    entries = small_entries()[:200]
    lay = Layout(lib, entries)
    cols = lay.columns()
    c = make_compressor(5)
    c.PrepareBatchAsync(len(entries), 4096)
    out = compress_batch_async(c, *cols)
    c.Dispose()                              # (nothing synchronised first: the context waits for its own work)
    assert_same(lay.fetch(out), expected_sync(4096, small_entries(), 5)[:200])
