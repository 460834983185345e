"""GPU tests of ZSTDMI_compressBatch on entries larger than one block: the multi-block frames with history that the default settings
write (levels 1-2: 64 KiB frames of four 16 KiB blocks; levels >= 3: 48 KiB or 32 KiB blocks in 240-256 KiB frames) take the batched
pass (ZSTDMI_debugLastBatchAlone), every entry's size and bytes are exactly what ZSTDMI_compressDevice gives for it alone on a
second context with the same parameters, every result decodes to its input under the oracle's decoder, and nothing outside an
entry's result is touched.  What still goes alone (empty entries, 4 MiB and more, more chunks than a pass, the far-candidate form
of the fast strategy, LDM, windows below 64 KiB) is counted exactly and stays identical to the single call.

Layout as in test_gpu_batch.py: destinations carved from one 0xA5 tensor at odd offsets with guards of 64 bytes or more, sources
carved from one tensor in shuffled order.

The decoder side: every set of results goes back through ZSTDMI_decompressBatch with capacities equal to the content sizes.  The
batched decoder hands an entry holding a frame without a content size to the single-call path (include/zstd_mi355x.h), so under
ZSTD_c_contentSizeFlag = 0 ZSTDMI_debugLastBatchAloneD equals the number of entries; everywhere else it is 0."""
import ctypes
import functools

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import get_error_code, is_error

pytestmark = pytest.mark.gpu

# around each framing's edges: 16 KiB blocks x 4 (levels 1-2), 48 KiB blocks x 5 = 245 760 (levels 3-4), 32 KiB blocks x 8 = 262 144 (level 5)
SIZES = [65537, 81920, 98304, 131072, 131073, 200000, 245760, 245761, 262144, 262145, 300000, 500000]
KINDS = ["text", "zipf", "rand", "zeros", "runs"]
SMALL_SIZES = [1, 4096, 65536, 0]
BIG = (4 << 20) + 1
ZSTD_c_windowLog, ZSTD_c_enableLongDistanceMatching, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 101, 160, 200, 201
TOO_SMALL = (1 << 64) - 70
# name -> (level, ((parameter, value), ...))
CONFIGS = {
    "level1": (1, ()), "level3": (3, ()), "level5": (5, ()),
    "level3-checksum": (3, ((ZSTD_c_checksumFlag, 1),)), "level3-no-content-size": (3, ((ZSTD_c_contentSizeFlag, 0),)),
    "level1-checksum": (1, ((ZSTD_c_checksumFlag, 1),)),
}


@functools.lru_cache(maxsize=None)
def data_of(kind, n, seed):
    return datagen.gen(kind, n, seed)


@functools.lru_cache(maxsize=None)
def frame_entries():
    return tuple(data_of(KINDS[i % len(KINDS)], n, n + 11) for i, n in enumerate(SIZES))


@functools.lru_cache(maxsize=None)
def mixed_entries():
    small = tuple(data_of(KINDS[i % len(KINDS)], n, n + 3) for i, n in enumerate(SMALL_SIZES))
    e = frame_entries()
    return e[:5] + small[:2] + e[5:9] + (data_of("text", BIG, 5),) + small[2:] + e[9:]


def make_compressor(level, params=()):
    c = z.Compressor(level)
    for p, v in params:
        c.SetParameter(p, v)
    return c


class Batch:
    """Sources in one tensor (shuffled order), destinations in another (0xA5, odd starts, guards of 64 bytes or more)."""

    def __init__(self, lib, entries, caps=None, seed=1, call="ZSTDMI_compressBatch"):
        import torch
        self.torch, self.lib, self.entries, self.n, self.call = torch, lib, entries, len(entries), call
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
        self.got = (ctypes.c_size_t * max(self.n, 1))()
        torch.cuda.synchronize()

    def run(self, ctx):
        srcs = (ctypes.c_void_p * self.n)(*[self.src.data_ptr() + a for a in self.src_at])
        sizes = (ctypes.c_size_t * self.n)(*[len(e) for e in self.entries])
        dsts = (ctypes.c_void_p * self.n)(*[self.dst.data_ptr() + a for a in self.dst_at])
        caps = (ctypes.c_size_t * self.n)(*self.caps)
        r = getattr(self.lib, self.call)(ctx, srcs, sizes, self.n, dsts, caps, self.got)
        self.host = self.dst.cpu().numpy()
        return r

    def result(self, i):
        """-> the entry's bytes, or its error code as a negative number"""
        g = self.got[i]
        if is_error(g):
            return -get_error_code(g)
        return self.host[self.dst_at[i]:self.dst_at[i] + g].tobytes()

    def assert_nothing_else_written(self):
        rest = self.host.copy()
        for i in range(self.n):
            if is_error(self.got[i]):      # (a failed entry's destination holds nothing of use; beyond its capacity nothing may change)
                rest[self.dst_at[i]:self.dst_at[i] + self.caps[i]] = 0xA5
            else:
                assert self.got[i] <= self.caps[i], i
                rest[self.dst_at[i]:self.dst_at[i] + self.got[i]] = 0xA5
        bad = np.flatnonzero(rest != 0xA5)
        assert bad.size == 0, f"bytes outside the reported results were written, first at {bad[:4]}"


def single_results(lib, cctx, entries):
    """every entry through ZSTDMI_compressDevice alone -> bytes, or the error code as a negative number"""
    import torch
    out = []
    room = torch.empty(lib.ZSTD_compressBound(max(len(e) for e in entries)) + 64, dtype=torch.uint8, device="cuda")
    for e in entries:
        src = torch.from_numpy(np.frombuffer(e or b"\0", dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        r = lib.ZSTDMI_compressDevice(cctx, room.data_ptr(), lib.ZSTD_compressBound(len(e)), src.data_ptr(), len(e))
        out.append(-get_error_code(r) if is_error(r) else room[:r].cpu().numpy().tobytes())
    return out


_singles = {}


def singles(lib, oracle, name, which):
    """the reference, computed once per run and left unchanged: entries `which` compressed one by one under configuration `name` on a
    context of their own, each checked against the oracle's decoder"""
    key = (name, which)
    if key not in _singles:
        entries = {"frames": frame_entries, "mixed": mixed_entries}[which]()
        level, params = CONFIGS[name]
        c = make_compressor(level, params)
        want = single_results(lib, c.cctx, entries)
        c.Dispose()
        for w, e in zip(want, entries):
            assert not isinstance(w, int), (name, len(e), w)
            assert oracle.decompress(w, len(e)) == e, (name, len(e))
        _singles[key] = want
    return _singles[key]


def round_trip(lib, blobs, entries, seed, alone):
    """compressed entries of at most 4 MiB back through ZSTDMI_decompressBatch, capacities exactly the content sizes"""
    keep = [i for i, b in enumerate(blobs) if len(b) <= 4 << 20]
    blobs, entries = [blobs[i] for i in keep], [entries[i] for i in keep]
    d = z.Decompressor()
    b = Batch(lib, blobs, caps=[len(e) for e in entries], seed=seed, call="ZSTDMI_decompressBatch")
    assert b.run(d.dctx) == 0
    for i, e in enumerate(entries):
        assert b.result(i) == e, (i, len(e))
    b.assert_nothing_else_written()
    assert lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == (len(entries) if alone else 0)
    d.Dispose()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_identity_and_batched_pass(gpu_lib, oracle, name):
    """Bytes equal the single call's, the oracle decodes them (singles), and no entry left the batched pass.  (Before multi-block
    frames were batched, ZSTDMI_debugLastBatchAlone here was the number of entries.)"""
    entries = frame_entries()
    want = singles(gpu_lib, oracle, name, "frames")
    level, params = CONFIGS[name]
    c = make_compressor(level, params)
    b = Batch(gpu_lib, entries)
    assert b.run(c.cctx) == 0
    for i, e in enumerate(entries):
        assert b.result(i) == want[i], (name, i, len(e), "differs from the single call")
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
    c.Dispose()
    round_trip(gpu_lib, [b.result(i) for i in range(len(entries))], entries, seed=21, alone=name == "level3-no-content-size")


@pytest.mark.parametrize("name", ["level1", "level3"])
def test_mixed_batch(gpu_lib, oracle, name):
    """one call over multi-block entries, entries of one block, an empty entry and one of 4 MiB + 1: alone go the empty one and the large one"""
    entries = mixed_entries()
    want = singles(gpu_lib, oracle, name, "mixed")
    level, params = CONFIGS[name]
    c = make_compressor(level, params)
    b = Batch(gpu_lib, entries, seed=2)
    assert b.run(c.cctx) == 0
    for i, e in enumerate(entries):
        assert b.result(i) == want[i], (name, i, len(e), "differs from the single call")
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == sum(1 for e in entries if len(e) == 0 or len(e) >= 4 << 20) == 2
    c.Dispose()
    round_trip(gpu_lib, [b.result(i) for i in range(len(entries))], entries, seed=22, alone=False)


def test_capacity_per_entry(gpu_lib, oracle):
    """an entry of several chunks that does not fit writes nothing of any of them — its whole destination, up to its capacity, still
    holds the fill (batch_place gives every one of its chunks the offset `span`) — and its neighbours are untouched by it"""
    entries = frame_entries()
    want = singles(gpu_lib, oracle, "level3", "frames")
    caps = [len(w) - 1 if i % 3 == 0 else len(w) for i, w in enumerate(want)]      # (the others: exactly the true size)
    c = make_compressor(3)
    b = Batch(gpu_lib, entries, caps=caps, seed=3)
    assert b.run(c.cctx) == 0
    for i in range(len(entries)):
        if i % 3 == 0:
            assert b.got[i] == TOO_SMALL, (i, len(entries[i]))
            mine = b.host[b.dst_at[i]:b.dst_at[i] + caps[i]]
            assert mine.size == caps[i] and (mine == 0xA5).all(), (i, len(entries[i]), "an entry that did not fit was partly written")
        else:
            assert b.result(i) == want[i], (i, len(entries[i]))
    b.assert_nothing_else_written()                                  # (guards, and what lies behind the results of the entries that fit)
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
    c.Dispose()


def test_pass_boundaries(gpu_lib, oracle):
    """passes of 16 chunks hold whole entries (2 to 11 chunks of 48 KiB each here); one entry of 18 chunks exceeds a pass and goes alone"""
    long_entry = data_of("text", 850000, 6)
    entries = frame_entries() + (long_entry,)

    def sixteen(lib, c):
        assert lib.ZSTDMI_CCtx_setPassChunks(c.cctx, 16) == 0
    ref = make_compressor(3)
    sixteen(gpu_lib, ref)
    want = single_results(gpu_lib, ref.cctx, entries)
    ref.Dispose()
    c = make_compressor(3)
    sixteen(gpu_lib, c)
    b = Batch(gpu_lib, entries, seed=4)
    assert b.run(c.cctx) == 0
    for i, e in enumerate(entries):
        assert b.result(i) == want[i], (i, len(e), "differs from the single call")
        assert oracle.decompress(want[i], len(e)) == e, (i, len(e))
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == sum(1 for e in entries if (len(e) + 49151) // 49152 > 16) == 1
    c.Dispose()


# (level, sizes, batched passes, entries alone) under ZSTDMI_CCtx_setPassChunks(4).  Level 3: chunks of 48 KiB in multi-block frames,
# around one chunk, one pass and one chunk more than a pass.  Level 1: one chunk of 64 KiB up to 64 KiB, above it blocks of 16 KiB.
# The counts are ZSTDMI_debugLastBatchPasses / ZSTDMI_debugLastBatchAlone as measured on an MI355X with the library of the commit
# before compress_entries became a sequence of steps over zmi_batch_pass.h (2026-10-21): the cut and the groups are to stay as they were.
_CB3 = 49152
FOUR_CHUNK_PASSES = [
    (3, (1, _CB3 - 1, _CB3, _CB3 + 1, 2 * _CB3, 3 * _CB3 + 1, 4 * _CB3, 4 * _CB3 + 1, 0), 5, 2),
    (1, (65536, 70000, 1000), 2, 1),
]


@pytest.mark.parametrize("level,sizes,passes,alone", FOUR_CHUNK_PASSES, ids=["level3", "level1"])
def test_passes_of_four_chunks(gpu_lib, oracle, level, sizes, passes, alone):
    """passes of at most four chunks: every entry's bytes are the single call's, and the call makes the passes and leaves the entries
    alone that it made and left before the host loop was cut into steps"""
    entries = tuple(data_of(KINDS[i % len(KINDS)], n, n + 17) for i, n in enumerate(sizes))
    ctxs = []
    for _ in range(2):
        c = make_compressor(level)
        assert gpu_lib.ZSTDMI_CCtx_setPassChunks(c.cctx, 4) == 0
        ctxs.append(c)
    ref, c = ctxs
    want = single_results(gpu_lib, ref.cctx, entries)
    b = Batch(gpu_lib, entries, seed=7)
    assert b.run(c.cctx) == 0
    for i, e in enumerate(entries):
        assert b.result(i) == want[i], (level, i, len(e), "differs from the single call")
        assert oracle.decompress(want[i], len(e)) == e, (level, i, len(e))
    b.assert_nothing_else_written()
    got = (gpu_lib.ZSTDMI_debugLastBatchPasses(c.cctx), gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx))
    print(f"four-chunk passes, level {level}: passes {got[0]} alone {got[1]}")
    assert got == (passes, alone)
    ref.Dispose(); c.Dispose()


def far_candidates(lib, c):
    assert lib.ZSTDMI_CCtx_setHistory(c.cctx, 16384, 0) == 0


def history_32k_frames_128k(lib, c):
    assert lib.ZSTDMI_CCtx_setHistory(c.cctx, 32768, 131072) == 0


@pytest.mark.parametrize("level,params,setup", [
    (3, (), history_32k_frames_128k),                                # 32 KiB blocks, 4 per frame
    (3, ((ZSTD_c_windowLog, 17),), None),                            # 48 KiB blocks, 2 per frame (a frame stays inside the 128 KiB window)
], ids=["level3-history32k-frames128k", "level3-windowlog17"])
def test_other_frame_shapes(gpu_lib, oracle, level, params, setup):
    """blocks per frame that the defaults never produce (ZSTDMI_CCtx_setHistory(h > 0, frameBytes), ZSTD_c_windowLog >= 16): the same
    table form, identity with the single call and the batched pass for every entry"""
    entries = frame_entries()
    ctxs = []
    for _ in range(2):
        c = make_compressor(level, params)
        if setup:
            setup(gpu_lib, c)
        ctxs.append(c)
    ref, c = ctxs
    want = single_results(gpu_lib, ref.cctx, entries)
    b = Batch(gpu_lib, entries, seed=6)
    assert b.run(c.cctx) == 0
    for i, e in enumerate(entries):
        assert b.result(i) == want[i], (i, len(e), "differs from the single call")
        assert oracle.decompress(want[i], len(e)) == e, (i, len(e))
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
    ref.Dispose(); c.Dispose()
    round_trip(gpu_lib, [b.result(i) for i in range(len(entries))], entries, seed=23, alone=False)


@pytest.mark.parametrize("level,params,setup", [
    (1, (), far_candidates),                                         # the fast strategy's full 64 KiB blocks with far candidates
    (3, ((ZSTD_c_enableLongDistanceMatching, 1),), None),
    (3, ((ZSTD_c_windowLog, 12),), None),
], ids=["level1-history16k", "level3-ldm", "windowlog12"])
def test_what_goes_alone_stays_correct(gpu_lib, oracle, level, params, setup):
    entries = [data_of(kind, 200000, 31 + k) for k, kind in enumerate(("text", "zipf", "runs"))]
    ctxs = []
    for _ in range(2):
        c = make_compressor(level, params)
        if setup:
            setup(gpu_lib, c)
        ctxs.append(c)
    ref, c = ctxs
    want = single_results(gpu_lib, ref.cctx, entries)
    b = Batch(gpu_lib, entries, seed=5)
    assert b.run(c.cctx) == 0
    for i, e in enumerate(entries):
        assert b.result(i) == want[i], (i, "differs from the single call")
        assert oracle.decompress(want[i], len(e)) == e, i
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 3
    ref.Dispose(); c.Dispose()
