"""GPU tests of ZSTDMI_compressPack: n device buffers into ONE seekable stream.  The stream must be, byte for byte, the frames
Compressor.Wrap writes for every entry alone, one entry's behind the other's, and one seek table of all their entries behind the last.

The expected stream is built without the call under test: every entry goes through Wrap with seek_table on, on another context with
the same configuration; read_seek_table splits the result into frames and table entries; expected = all frames + make_table(all
entries).  (An entry above 64 KiB under single_frame is refused a table by Wrap — it is one frame: its entry is (frame bytes, size).)

Layout of every call: d_dst starts HEAD (an odd number of) bytes into a buffer filled with 0xA5; everything in front of d_dst and at or
beyond d_dst + dstCapacity must still be 0xA5 afterwards.  Sources are carved from one tensor in shuffled order, at odd places."""
import ctypes
import functools
import os
import struct
import sys

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_train as mgt  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD, TAIL, CANARY = 37, 64, 0xA5
ZSTD_c_windowLog, ZSTD_c_minMatch, ZSTD_c_enableLongDistanceMatching = 101, 105, 160
ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 200, 201
TOO_SMALL, UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall, ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
SRC_WRONG = ZSTD_ErrorCode.ZSTD_error_srcSize_wrong
SIZES = [0, 1, 7, 300, 4095, 4096, 4097, 65535, 65536, 65537, 300000]
KINDS = ["text", "zipf", "rand"]

# name -> keyword arguments of make_compressor
CONFIGS = {
    "level1": dict(level=1), "level3": dict(level=3), "level5": dict(level=5),
    "checksum": dict(level=3, params=((ZSTD_c_checksumFlag, 1),)),
    "no-content-size": dict(level=3, params=((ZSTD_c_contentSizeFlag, 0),)),
    "windowlog12": dict(level=1, params=((ZSTD_c_windowLog, 12),)),
    "raw-dictionary": dict(level=1, dic="rawcontent_6000.dict"),
    "formatted-dictionary": dict(level=3, dic="trained_16k.dict"),
    "dict-entropy": dict(level=1, dic="trained_16k.dict", entropy=True),
    "dict-index-raw": dict(level=1, dic="rawcontent_6000.dict", index=True),
    "dict-index-formatted": dict(level=1, dic="trained_16k.dict", index=True, entropy=True),
    "ldm": dict(level=3, params=((ZSTD_c_enableLongDistanceMatching, 1),)),
    "single-frame": dict(level=3, single=True),
}


def golden_bytes(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def make_compressor(level=3, params=(), dic=None, entropy=False, index=False, single=False, pass_chunks=None):
    c = z.Compressor(level)
    for p, v in params:
        c.SetParameter(p, v)
    if dic is not None:
        c.LoadDictionary(golden_bytes(dic))
    if entropy:
        c.dict_entropy = True
    if index:
        c.dict_index = True
    if single:
        c.single_frame = True
    if pass_chunks is not None:
        assert z._ffi.load().ZSTDMI_CCtx_setPassChunks(c.cctx, pass_chunks) == 0
    return c


def make_table(entries):
    """the seek table of `entries` = [(cSize, dSize), ...]: 8-byte entries, descriptor 0"""
    body = b"".join(struct.pack("<II", c, d) for c, d in entries)
    return struct.pack("<II", 0x184D2A5E, len(body) + 9) + body + struct.pack("<IBI", len(entries), 0, 0x8F92EAB1)


def alone(c, entry):
    """-> (the frames Wrap writes for the entry, its table entries), on the compressor c"""
    try:
        c.seek_table = True
        blob = c.Wrap(entry)
    except ZstdException as e:
        # one frame per call has no table of its own (include/zstd_mi355x.h, ZSTDMI_CCtx_setSingleFrame): the entry is that one frame
        assert c.single_frame and len(entry) > 65536 and e.code == UNSUPPORTED, e
        c.seek_table = False
        frame = c.Wrap(entry)
        return frame, [(len(frame), len(entry))]
    finally:
        c.seek_table = False
    rows, table_bytes = z.read_seek_table(blob)
    return blob[:len(blob) - table_bytes], rows


def expected_of(entries, **config):
    """-> (the expected stream, its table entries)"""
    frames, rows = [], []
    with make_compressor(**config) as c:
        for e in entries:
            f, r = alone(c, e)
            frames.append(f)
            rows += r
    return b"".join(frames) + make_table(rows), rows


@functools.lru_cache(maxsize=None)
def data_of(kind, n, seed):
    return datagen.gen(kind, n, seed)


@functools.lru_cache(maxsize=None)
def matrix_entries():
    out = [data_of(kind, n, n + 17) for n in SIZES for kind in KINDS]
    out.insert(20, data_of("rand", 4 << 20, 99))
    return tuple(out)


class Pack:
    """the sources on the device (shuffled, odd places), and a canary-filled destination per call"""

    def __init__(self, lib, entries, seed=1, null_sources=()):
        import torch
        self.torch, self.lib, self.entries, self.n = torch, lib, list(entries), len(entries)
        order = np.random.default_rng(seed).permutation(self.n)
        at, parts, self.src_at = 3, [bytes(3)], [0] * self.n
        for i in order:
            self.src_at[i] = at
            parts.append(self.entries[i]); parts.append(bytes(5))
            at += len(self.entries[i]) + 5
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).cuda()
        self.sizes = [len(e) for e in self.entries]
        self.ptrs = [None if (i in null_sources or not self.sizes[i]) else self.src.data_ptr() + self.src_at[i] for i in range(self.n)]
        self.bound = lib.ZSTDMI_packBound((ctypes.c_size_t * max(self.n, 1))(*self.sizes), self.n)
        assert not is_error(self.bound)

    def run(self, cctx, cap=None):
        """-> the stream's bytes, or the error code as a negative number; the canary is checked either way"""
        torch = self.torch
        cap = self.bound if cap is None else cap
        dst = torch.full((HEAD + cap + TAIL,), CANARY, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r = self.lib.ZSTDMI_compressPack(cctx, dst.data_ptr() + HEAD, cap, (ctypes.c_void_p * max(self.n, 1))(*self.ptrs),
                                         (ctypes.c_size_t * max(self.n, 1))(*self.sizes), self.n)
        host = dst.cpu().numpy()
        assert (host[:HEAD] == CANARY).all(), "bytes in front of d_dst were written"
        bad = np.flatnonzero(host[HEAD + cap:] != CANARY)
        assert bad.size == 0, f"bytes at or beyond d_dst + dstCapacity were written, first at capacity + {bad[:4]}"
        if is_error(r):
            return -get_error_code(r)
        assert r <= cap
        return host[HEAD:HEAD + r].tobytes()


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], dtype=np.uint8) != np.frombuffer(b[:n], dtype=np.uint8))
    return f"lengths {len(a)} / {len(b)}, first difference at {d[0] if d.size else n}"


def batch_alone(lib, cctx, pack):
    """ZSTDMI_debugLastBatchAlone of the same entries through ZSTDMI_compressBatch"""
    import torch
    caps = [lib.ZSTD_compressBound(s) for s in pack.sizes]
    starts = np.concatenate([[0], np.cumsum(caps)])
    out = torch.empty(int(starts[-1]) + 1, dtype=torch.uint8, device="cuda")
    got = (ctypes.c_size_t * pack.n)()
    torch.cuda.synchronize()
    r = lib.ZSTDMI_compressBatch(cctx, (ctypes.c_void_p * pack.n)(*pack.ptrs), (ctypes.c_size_t * pack.n)(*pack.sizes), pack.n,
                                 (ctypes.c_void_p * pack.n)(*[out.data_ptr() + int(s) for s in starts[:-1]]), (ctypes.c_size_t * pack.n)(*caps), got)
    assert r == 0
    return lib.ZSTDMI_debugLastBatchAlone(cctx)


# ---------------------------------------------------------------- identity ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_pack_is_the_entries_alone_side_by_side(gpu_lib, name):
    entries = matrix_entries()
    want, rows = expected_of(entries, **CONFIGS[name])
    pack = Pack(gpu_lib, entries, seed=len(name))
    with make_compressor(**CONFIGS[name]) as c:
        got = pack.run(c.cctx)
        assert not isinstance(got, int), got
        assert got == want, first_difference(got, want)
        assert gpu_lib.ZSTDMI_debugLastPackFrames(c.cctx) == len(rows)
        took_alone = gpu_lib.ZSTDMI_debugLastPackAlone(c.cctx)
        assert took_alone == batch_alone(gpu_lib, c.cctx, pack)
        assert took_alone >= len(KINDS)         # (the empty entries at least)
        assert took_alone < len(entries)        # (and the batched rounds did run)
    assert z.read_seek_table(got)[0] == rows


# ---------------------------------------------------------------- entry counts at the edges of the scan and the gather ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_records():
    """4097 records of 1 .. 300 bytes, and what Wrap writes for each"""
    text, r = data_of("text", 700000, 5), np.random.default_rng(6)
    recs, at = [], 0
    for _ in range(4097):
        n = int(r.integers(1, 301))
        recs.append(text[at:at + n])
        at += n
    frames, rows = [], []
    with make_compressor(level=3) as c:
        for e in recs:
            f, row = alone(c, e)
            frames.append(f)
            rows += row
    return recs, frames, rows


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 4097])
def test_entry_counts(gpu_lib, n):
    recs, frames, rows = small_records()
    want = b"".join(frames[:n]) + make_table(rows[:n])
    with make_compressor(level=3) as c:
        got = Pack(gpu_lib, recs[:n], seed=n).run(c.cctx)
        assert got == want, first_difference(got, want)
        assert gpu_lib.ZSTDMI_debugLastPackFrames(c.cctx) == n and gpu_lib.ZSTDMI_debugLastPackAlone(c.cctx) == 0


# ---------------------------------------------------------------- rounds and order ----------------------------------------------------------------
def round_entries():
    """about 40 entries of several parameter classes; alone ones (empty; long-distance matching above one block) at the front, in
    between and at the end"""
    sizes = [300, 5000, 20000, 60000, 1, 140, 16384, 16385, 4096, 33000]
    out = [b"", data_of("text", 70000, 1)]
    for k in range(36):
        out.append(data_of(KINDS[k % 3], sizes[k % len(sizes)] + k, 200 + k))
        if k in (4, 5, 17, 30):
            out.append(b"" if k & 1 else data_of("text", 70000 + k, 2))
    return out + [data_of("text", 66000, 3), b""]


def test_rounds_and_order(gpu_lib):
    config = dict(level=3, params=((ZSTD_c_enableLongDistanceMatching, 1),))
    entries = round_entries()
    want, rows = expected_of(entries, pass_chunks=4, **config)
    pack = Pack(gpu_lib, entries, seed=9)
    with make_compressor(pass_chunks=4, **config) as c:
        got = pack.run(c.cctx)
        assert got == want, first_difference(got, want)
        assert gpu_lib.ZSTDMI_debugLastPackFrames(c.cctx) == len(rows)
        assert gpu_lib.ZSTDMI_debugLastPackAlone(c.cctx) == sum(1 for e in entries if len(e) == 0 or len(e) > 65536)
    with make_compressor(**config) as c:        # the default pass size: one round between two alone entries, the same bytes
        whole = pack.run(c.cctx)
    assert got == whole, first_difference(got, whole)


# ---------------------------------------------------------------- capacity ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["level1", "windowlog12"])      # (the long entries: batched rounds; alone, straight to their place)
def test_capacity(gpu_lib, name):
    entries = [data_of("text", 300000, 41), b"", data_of("zipf", 5000, 42), data_of("rand", 70000, 43), data_of("text", 777, 44), data_of("text", 65537, 45)]
    want, rows = expected_of(entries, **CONFIGS[name])
    frames_bytes = sum(c for c, _ in rows)
    assert len(rows) > len(entries)             # (the 300000-byte entry is several frames at level 1)
    pack = Pack(gpu_lib, entries)
    with make_compressor(**CONFIGS[name]) as c:
        assert pack.run(c.cctx) == want         # ZSTDMI_packBound suffices
        assert pack.run(c.cctx, len(want)) == want
        assert pack.run(c.cctx, len(want) - 1) == -TOO_SMALL
        first = rows[0][0]
        for cap in (0, 1, first - 1, first + 3, frames_bytes // 2, frames_bytes - 1):       # ends inside the frames
            assert pack.run(c.cctx, cap) == -TOO_SMALL, cap
        for cap in (frames_bytes, frames_bytes + 16, frames_bytes + 17, len(want) - 8):     # all frames, not the table
            assert pack.run(c.cctx, cap) == -TOO_SMALL, cap
        assert pack.run(c.cctx, len(want)) == want
        empty = Pack(gpu_lib, [])
        assert empty.bound == 17
        assert empty.run(c.cctx, 17) == make_table([])
        assert gpu_lib.ZSTDMI_debugLastPackFrames(c.cctx) == 0
        assert empty.run(c.cctx, 16) == -TOO_SMALL
        assert empty.run(c.cctx) == make_table([])


@pytest.mark.parametrize("name", ["level5", "raw-dictionary", "no-content-size"])
def test_pack_bound_always_suffices(gpu_lib, name):
    """incompressible entries of every size class: the frames come close to ZSTD_compressBound, the table to its bound"""
    entries = [data_of("rand", n, n) for n in (1, 2, 4095, 4096, 4097, 8191, 8192, 65535, 65536, 65537, 131072, 300000)] + [b""] * 3
    pack = Pack(gpu_lib, entries)
    with make_compressor(**CONFIGS[name]) as c:
        got = pack.run(c.cctx)
        assert not isinstance(got, int), got
    assert sum(d for _, d in z.read_seek_table(got)[0]) == sum(pack.sizes)


# ---------------------------------------------------------------- reading back ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["level1", "level3", "checksum", "raw-dictionary", "dict-index-formatted"])
def test_reading_back(gpu_lib, oracle, name):
    entries = [e for e in matrix_entries() if len(e) <= 300000]
    config = CONFIGS[name]
    dic = golden_bytes(config["dic"]) if "dic" in config else None
    sizes = [len(e) for e in entries]
    with make_compressor(**config) as c:
        blob = z.compress_pack(c, entries)
    content = b"".join(entries)
    assert oracle.decompress(blob, len(content), dic) == content
    with z.Decompressor() as d:
        if dic is not None:
            d.LoadDictionary(dic)
        assert d.Unwrap(blob) == content
        ranges = z.pack_ranges(sizes)
        assert len(ranges) == len(entries) and ranges[-1] == (len(content) - sizes[-1], sizes[-1])
        back = d.unwrap_ranges(blob, ranges)
        assert len(back) == len(entries)
        for i, (b, e) in enumerate(zip(back, entries)):
            assert bytes(b) == e, (i, len(e))
        assert bytes(back[sizes.index(0)]) == b""
        i = sizes.index(300)
        assert bytes(d.unwrap_ranges(blob, [ranges[i]])[0]) == entries[i]
        assert gpu_lib.ZSTDMI_debugLastRangesFrames(d.dctx) == 1


def test_json_records_read_back_record_by_record(gpu_lib, oracle):
    recs, dic = mgt.json_records(2000, 77)[1000:], golden_bytes("train_default_json.dict")
    with make_compressor(level=1, dic="train_default_json.dict", index=True) as c:
        blob = z.compress_pack(c, recs)
        assert gpu_lib.ZSTDMI_debugLastPackFrames(c.cctx) == len(recs) and gpu_lib.ZSTDMI_debugLastPackAlone(c.cctx) == 0
    rows = z.read_seek_table(blob)[0]
    assert [d for _, d in rows] == [len(r) for r in recs]
    assert oracle.decompress(blob, sum(len(r) for r in recs), dic) == b"".join(recs)
    with z.Decompressor() as d:
        d.LoadDictionary(dic)
        back = d.unwrap_ranges(blob, z.pack_ranges(len(r) for r in recs))
        for i, (b, r) in enumerate(zip(back, recs)):
            assert bytes(b) == r, i
        assert bytes(d.unwrap_ranges(blob, [z.pack_ranges(len(r) for r in recs)[123]])[0]) == recs[123]
        assert gpu_lib.ZSTDMI_debugLastRangesFrames(d.dctx) == 1


# ---------------------------------------------------------------- errors and refusals ----------------------------------------------------------------
def single_code(lib, cctx, entry):
    """the error ZSTDMI_compressDevice gives for the entry alone"""
    import torch
    src = torch.from_numpy(np.frombuffer(entry, dtype=np.uint8).copy()).cuda()
    dst = torch.empty(lib.ZSTD_compressBound(len(entry)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = lib.ZSTDMI_compressDevice(cctx, dst.data_ptr(), dst.numel(), src.data_ptr(), len(entry))
    assert is_error(r)
    return get_error_code(r)


def test_errors_and_refusals_leave_the_context_as_it_was(gpu_lib):
    import torch
    lib = gpu_lib
    entries = [data_of("text", 3000, 51), data_of("zipf", 70000, 52), b"", data_of("text", 500, 53)]
    probe = data_of("text", 150000, 54)
    pack = Pack(lib, entries)
    with make_compressor(level=1, dic="trained_16k.dict") as c:
        c.seek_table = True
        before = c.Wrap(probe)
        assert z.read_seek_table(before)[1] > 17
        other = Pack(lib, [b"", data_of("text", 100, 55), b""])
        assert batch_refused(lib, c.cctx, other) == UNSUPPORTED        # (the batch under the seek-table switch: still refused)
        c.seek_table = False
        batch_alone_before = batch_alone(lib, c.cctx, other)
        assert batch_alone_before == 2
        c.seek_table = True

        def unchanged():
            assert c.Wrap(probe) == before                          # the seek-table switch, the dictionary, the parameters
            assert lib.ZSTDMI_debugLastBatchAlone(c.cctx) == batch_alone_before

        good = pack.run(c.cctx)                                     # a successful pack: no table per entry although the switch is on
        assert good == expected_of(entries, level=1, dic="trained_16k.dict")[0]
        unchanged()
        # a NULL source with a size
        assert Pack(lib, entries, null_sources=(1,)).run(c.cctx) == -SRC_WRONG
        unchanged()
        # several device workers
        assert lib.ZSTDMI_CCtx_setDevices(c.cctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        assert pack.run(c.cctx) == -UNSUPPORTED
        assert lib.ZSTDMI_CCtx_setDevices(c.cctx, (ctypes.c_int * 1)(0), 1) == 0
        unchanged()
        assert pack.run(c.cctx) == good
    # a refused sticky parameter: the single call's code
    with make_compressor(level=1, params=((ZSTD_c_minMatch, 6),)) as c:
        c.Level = 3
        assert pack.run(c.cctx) == -single_code(lib, c.cctx, entries[0]) == -UNSUPPORTED
        c.Level = 1
        assert pack.run(c.cctx) == expected_of(entries, level=1, params=((ZSTD_c_minMatch, 6),))[0]
    # a pending prefix
    with make_compressor(level=3) as c:
        before = c.Wrap(probe)
        prefix = torch.from_numpy(np.frombuffer(data_of("text", 4000, 56), dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        assert lib.ZSTD_CCtx_refPrefix(c.cctx, prefix.data_ptr(), prefix.numel()) == 0
        assert pack.run(c.cctx) == -UNSUPPORTED
        assert lib.ZSTD_CCtx_refPrefix(c.cctx, None, 0) == 0
        assert c.Wrap(probe) == before
        assert pack.run(c.cctx) == expected_of(entries, level=3)[0]
        assert c.Wrap(probe) == before


def batch_refused(lib, cctx, pack):
    import torch
    out = torch.empty(4096, dtype=torch.uint8, device="cuda")
    got = (ctypes.c_size_t * pack.n)()
    r = lib.ZSTDMI_compressBatch(cctx, (ctypes.c_void_p * pack.n)(*pack.ptrs), (ctypes.c_size_t * pack.n)(*pack.sizes), pack.n,
                                 (ctypes.c_void_p * pack.n)(*[out.data_ptr() + 1024 * i for i in range(pack.n)]), (ctypes.c_size_t * pack.n)(*[1024] * pack.n), got)
    assert is_error(r)
    return get_error_code(r)


# ---------------------------------------------------------------- determinism, the Python mirror ----------------------------------------------------------------
def test_same_call_writes_the_same_bytes(gpu_lib):
    entries = [e for e in matrix_entries() if len(e) <= 300000]
    pack = Pack(gpu_lib, entries, seed=3)
    with make_compressor(level=3) as c:
        a = pack.run(c.cctx)
        b = pack.run(c.cctx)
    with make_compressor(level=3) as c:
        fresh = Pack(gpu_lib, entries, seed=4).run(c.cctx)
    assert not isinstance(a, int) and a == b == fresh


def test_python_mirror(gpu_lib):
    import torch
    entries = [data_of("text", 5000, 61), b"", data_of("zipf", 100000, 62), data_of("rand", 9, 63)]
    want, rows = expected_of(entries, level=3)
    with make_compressor(level=3) as c:
        blob = z.compress_pack(c, entries)
        assert isinstance(blob, bytes) and blob == want
        assert z.read_seek_table(blob)[0] == rows
        tensors = [torch.from_numpy(np.frombuffer(e or b"\0", dtype=np.uint8)[:len(e)].copy()).cuda() for e in entries]
        out = z.compress_pack(c, tensors)
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.numel() == len(want)
        assert out.cpu().numpy().tobytes() == want
        assert z.compress_pack(c, []) == make_table([])
        c.seek_table = True                     # (the context's own switch is not consulted)
        assert z.compress_pack(c, entries) == want
    assert z.pack_ranges([3, 0, 5]) == [(0, 3), (3, 0), (3, 5)] and z.pack_ranges([]) == []
