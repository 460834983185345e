"""GPU tests of ZSTDMI_compressBatch and ZSTDMI_decompressBatch: every entry's size (or error code) and bytes are exactly what the
single device call gives for that entry alone on another context with the same parameters, the entries the batched pass is for
do take it (ZSTDMI_debugLastBatchAlone / ..AloneD), and nothing outside an entry's result is touched.

Layout of every test: all destinations are carved from one tensor filled with 0xA5, start at odd offsets and have at least 64 guard
bytes between them; everything outside the bytes an entry reports as written must still be 0xA5 afterwards.  Sources are carved from
one tensor in shuffled order, at whatever alignment that gives."""
import ctypes
import functools
import os

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [0, 1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 1000, 4095, 4096, 4097, 16383, 16384, 16385, 65535, 65536, 65537, 200000]
MATRIX_KINDS = ["text", "zipf", "rand", "zeros"]
ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag, ZSTD_c_dictIDFlag, ZSTD_c_enableLongDistanceMatching = 200, 201, 202, 160
TOO_SMALL = (1 << 64) - 70
# name -> (level, ((parameter, value), ...))
CONFIGS = {
    "level-5": (-5, ()), "level1": (1, ()), "level3": (3, ()), "level5": (5, ()),
    "level3-checksum": (3, ((ZSTD_c_checksumFlag, 1),)), "level3-no-content-size": (3, ((ZSTD_c_contentSizeFlag, 0),)),
    "level3-ldm": (3, ((ZSTD_c_enableLongDistanceMatching, 1),)),
}


@functools.lru_cache(maxsize=None)
def data_of(kind, n, seed):
    return datagen.gen(kind, n, seed)


@functools.lru_cache(maxsize=None)
def matrix_entries():
    return tuple(data_of(kind, n, n + 11) for n in SIZES for kind in MATRIX_KINDS)


def make_compressor(level, params=(), dict_bytes=None):
    c = z.Compressor(level)
    for p, v in params:
        c.SetParameter(p, v)
    if dict_bytes is not None:
        c.LoadDictionary(dict_bytes)
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

    def run(self, cctx):
        srcs = (ctypes.c_void_p * self.n)(*[self.src.data_ptr() + a for a in self.src_at])
        sizes = (ctypes.c_size_t * self.n)(*[len(e) for e in self.entries])
        dsts = (ctypes.c_void_p * self.n)(*[self.dst.data_ptr() + a for a in self.dst_at])
        caps = (ctypes.c_size_t * self.n)(*self.caps)
        r = getattr(self.lib, self.call)(cctx, srcs, sizes, self.n, dsts, caps, self.got)
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


def single_results(lib, cctx, entries, caps=None):
    """every entry through ZSTDMI_compressDevice alone -> bytes, or the error code as a negative number"""
    import torch
    out = []
    room = torch.empty(lib.ZSTD_compressBound(max(len(e) for e in entries)) + 64, dtype=torch.uint8, device="cuda")
    for i, e in enumerate(entries):
        src = torch.from_numpy(np.frombuffer(e or b"\0", dtype=np.uint8).copy()).cuda()
        cap = caps[i] if caps is not None else lib.ZSTD_compressBound(len(e))
        torch.cuda.synchronize()
        r = lib.ZSTDMI_compressDevice(cctx, room.data_ptr(), cap, src.data_ptr(), len(e))
        out.append(-get_error_code(r) if is_error(r) else room[:r].cpu().numpy().tobytes())
    return out


_matrix_cache = {}


def matrix_singles(lib, name):
    """the matrix entries compressed one by one under configuration `name`, on a context of their own (computed once per run)"""
    if name not in _matrix_cache:
        level, params = CONFIGS[name]
        c = make_compressor(level, params)
        _matrix_cache[name] = single_results(lib, c.cctx, matrix_entries())
        c.Dispose()
    return _matrix_cache[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_identity_with_single_calls(gpu_lib, oracle, name):
    entries = matrix_entries()
    want = matrix_singles(gpu_lib, name)
    level, params = CONFIGS[name]
    c = make_compressor(level, params)
    b = Batch(gpu_lib, entries)
    assert b.run(c.cctx) == 0
    for i, e in enumerate(entries):
        assert not isinstance(want[i], int), (i, len(e), want[i])
        assert b.result(i) == want[i], (name, i, len(e), "differs from the single call")
        assert oracle.decompress(want[i], len(e)) == e, (name, i, len(e))
    b.assert_nothing_else_written()
    # a condition, not a measurement: every entry of one block took the batched pass
    assert 0 <= gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) <= sum(1 for e in entries if len(e) == 0 or len(e) > 65536)
    c.Dispose()


@pytest.mark.parametrize("dict_file", ["rawcontent_6000.dict", "trained_16k.dict"])
@pytest.mark.parametrize("dict_id_flag", [1, 0])
def test_identity_with_dictionaries(gpu_lib, oracle, dict_file, dict_id_flag):
    import torch
    dict_bytes = open(os.path.join(GOLDEN, dict_file), "rb").read()
    sizes = [100, 333, 1000, 4096, 5000, 12289, 16384, 20000, 32768, 40000]
    entries = [data_of(kind, n, n + 5) for n in sizes for kind in ("text", "zipf", "mixed")]
    params = ((ZSTD_c_dictIDFlag, dict_id_flag),)
    ref = make_compressor(3, params, dict_bytes)
    want = single_results(gpu_lib, ref.cctx, entries)
    c = make_compressor(3, params, dict_bytes)
    b = Batch(gpu_lib, entries, seed=2)
    assert b.run(c.cctx) == 0
    d = z.Decompressor(); d.LoadDictionary(dict_bytes)
    for i, e in enumerate(entries):
        assert b.result(i) == want[i], (dict_file, i, len(e))
        out = torch.empty(len(e), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r = gpu_lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), len(e), b.dst.data_ptr() + b.dst_at[i], b.got[i])
        assert r == len(e) and out.cpu().numpy().tobytes() == e, (dict_file, i, len(e))
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0           # (every entry here is one block behind the dictionary)
    round_trip(gpu_lib, [b.result(i) for i in range(len(entries))], entries, seed=12, dict_bytes=dict_bytes)
    for x in (ref, c, d):
        x.Dispose()


def test_capacity_per_entry(gpu_lib):
    entries = matrix_entries()
    want = matrix_singles(gpu_lib, "level3")
    caps = [len(w) - 1 if i % 3 == 0 else len(w) for i, w in enumerate(want)]      # (the others: exactly the true size)
    c = make_compressor(3)
    b = Batch(gpu_lib, entries, caps=caps, seed=3)
    assert b.run(c.cctx) == 0
    for i in range(len(entries)):
        if i % 3 == 0:
            assert b.got[i] == TOO_SMALL, (i, len(entries[i]))
        else:
            assert b.result(i) == want[i], (i, len(entries[i]))
    b.assert_nothing_else_written()                                  # (guards, and everything of the entries that did not fit)
    c.Dispose()


SLICE_KINDS = ("text", "zipf", "rand", "mixed", "runs")


def sliced_entries(rng, count, lo, hi):
    """`count` entries of lo <= size < hi bytes, of mixed kinds: slices of one MiB of each kind"""
    pool = {k: data_of(k, 1 << 20, 77) for k in SLICE_KINDS}
    out = []
    for i in range(count):
        n = int(rng.integers(lo, hi)); at = int(rng.integers(0, (1 << 20) - n))
        out.append(pool[SLICE_KINDS[i % 5]][at:at + n])
    return out


def frame_header_size(blob):
    fhd = blob[4]
    single, fcs = (fhd >> 5) & 1, fhd >> 6
    return 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0) if fcs == 0 else 1 << fcs)


def single_decodes(lib, dctx, blobs, caps):
    """every blob through ZSTDMI_decompressDevice alone -> bytes, or the error code as a negative number"""
    import torch
    out = []
    room = torch.empty(max(caps) + 64, dtype=torch.uint8, device="cuda")
    for blob, cap in zip(blobs, caps):
        src = torch.from_numpy(np.frombuffer(blob or b"\0", dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        r = lib.ZSTDMI_decompressDevice(dctx, room.data_ptr(), cap, src.data_ptr(), len(blob))
        out.append(-get_error_code(r) if is_error(r) else room[:r].cpu().numpy().tobytes())
    return out


def round_trip(lib, blobs, entries, seed, dict_bytes=None):
    """the compressed entries back through ZSTDMI_decompressBatch (capacities exactly the content sizes), all in the batched pass"""
    d = z.Decompressor()
    if dict_bytes is not None:
        d.LoadDictionary(dict_bytes)
    b = Batch(lib, blobs, caps=[len(e) for e in entries], seed=seed, call="ZSTDMI_decompressBatch")
    assert b.run(d.dctx) == 0
    for i, e in enumerate(entries):
        assert b.result(i) == e, (i, len(e))
    b.assert_nothing_else_written()
    assert lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == 0
    d.Dispose()


@functools.lru_cache(maxsize=None)
def record_pool():
    return tuple(data_of("text", 3000, 100 + k) for k in range(16))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025])
def test_entry_counts_at_the_edges(gpu_lib, oracle, n):
    pool = record_pool()
    ref = make_compressor(1)
    want = single_results(gpu_lib, ref.cctx, pool)
    entries = [pool[(i * 7) % 16] for i in range(n)]
    c = make_compressor(1)
    b = Batch(gpu_lib, entries, seed=n)
    assert b.run(c.cctx) == 0
    for i in range(n):
        assert b.result(i) == want[(i * 7) % 16], (n, i)
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
    for k in range(16):
        assert oracle.decompress(want[k], 3000) == pool[k]
    round_trip(gpu_lib, [b.result(i) for i in range(n)], entries, seed=n + 1)
    ref.Dispose(); c.Dispose()


def test_several_passes(gpu_lib, oracle):
    rng = np.random.default_rng(8)
    entries = sliced_entries(rng, 300, 1, 9000)
    c = make_compressor(3)
    assert gpu_lib.ZSTDMI_CCtx_setPassChunks(c.cctx, 64) == 0
    b = Batch(gpu_lib, entries, seed=4)
    assert b.run(c.cctx) == 0
    picks = sorted(rng.choice(300, 32, replace=False).tolist())
    ref = make_compressor(3)
    want = single_results(gpu_lib, ref.cctx, [entries[i] for i in picks])
    for k, i in enumerate(picks):
        assert b.result(i) == want[k], i
    for i, e in enumerate(entries):
        assert oracle.decompress(b.result(i), len(e)) == e, i
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
    round_trip(gpu_lib, [b.result(i) for i in range(300)], entries, seed=9)
    ref.Dispose(); c.Dispose()


def test_many_small_entries(gpu_lib, oracle):
    rng = np.random.default_rng(2024)
    entries = sliced_entries(rng, 3000, 512, 8193)
    c = make_compressor(1)
    b = Batch(gpu_lib, entries, seed=5)
    assert b.run(c.cctx) == 0
    first = [b.result(i) for i in range(3000)]
    assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
    b.assert_nothing_else_written()
    for i, e in enumerate(entries):
        assert oracle.decompress(first[i], len(e)) == e, i
    picks = sorted(rng.choice(3000, 200, replace=False).tolist())
    ref = make_compressor(1)
    want = single_results(gpu_lib, ref.cctx, [entries[i] for i in picks])
    for k, i in enumerate(picks):
        assert first[i] == want[k], i
    b2 = Batch(gpu_lib, entries, seed=5)                             # determinism: the same call again
    assert b2.run(c.cctx) == 0
    assert all(b2.result(i) == first[i] for i in range(3000))
    round_trip(gpu_lib, first, entries, seed=10)
    ref.Dispose(); c.Dispose()


def test_context_untouched(gpu_lib):
    data = data_of("text", 300000, 9)
    c = make_compressor(3); d = z.Decompressor()
    before = c.Wrap(data)
    b = Batch(gpu_lib, list(record_pool()), seed=6)
    assert b.run(c.cctx) == 0
    pool = list(record_pool())
    assert d.Unwrap(before) == data
    round_blobs = [b.result(i) for i in range(len(pool))]
    db = Batch(gpu_lib, round_blobs, caps=[len(e) for e in pool], seed=6, call="ZSTDMI_decompressBatch")
    assert db.run(d.dctx) == 0 and all(db.result(i) == pool[i] for i in range(len(pool)))
    after = c.Wrap(data)
    assert after == before and d.Unwrap(after) == data
    c.Dispose(); d.Dispose()


def test_several_device_workers_are_refused(gpu_lib, oracle):
    c = make_compressor(1)
    devs = (ctypes.c_int * 2)(0, 0)
    assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, devs, 2) == 0
    b = Batch(gpu_lib, list(record_pool())[:4], seed=7)
    r = b.run(c.cctx)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
    assert (b.host == 0xA5).all()
    c.Dispose()
    d = z.Decompressor()
    assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, devs, 2) == 0
    blobs = [oracle.compress(e, 1, 0, 0) for e in list(record_pool())[:4]]
    b = Batch(gpu_lib, blobs, caps=[3000] * 4, seed=7, call="ZSTDMI_decompressBatch")
    r = b.run(d.dctx)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
    assert (b.host == 0xA5).all()
    d.Dispose()


def test_python_mirror(gpu_lib):
    import torch
    items = [data_of("text", 3000, 1), b"", data_of("zipf", 70000, 2), bytearray(data_of("mixed", 9000, 3)), data_of("text", 200000, 4)]
    with z.Compressor(3) as c, z.Decompressor() as d:
        out = z.compress_batch(c, items)
        assert len(out) == len(items) and all(isinstance(o, bytes) for o in out)
        for o, e in zip(out, items):
            assert d.Unwrap(o) == bytes(e)
            assert o == c.Wrap(bytes(e))
        tensors = [torch.from_numpy(np.frombuffer(bytes(e) or b"\0", dtype=np.uint8).copy()).cuda()[:len(e)] for e in items]
        tout = z.compress_batch(c, tensors)
        assert [t.cpu().numpy().tobytes() for t in tout] == out
        assert z.compress_batch(c, []) == [] and z.decompress_batch(d, [], []) == []
        assert z.decompress_batch(d, out, [len(e) for e in items]) == [bytes(e) for e in items]
        back = z.decompress_batch(d, tout, [len(e) + 7 for e in items])
        assert [t.cpu().numpy().tobytes() for t in back] == [bytes(e) for e in items]
        damaged = list(out)
        damaged[2] = damaged[2][:-1]
        with pytest.raises(ZstdException) as err:
            z.decompress_batch(d, damaged, [len(e) for e in items])
        assert "item 2" in str(err.value)
        with pytest.raises(TypeError):
            z.compress_batch(c, [items[0], tensors[0]])


def test_decompress_identity_on_foreign_frames(gpu_lib, oracle, golden, golden_dict):
    """Frames of other encoders (libzstd at levels 1 .. 19, multi-frame, skippable, checksummed, streams without a content size) and
    oracle-built ones: sizes and bytes equal the single call's; only the entries holding an unsized frame are decoded alone."""
    text = data_of("text", 300000, 21)
    blobs = [open(c["path"], "rb").read() for c in golden]
    unsized = [c for c in golden_dict if not c.get("dict")]
    blobs += [c["blob"] for c in unsized]
    blobs += [oracle.compress(text, 1, 0, 0), oracle.compress(text, 5, 1, 0)]
    assert all(isinstance(x, bytes) for x in blobs)
    blobs += [bytes([0x5A, 0x2A, 0x4D, 0x18, 5, 0, 0, 0]) + b"hello" + oracle.compress(text[:7000], 1, 0, 0), b""]
    caps = [(1 << 20) + 4096] * len(blobs)
    ref = z.Decompressor()
    want = single_decodes(gpu_lib, ref.dctx, blobs, caps)
    assert all(not isinstance(w, int) for w in want)
    assert want[len(golden) + len(unsized)] == text and want[-2] == text[:7000] and want[-1] == b""
    d = z.Decompressor()
    b = Batch(gpu_lib, blobs, caps=caps, seed=13, call="ZSTDMI_decompressBatch")
    assert b.run(d.dctx) == 0
    for i in range(len(blobs)):
        assert b.result(i) == want[i], (i, len(blobs[i]))
    b.assert_nothing_else_written()
    assert all(c.get("unsized") for c in unsized) and len(unsized) >= 4
    assert gpu_lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == len(unsized)
    ref.Dispose(); d.Dispose()


def test_decompress_identity_with_a_formatted_dictionary(gpu_lib, golden_dict):
    cases = [c for c in golden_dict if c.get("dict") == "trained_16k.dict"]
    assert len(cases) >= 5
    blobs = [c["blob"] for c in cases]
    caps = [c["n"] for c in cases]
    ref = z.Decompressor(); ref.LoadDictionary(cases[0]["dict_bytes"])
    want = single_decodes(gpu_lib, ref.dctx, blobs, caps)
    assert all(not isinstance(w, int) and len(w) == c["n"] for w, c in zip(want, cases))
    d = z.Decompressor(); d.LoadDictionary(cases[0]["dict_bytes"])
    b = Batch(gpu_lib, blobs, caps=caps, seed=14, call="ZSTDMI_decompressBatch")
    assert b.run(d.dctx) == 0
    for i in range(len(blobs)):
        assert b.result(i) == want[i], cases[i]["file"]
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == 0
    ref.Dispose(); d.Dispose()


def test_damage_among_good_entries(gpu_lib, oracle, golden_dict):
    """40 good entries, eight of them damaged (one kind each, fixed by seed): every damaged entry answers with the single call's error
    code, every good one is restored exactly.  (Nothing here is meant to fault: the decoder bounds every read and write itself.)"""
    rng = np.random.default_rng(31)
    entries = sliced_entries(rng, 40, 2000, 30000)
    blobs = [oracle.compress(e, 1 + (i % 2) * 2, 1 if i % 4 == 3 else 0, 0) for i, e in enumerate(entries)]
    assert all(isinstance(x, bytes) for x in blobs)
    caps = [len(e) for e in entries]
    blobs[2] = blobs[2][:-1]                                         # cut by one byte
    blobs[5] = blobs[5][:5]                                          # cut inside the header
    blobs[8] = b"\x00\x01\x02\x03" + blobs[8][4:]                    # magic overwritten
    assert blobs[11][4] & 4                                          # (a checksummed frame)
    flip = bytearray(blobs[11]); flip[len(flip) // 2] ^= 0x10; blobs[11] = bytes(flip)      # a byte flipped in its middle
    flip = bytearray(blobs[14]); flip[frame_header_size(blobs[14])] ^= 0x06; blobs[14] = bytes(flip)     # the first block header: another block type
    blobs[17] = blobs[17] + b"\x00"                                   # one trailing byte
    caps[20] -= 1                                                    # capacity = content - 1
    blobs[23] = next(c["blob"] for c in golden_dict if c.get("dict") == "trained_16k.dict" and c["n"] == 5000)   # names a dictID, none loaded
    caps[23] = 5000
    damaged = (2, 5, 8, 11, 14, 17, 20, 23)
    ref = z.Decompressor()
    want = single_decodes(gpu_lib, ref.dctx, blobs, caps)
    for i in range(40):
        assert isinstance(want[i], int) == (i in damaged), (i, want[i] if isinstance(want[i], int) else len(want[i]))
    d = z.Decompressor()
    b = Batch(gpu_lib, blobs, caps=caps, seed=15, call="ZSTDMI_decompressBatch")
    assert b.run(d.dctx) == 0
    for i in range(40):
        assert b.result(i) == want[i], (i, b.result(i) if isinstance(b.result(i), int) else "bytes", want[i] if isinstance(want[i], int) else "bytes")
        if i not in damaged:
            assert b.result(i) == entries[i], i
    b.assert_nothing_else_written()
    assert gpu_lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == 0
    ref.Dispose(); d.Dispose()
