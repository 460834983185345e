"""GPU tests of ZSTDMI_DCtx_prepareBatchAsync / ZSTDMI_decompressBatchAsync (include/zstd_mi355x.h "the decompress counterpart")
through the C ABI and batch.decompress_batch_async: the five arrays are CUDA tensors, the call only enqueues, and what arrives is —
per entry, size or error code and bytes — what ZSTDMI_decompressBatch gives on a second context with the same setup and
ZSTDMI_DCtx_setBatchUnsized(1), but for the header's four exceptions (a size above the bound, the limits, unsized frames always in
the shared pass, no origin path).

Layout of every call (DLayout): sources carved from one tensor in shuffled order at whatever alignment that gives, destinations from one
tensor filled with 0xA5 at odd offsets with 64 guard bytes or more between them; everything outside the bytes an entry reports as
written — for a failed entry: outside its capacity — must still be 0xA5 afterwards.  (Nothing here is meant to fault: the decoder
bounds every read and write itself.)"""
import ctypes
import functools
import os

import numpy as np
import pytest

import datagen
import forge_cases
import zstd_forge as forge
import zstdsharp_amd as z
from zstdsharp_amd.batch import compress_batch_async, decompress_batch_async
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 200, 201
PREFIX_UNKNOWN, WRONG_DICT, WS_TOO_SMALL, TOO_SMALL, SRC_WRONG = -10, -32, -66, -70, -72
MAX_ENTRIES = 1024


@functools.lru_cache(maxsize=None)
def data_of(kind, n, seed):
    return datagen.gen(kind, n, seed)


@functools.lru_cache(maxsize=None)
def golden_bytes(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


_compressors = {}


@functools.lru_cache(maxsize=None)
def wrap(data, level=3, checksum=0, content_size=1, dictionary=None, single_frame=False):
    """data through this compressor (one context per setup, kept for the run)"""
    key = (level, checksum, content_size, dictionary, single_frame)
    if key not in _compressors:
        c = z.Compressor(level)
        c.SetParameter(ZSTD_c_checksumFlag, checksum)
        c.SetParameter(ZSTD_c_contentSizeFlag, content_size)
        if dictionary is not None:
            c.LoadDictionary(golden_bytes(dictionary))
        if single_frame:
            c.single_frame = True
        _compressors[key] = c
    return _compressors[key].Wrap(data)


# ---- what a run of sized frames holds, read from its bytes (RFC 8878): the numbers the limits are about ----
def _nb_seq(body):
    b = bytes(body) + bytes(8)
    kind, lhl = b[0] & 3, (b[0] >> 2) & 3
    lhc = int.from_bytes(b[:4], "little")
    if kind >= 2:
        if lhl <= 1:
            at = 3 + ((lhc >> 14) & 0x3FF)
        elif lhl == 2:
            at = 4 + (lhc >> 18)
        else:
            at = 5 + (lhc >> 22) + (b[4] << 10)
    else:
        lh, size = (1, b[0] >> 3) if lhl in (0, 2) else (2, (lhc & 0xFFFF) >> 4) if lhl == 1 else (3, (lhc & 0xFFFFFF) >> 4)
        at = lh + (size if kind == 0 else 1)
    n = b[at]
    if n == 0xFF:
        return b[at + 1] + (b[at + 2] << 8) + 0x7F00
    return ((n - 0x80) << 8) + b[at + 1] if n > 0x7F else n


def frame_counts(blob):
    """-> (frames, blocks, content bytes, sequences) of a run of frames that all carry a content size (skippable frames count nothing)"""
    pos = frames = blocks = content = seqs = 0
    while pos < len(blob):
        magic = int.from_bytes(blob[pos:pos + 4], "little")
        if (magic & 0xFFFFFFF0) == forge.SKIP_MAGIC:
            pos += 8 + int.from_bytes(blob[pos + 4:pos + 8], "little")
            continue
        assert magic == forge.MAGIC
        fhd = blob[pos + 4]
        single, fcs, did = (fhd >> 5) & 1, fhd >> 6, (0, 1, 2, 4)[fhd & 3]
        at = pos + 5 + (0 if single else 1) + did
        assert fcs or single, "a frame without a content size"
        width = 1 if fcs == 0 else 1 << fcs
        content += int.from_bytes(blob[at:at + width], "little") + (256 if fcs == 1 else 0)
        q = at + width
        while True:
            bh = int.from_bytes(blob[q:q + 3], "little")
            last, kind, size = bh & 1, (bh >> 1) & 3, bh >> 3
            if kind == 2:
                seqs += _nb_seq(blob[q + 3:q + 3 + size])
            q += 3 + (1 if kind == 1 else size)
            blocks += 1
            if last:
                break
        pos = q + (4 if fhd & 4 else 0)
        frames += 1
    return frames, blocks, content, seqs


def total_counts(blobs):
    return tuple(sum(x) for x in zip(*[frame_counts(b) for b in blobs]))


class DLayout:
    """Sources and destinations on the device; the four input columns as CUDA int64 tensors."""

    def __init__(self, blobs, caps, seed=1):
        import torch
        self.torch, self.blobs, self.n, self.caps = torch, list(blobs), len(blobs), list(caps)
        order = np.random.default_rng(seed).permutation(self.n)
        self.src_at = [0] * self.n
        at, parts = 3, [bytes(3)]
        for i in order:
            self.src_at[i] = at
            parts.append(self.blobs[i]); parts.append(bytes(5))
            at += len(self.blobs[i]) + 5
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).cuda()
        self.dst_at, at = [], 1
        for cap in self.caps:
            self.dst_at.append(at)
            at = (at + cap + 64) | 1
        self.dst = torch.full((at + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.src_ptr = [self.src.data_ptr() + a for a in self.src_at]
        self.dst_ptr = [self.dst.data_ptr() + a for a in self.dst_at]
        self.sizes = [len(b) for b in self.blobs]

    def columns(self, n=None):
        t = self.torch
        n = self.n if n is None else n
        return [t.tensor(col[:n], dtype=t.int64, device="cuda") for col in (self.src_ptr, self.sizes, self.dst_ptr, self.caps)]

    def run_async(self, d, n=None):
        """enqueue, then — the test's business, not the call's — wait and fetch -> [bytes, or the error code as a negative number]"""
        return self.fetch(decompress_batch_async(d, *self.columns(n)))

    def fetch(self, out):
        self.torch.cuda.synchronize()
        self.got = [int(x) for x in out.cpu().tolist()]
        self.host = self.dst.cpu().numpy()
        return [self.host[self.dst_at[i]:self.dst_at[i] + g].tobytes() if g >= 0 else g for i, g in enumerate(self.got)]

    def run_sync(self, d, n=None, wait=True):
        n = self.n if n is None else n
        lib, got = d._lib, (ctypes.c_size_t * n)()
        if wait:
            self.torch.cuda.synchronize()      # (a reference context runs on a stream of its own)
        r = lib.ZSTDMI_decompressBatch(d.dctx, (ctypes.c_void_p * n)(*[p or None for p in self.src_ptr[:n]]), (ctypes.c_size_t * n)(*self.sizes[:n]), n,
                                       (ctypes.c_void_p * n)(*[p or None for p in self.dst_ptr[:n]]), (ctypes.c_size_t * n)(*self.caps[:n]), got)
        assert r == 0, r
        self.got = [-get_error_code(g) if is_error(g) else int(g) for g in got]
        self.host = self.dst.cpu().numpy()
        return [self.host[self.dst_at[i]:self.dst_at[i] + g].tobytes() if g >= 0 else g for i, g in enumerate(self.got)]

    def assert_canaries(self, untouched=()):
        """nothing outside the reported results (a failed entry: outside its capacity; `untouched`: not a byte of these entries)"""
        rest = self.host.copy()
        for i, g in enumerate(self.got):
            if i in untouched:
                continue
            if g >= 0:
                assert g <= self.caps[i], i
                rest[self.dst_at[i]:self.dst_at[i] + g] = 0xA5
            elif self.dst_ptr[i]:
                rest[self.dst_at[i]:self.dst_at[i] + self.caps[i]] = 0xA5
        bad = np.flatnonzero(rest != 0xA5)
        assert bad.size == 0, f"bytes outside the reported results were written, first at {bad[:4]}"


def sync_context(setup=None):
    d = z.Decompressor()
    d.batch_unsized = True
    if setup:
        setup(d)
    return d


def prepared(max_entries, bound, content, frames=0, blocks=0, seqs=0, setup=None, lit=0):
    d = z.Decompressor()
    if setup:
        setup(d)
    assert d._lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, lit) == 0
    d.PrepareBatchAsync(max_entries, bound, content, frames, blocks, seqs)
    return d


def assert_same(got, want):
    assert len(got) == len(want)
    diff = [i for i in range(len(want)) if got[i] != want[i]]
    assert not diff, f"entries {diff[:8]} differ from the synchronous batch ({len(diff)} of {len(want)}): {[(got[i] if isinstance(got[i], int) else len(got[i]), want[i] if isinstance(want[i], int) else len(want[i])) for i in diff[:4]]}"


# ---- 1. parity with the synchronous batch ----
def forged(blocks):
    """a frame written field by field (zstd_forge) -> (frame, capacity = its content's length, content)"""
    frame, content = forge.frame(blocks)
    return frame, len(content), content


@functools.lru_cache(maxsize=None)
def parity_mix():
    """-> (blobs, capacities, the content each entry must regenerate)"""
    text4k, text256k, one = data_of("text", 4096, 11), data_of("text", 256 << 10, 12), b"Z"
    a, b = data_of("text", 3000, 13), data_of("zipf", 2500, 14)
    unsized_data = data_of("text", 5000, 15)
    unsized = wrap(unsized_data, content_size=0)
    assert unsized[4] >> 6 == 0 and not (unsized[4] >> 5) & 1           # no content size, a window descriptor
    unsized = unsized[:5] + bytes([(19 - 10) << 3]) + unsized[6:]       # (the window restated as 2^19: its bound is blocks x 128 KiB)
    golden = golden_bytes("text_70000_l5.zst")
    multi = wrap(text256k, single_frame=True)
    assert frame_counts(multi)[0] == 1 and frame_counts(multi)[1] > 1     # one frame of several blocks
    entries = [
        (wrap(b""), 0, b""), (wrap(one), 1, one),
        forged([{"t": "raw", "data": data_of("rand", 4096, 16)}]), forged([{"t": "rle", "byte": 65, "size": 4096}]),
        (wrap(text4k), 4096, text4k),
        (multi, len(text256k), text256k),
        (wrap(a) + forge.skippable(3, b"not content") + wrap(b), len(a) + len(b), a + b),
        (wrap(text4k, checksum=1), 4096 + 7, text4k),
        (unsized, len(unsized_data), unsized_data),                       # capacity far below the bound, exactly the content
        (golden, 70000, None),
    ]
    return tuple(e[0] for e in entries), tuple(e[1] for e in entries), tuple(e[2] for e in entries)


@functools.lru_cache(maxsize=None)
def parity_expected():
    blobs, caps, content = parity_mix()
    with sync_context() as d:
        want = DLayout(blobs, caps, seed=7).run_sync(d)
    for w, c in zip(want, content):
        assert isinstance(w, bytes) and (c is None or w == c)
    return tuple(want)


@pytest.mark.parametrize("lit", [0, 1, 2, 3])
def test_parity_with_the_synchronous_batch(gpu_lib, lit):
    blobs, caps, _ = parity_mix()
    want = parity_expected()
    with prepared(16, 256 << 10, 1 << 20, frames=32, lit=lit) as d:
        lay = DLayout(blobs, caps)
        assert_same(lay.run_async(d), want)
        lay.assert_canaries()


# ---- 2. counts at the kernel edges ----
@functools.lru_cache(maxsize=None)
def small_frames():
    """257 one-frame entries of 100 .. 700 bytes of text and zipf bytes at levels 1 and 3"""
    rng = np.random.default_rng(5)
    out = []
    for i in range(257):
        n = int(rng.integers(100, 701))
        out.append(wrap(data_of("zipf" if i % 3 == 2 else "text", 200000, 20)[700 * i:700 * i + n], level=1 if i % 2 else 3))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def small_expected():
    blobs = small_frames()
    with sync_context() as d:
        return tuple(DLayout(blobs, [frame_counts(b)[2] for b in blobs], seed=7).run_sync(d))


def test_entry_counts_at_the_kernel_edges(gpu_lib):
    blobs, want = small_frames(), small_expected()
    assert all(isinstance(w, bytes) for w in want)
    with prepared(MAX_ENTRIES, 4096, 1 << 20) as d:
        for n in (1, 63, 64, 65, 255, 256, 257):
            lay = DLayout(blobs[:n], [len(w) for w in want[:n]], seed=n)
            assert_same(lay.run_async(d), want[:n])
            lay.assert_canaries()


@pytest.mark.parametrize("slack", [0, 1])
def test_limits_equal_to_the_actual_counts(gpu_lib, slack):
    blobs, want = small_frames()[:65], small_expected()[:65]
    frames, blocks, content, seqs = total_counts(blobs)
    assert frames == 65 and seqs > 0
    with prepared(65 + slack, max(map(len, blobs)) + slack, content + slack, frames + slack, blocks + slack, seqs + slack) as d:
        lay = DLayout(blobs, [len(w) for w in want])
        assert_same(lay.run_async(d), want)
        lay.assert_canaries()


def test_no_entry_reaches_the_lists(gpu_lib):
    """every entry fails its header: zero frames and zero blocks run through every stage"""
    blobs = [b"\x00" + b[1:] for b in small_frames()[:70]]
    caps = [700] * len(blobs)
    with sync_context() as d:
        want = DLayout(blobs, caps, seed=7).run_sync(d)
    assert want == [PREFIX_UNKNOWN] * len(blobs)
    with prepared(MAX_ENTRIES, 4096, 1 << 20) as d:
        lay = DLayout(blobs, caps)
        assert_same(lay.run_async(d), want)
        lay.assert_canaries(untouched=range(len(blobs)))
        good = DLayout(small_frames()[:5], [700] * 5)           # (and the context is as good as before)
        assert_same(good.run_async(d), small_expected()[:5])


# ---- 3. the rule of the limits ----
def _limit_case(limit):
    """five one-frame entries behind one that fails its header; the limit admits exactly the first three decodable ones"""
    if limit == "sequences":
        data = [data_of("text", 1500, 40 + i) for i in range(5)]
    else:
        data = [data_of("text", 1000, 40 + i) for i in range(5)]
    blobs = [wrap(x) for x in data]
    counts = [frame_counts(b) for b in blobs]
    assert all(c[:3] == (1, 1, len(x)) and c[3] > 1 for c, x in zip(counts, data))
    three = tuple(sum(c[k] for c in counts[:3]) for k in range(4))
    kw = dict(frames=16, blocks=16, seqs=0)
    content = 1 << 16
    if limit == "frames":
        kw["frames"] = 3
    elif limit == "blocks":
        kw["blocks"] = 3
    elif limit == "content":
        content = three[2] + counts[3][2] - 1               # one byte short of the fourth
    else:
        kw["seqs"] = three[3] + counts[3][3] - 1             # one record short of the fourth
    return data, blobs, content, kw


@pytest.mark.parametrize("limit", ["frames", "blocks", "content", "sequences"])
def test_the_limits(gpu_lib, limit):
    data, blobs, content, kw = _limit_case(limit)
    bad = b"\x00" + blobs[0][1:]
    entries = [bad] + blobs
    caps = [2000] * len(entries)
    with prepared(16, 4096, content, **kw) as d:
        lay = DLayout(entries, caps)
        got = lay.run_async(d)
        assert got == [PREFIX_UNKNOWN] + data[:3] + [WS_TOO_SMALL, WS_TOO_SMALL], [g if isinstance(g, int) else len(g) for g in got]
        lay.assert_canaries(untouched=(0, 4, 5))
        # (a call that stays inside the limits, on the same context, is served as before)
        lay3 = DLayout(blobs[:3], caps[:3])
        assert lay3.run_async(d) == data[:3]
    # one more of what was short, and the fourth decodes (the fifth is still beyond)
    if limit in ("content", "sequences"):
        if limit == "content":
            content += 1
        else:
            kw["seqs"] += 1
        with prepared(16, 4096, content, **kw) as d:
            lay = DLayout(entries, caps)
            assert lay.run_async(d) == [PREFIX_UNKNOWN] + data[:4] + [WS_TOO_SMALL]
            lay.assert_canaries(untouched=(0, 5))


# ---- 4. per-entry verdicts, each between good neighbours ----
def test_per_entry_verdicts(gpu_lib):
    good = small_frames()[:9]
    want_good = small_expected()[:9]
    victim_data = data_of("text", 3000, 60)
    victim, checked = wrap(victim_data), wrap(victim_data, checksum=1)
    flipped = bytearray(checked); flipped[len(checked) // 2] ^= 0x40       # (behind a checksum: no flipped byte decodes unnoticed)
    foreign = wrap(data_of("text", 2000, 61), dictionary="trained_16k.dict")
    assert z.get_dict_id_from_frame(foreign) != 0
    # kind -> (blob, capacity)
    cases = {"above-bound": (victim, 3000), "null-src": (victim, 3000), "null-dst": (victim, 3000), "short": (victim, 2999), "flipped": (bytes(flipped), 3000),
             "truncated": (victim[:-3], 3000), "trailing": (victim + b"\x01\x02", 3000), "wrong-dict": (foreign, 2000)}
    entries, caps, kind = [], [], []
    for i, g in enumerate(good):
        entries.append(g); caps.append(len(want_good[i])); kind.append(None)
        if i < len(cases):
            k = list(cases)[i]
            entries.append(cases[k][0]); caps.append(cases[k][1]); kind.append(k)

    def adjust(lay, asynchronous):
        for i, k in enumerate(kind):
            if k == "null-src":
                lay.src_ptr[i] = 0
            elif k == "null-dst":
                lay.dst_ptr[i] = 0
            elif k == "above-bound" and asynchronous:
                lay.sizes[i] = 4097
    with sync_context() as d:
        ref = DLayout(entries, caps, seed=7)
        adjust(ref, False)
        want = ref.run_sync(d)
    assert want[kind.index("null-src")] == SRC_WRONG and want[kind.index("short")] == TOO_SMALL and want[kind.index("wrong-dict")] == WRONG_DICT
    assert want[kind.index("null-dst")] == TOO_SMALL and want[kind.index("truncated")] == SRC_WRONG and want[kind.index("trailing")] == SRC_WRONG
    assert isinstance(want[kind.index("flipped")], int) and want[kind.index("above-bound")] == victim_data
    want[kind.index("above-bound")] = SRC_WRONG          # (the header's first exception)
    with prepared(32, 4096, 1 << 16) as d:
        lay = DLayout(entries, caps)
        adjust(lay, True)
        got = lay.run_async(d)
        assert_same(got, want)
        assert [g for g, k in zip(got, kind) if k is None] == list(want_good)
        lay.assert_canaries(untouched=[i for i, k in enumerate(kind) if k in ("above-bound", "null-src", "null-dst", "short", "truncated", "trailing", "wrong-dict")])


# ---- 5. dictionaries ----
DICT_SETUPS = ["raw-loaded", "formatted-loaded", "ddict", "set-of-two"]


@pytest.mark.parametrize("setup", DICT_SETUPS)
def test_dictionaries(gpu_lib, setup):
    names = {"raw-loaded": ("rawcontent_6000.dict",), "formatted-loaded": ("trained_16k.dict",), "ddict": ("trained_16k.dict",),
             "set-of-two": ("trained_16k.dict", "train_default_json.dict")}[setup]
    data = [data_of("text", 400 + 37 * i, 70 + i) for i in range(24)]
    blobs = [wrap(x, level=1 if i % 2 else 3, dictionary=names[i % len(names)]) for i, x in enumerate(data)]
    if setup == "set-of-two":
        assert len({z.get_dict_id_from_frame(b) for b in blobs}) == 2
    keep = [z.DDict(golden_bytes(n)) for n in names] if setup in ("ddict", "set-of-two") else []

    def configure(d):
        if setup == "set-of-two":
            d.SetParameter(z.ZSTD_d_refMultipleDDicts, 1)
        if keep:
            for dd in keep:
                d.RefDDict(dd)
        else:
            d.LoadDictionary(golden_bytes(names[0]))
    caps = [len(x) for x in data]
    with sync_context(configure) as d:
        want = DLayout(blobs, caps, seed=7).run_sync(d)
    assert want == data
    with prepared(32, 4096, 1 << 16, setup=configure) as d:
        lay = DLayout(blobs, caps)
        assert_same(lay.run_async(d), want)
        lay.assert_canaries()
    for dd in keep:
        dd.Dispose()


def first_block_literals(blob):
    """-> the literals-section type (2: Huffman with a tree, 3: treeless) of a sized frame's first block; None: not a compressed block"""
    fhd = blob[4]
    single, fcs, did = (fhd >> 5) & 1, fhd >> 6, (0, 1, 2, 4)[fhd & 3]
    at = 5 + (0 if single else 1) + did + ((1 if single else 0) if fcs == 0 else 1 << fcs)
    bh = int.from_bytes(blob[at:at + 3], "little")
    return blob[at + 3] & 3 if (bh >> 1) & 3 == 2 else None


@functools.lru_cache(maxsize=None)
def set_mix():
    """-> (blobs, contents): six frames of 2 .. 4 KiB of text that name two dictionaries in turn, each with Huffman literals and
    sequences, and in their middle a forged frame of FIVE blocks without a dictID (the current DDict's) — more blocks than a lane of
    block_link_small takes, so the frame is a wave's of block_link — whose last block repeats its first block's Huffman table"""
    names = ("trained_16k.dict", "train_default_json.dict")
    data = [data_of("text", 2000 + 411 * i, 90 + i) for i in range(6)]
    blobs = [wrap(x, level=3 if i % 2 else 1, dictionary=names[i % 2]) for i, x in enumerate(data)]
    assert len({z.get_dict_id_from_frame(b) for b in blobs}) == 2
    assert all(first_block_literals(b) in (2, 3) and frame_counts(b)[3] > 0 for b in blobs)
    five, content = next(c[2] for c in forge_cases.CASES if c[0] == "huf_treeless_gap_s4")()
    assert frame_counts(five)[1] == 5
    return tuple(blobs[:3] + [five] + blobs[3:]), tuple(data[:3] + [content] + data[3:])


@functools.lru_cache(maxsize=None)
def set_mix_expected():
    blobs, content = set_mix()
    keep = [z.DDict(golden_bytes(n)) for n in ("trained_16k.dict", "train_default_json.dict")]
    with sync_context(lambda d: _ref_set(d, keep)) as d:
        want = DLayout(blobs, [len(x) for x in content], seed=7).run_sync(d)
    for dd in keep:
        dd.Dispose()
    assert want == list(content)
    return tuple(want)


def _ref_set(d, ddicts):
    d.SetParameter(z.ZSTD_d_refMultipleDDicts, 1)
    for dd in ddicts:
        d.RefDDict(dd)


@pytest.mark.parametrize("lit", [1, 2, 3])
def test_a_ddict_set_under_every_literal_decoder(gpu_lib, lit):
    """the set instances that take their counts from the status words, each literal decoder forced: what the synchronous batch gives,
    which is the data (and, for the forged frame, what zstd_forge's own executor regenerates)"""
    blobs, content = set_mix()
    want = set_mix_expected()
    keep = [z.DDict(golden_bytes(n)) for n in ("trained_16k.dict", "train_default_json.dict")]
    with prepared(8, 4096, 1 << 16, setup=lambda d: _ref_set(d, keep), lit=lit) as d:
        lay = DLayout(blobs, [len(x) for x in content])
        assert_same(lay.run_async(d), want)
        lay.assert_canaries()
    for dd in keep:
        dd.Dispose()


# ---- 6. no host round trip ----
def test_no_host_wait_and_no_allocation_across_async_calls(gpu_lib):
    lib = gpu_lib
    blobs, want = small_frames()[:64], small_expected()[:64]
    with prepared(64, 4096, 1 << 16) as d:
        lay = DLayout(blobs, [len(w) for w in want])
        cols = lay.columns()
        waits, allocs = lib.ZSTDMI_debugHostWaitsD(d.dctx), lib.ZSTDMI_debugDeviceAllocsD(d.dctx)
        assert allocs > 0                    # (the prepare sized the work buffers: the counter counts)
        outs = [decompress_batch_async(d, *cols) for _ in range(3)]
        assert lib.ZSTDMI_debugHostWaitsD(d.dctx) == waits
        assert lib.ZSTDMI_debugDeviceAllocsD(d.dctx) == allocs
        assert_same(lay.fetch(outs[-1]), want)
        lay.run_sync(d)
        assert lib.ZSTDMI_debugHostWaitsD(d.dctx) > waits


# ---- 7. in-stream use: compress_batch_async's sizes go straight in ----
@pytest.mark.parametrize("side_stream", [False, True])
def test_in_stream_use(gpu_lib, side_stream):
    import torch
    n, bound, failing = 200, 4096, 17
    pool_host = data_of("text", n * bound, 31)
    with z.Compressor(1) as c:
        cap = c.GetCompressBound(bound)
        c.PrepareBatchAsync(n, bound)
        with prepared(n, cap, n * bound) as d:
            stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                pool = torch.from_numpy(np.frombuffer(pool_host, dtype=np.uint8).copy()).cuda()
                gen = torch.Generator(device="cuda"); gen.manual_seed(5)
                lengths = torch.randint(1, bound + 1, (n,), device="cuda", generator=gen, dtype=torch.int64)
                srcs = pool.data_ptr() + torch.cumsum(lengths, 0) - lengths
                comp = torch.full((n * (cap + 3),), 0xA5, dtype=torch.uint8, device="cuda")
                comp_at = comp.data_ptr() + torch.arange(n, device="cuda", dtype=torch.int64) * (cap + 3)
                comp_caps = torch.full((n,), cap, dtype=torch.int64, device="cuda")
                comp_caps[failing] = 3                       # (no frame fits: the compressor answers dstSize_tooSmall there)
                csizes = compress_batch_async(c, srcs, lengths, comp_at, comp_caps)
                back = torch.full((n * (bound + 3),), 0xA5, dtype=torch.uint8, device="cuda")
                back_at = back.data_ptr() + torch.arange(n, device="cuda", dtype=torch.int64) * (bound + 3)
                out = decompress_batch_async(d, comp_at, csizes, back_at, lengths)      # the host never holds a length
                total = out.clamp(min=0).sum()
            torch.cuda.synchronize()            # the one wait, at the very end
    lengths_h, out_h, back_h, cs_h = lengths.cpu().numpy(), out.cpu().numpy(), back.cpu().numpy(), csizes.cpu().numpy()
    assert cs_h[failing] == TOO_SMALL and out_h[failing] == SRC_WRONG
    assert int(total) == int(lengths_h.sum()) - int(lengths_h[failing])
    at = 0
    for i in range(n):
        mine = back_h[i * (bound + 3):(i + 1) * (bound + 3)]
        if i == failing:
            assert (mine == 0xA5).all()
        else:
            assert out_h[i] == lengths_h[i], i
            assert mine[:lengths_h[i]].tobytes() == pool_host[at:at + lengths_h[i]], i
            assert (mine[lengths_h[i]:] == 0xA5).all(), i
        at += int(lengths_h[i])


# ---- 8. staleness, refusals, lifetime ----
def _raises(code, fn, *args):
    with pytest.raises(ZstdException) as e:
        fn(*args)
    assert e.value.code == code, e.value.code


def test_staleness_and_refusals(gpu_lib):
    lib = gpu_lib
    stage_wrong, unsupported = ZSTD_ErrorCode.ZSTD_error_stage_wrong, ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
    blobs, want = small_frames()[:20], small_expected()[:20]
    lay = DLayout(blobs, [len(w) for w in want])
    limits = (10, 4096, 1 << 16)
    with z.Decompressor() as d, z.DDict(golden_bytes("trained_16k.dict")) as dd:
        _raises(stage_wrong, decompress_batch_async, d, *lay.columns())          # no prepare
        d.PrepareBatchAsync(*limits)
        _raises(stage_wrong, decompress_batch_async, d, *lay.columns())          # n > maxEntries
        assert_same(lay.fetch(decompress_batch_async(d, *lay.columns(10))), want[:10])
        setters = [lambda: d.SetParameter(z.ZSTD_d_windowLogMax, 27), lambda: setattr(d, "batch_unsized", False), lambda: setattr(d, "stream_segment", 0),
                   lambda: lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, 0), lambda: lib.ZSTDMI_DCtx_setExecWaves(d.dctx, 0), lambda: lib.ZSTDMI_DCtx_setOverlap(d.dctx, 0),
                   lambda: lib.ZSTDMI_DCtx_setLongFrames(d.dctx, 0), lambda: lib.ZSTDMI_DCtx_setProfiling(d.dctx, 0), lambda: lib.ZSTDMI_DCtx_setDevice(d.dctx, 0),
                   lambda: d.LoadDictionary(golden_bytes("rawcontent_6000.dict")), lambda: d.RefDDict(dd), lambda: d.RefDDict(None)]
        for s in setters:                                                         # (the value it had: any setter invalidates)
            s()
            _raises(stage_wrong, decompress_batch_async, d, *lay.columns(10))
            d.PrepareBatchAsync(*limits)
            decompress_batch_async(d, *lay.columns(10))
        # the prepare's refusals behind a device
        lib.ZSTDMI_DCtx_setLongFrames(d.dctx, 2)
        _raises(unsupported, d.PrepareBatchAsync, *limits)
        _raises(stage_wrong, decompress_batch_async, d, *lay.columns(10))        # (a refused prepare leaves none)
        lib.ZSTDMI_DCtx_setLongFrames(d.dctx, 0)
        d.RefPrefix(b"some prefix of more than eight bytes")
        _raises(unsupported, d.PrepareBatchAsync, *limits)
        _raises(unsupported, d.PrepareBatchAsync, *limits)                       # (the prefix stays pending)
        d.LoadDictionary(None)
        assert lib.ZSTDMI_DCtx_setDevices(d.dctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        _raises(unsupported, d.PrepareBatchAsync, *limits)
        assert lib.ZSTDMI_DCtx_setDevices(d.dctx, None, 0) == 0
        _raises(ZSTD_ErrorCode.ZSTD_error_memory_allocation, d.PrepareBatchAsync, 10, 4096, 1 << 45)      # (32 TiB of literal scratch)
        _raises(stage_wrong, decompress_batch_async, d, *lay.columns(10))
        d.PrepareBatchAsync(20, 4096, 1 << 16)
        assert_same(lay.fetch(decompress_batch_async(d, *lay.columns())), want)
        lay.assert_canaries()


def test_dispose_straight_after_an_async_call(gpu_lib):
    blobs, want = small_frames()[:200], small_expected()[:200]
    lay = DLayout(blobs, [len(w) for w in want])
    cols = lay.columns()
    d = prepared(200, 4096, 1 << 18)
    out = decompress_batch_async(d, *cols)
    d.Dispose()                              # (nothing synchronised first: the context waits for its own work)
    assert_same(lay.fetch(out), want)
    lay.assert_canaries()


def test_back_to_back_then_a_larger_synchronous_batch(gpu_lib):
    blobs, want = small_frames(), small_expected()
    big_blobs, big_caps, _ = parity_mix()
    with prepared(100, 4096, 1 << 17) as d:
        d.batch_unsized = True
        d.PrepareBatchAsync(100, 4096, 1 << 17)
        a, b = DLayout(blobs[:100], [len(w) for w in want[:100]], seed=3), DLayout(blobs[100:200], [len(w) for w in want[100:200]], seed=4)
        out_a = decompress_batch_async(d, *a.columns())
        out_b = decompress_batch_async(d, *b.columns())       # (no synchronisation in between)
        big = DLayout(big_blobs, big_caps, seed=5)
        got_big = big.run_sync(d, wait=False)                 # more content than the prepare sized: the buffers regrow behind the enqueued work
        assert_same(a.fetch(out_a), want[:100])
        assert_same(b.fetch(out_b), want[100:200])
        a.assert_canaries(); b.assert_canaries()
        assert_same(got_big, parity_expected())
