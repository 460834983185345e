"""GPU tests of ZSTDMI_compressBatchCDicts (include/zstd_mi355x.h "a CDict per entry"): one batch whose entries lie behind different
digested dictionaries.  The yardstick is never the new call, nor the batch code: per entry it is another context with the same
parameters and switches doing RefCDict(cdicts[i]) + the single call (Wrap) on that entry.  ZSTDMI_debugLastBatchPasses and ZSTDMI_debugLastBatchSetChunks show
that entries behind different dictionaries shared a pass — the feature — and not one round per dictionary inside the call."""
import ctypes
import functools
import os

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error
from test_gpu_ddict_set import dic, with_id
from test_gpu_dict_index import rand_dict
from test_gpu_dict_index_chain import dense_head, text

pytestmark = pytest.mark.gpu

ZSTD_c_windowLog, ZSTD_c_checksumFlag, ZSTD_c_dictIDFlag = 101, 201, 202
UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
TOO_SMALL = ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall
BIG = ("train_default_json.dict", "train_default_text.dict", "train_default_zipf.dict")      # 112 640 bytes each
K8 = ("train_d6_f20_a1_k537_8k.dict", "train_d8_f16_a1_k1024_8k.dict")
SIZES = (300, 777, 1500, 4096, 2049, 3333, 512, 4000)       # (the size list of test_gpu_ddict_set.records())
# the dictionary switches: (dict_index, dict_index_strategy or None, dict_index_chain)
INDEX = [pytest.param((False, None, False), id="staged"), pytest.param((True, None, False), id="index"),
         pytest.param((True, 2, False), id="index-strategy2"), pytest.param((True, None, True), id="index-chain")]


@functools.lru_cache(maxsize=None)
def pool(kind):
    return datagen.gen(kind, 120000, 500 if kind == "text" else 501)


def records(n=40):
    """n records of 300 B to 4 KiB cut from one text and one zipf pool; record i is zipf when i % 3 == 2"""
    return [pool("zipf" if i % 3 == 2 else "text")[2500 * i:2500 * i + SIZES[i % len(SIZES)]] for i in range(n)]


def dict_bytes(name):
    """a golden dictionary, "name#id" = the same under another dictID, "D" / "D2" = 112 640 random bytes (raw content)"""
    if name == "D":
        return rand_dict()
    if name == "D2":
        return datagen.gen("rand", 112640, 77)
    if "#" in name:
        base, dict_id = name.split("#")
        return with_id(dic(base), int(dict_id))
    return dic(name)


@pytest.fixture(scope="module")
def cdicts(gpu_lib):
    """CDicts made once per (name, level): get(name, level); None stays None"""
    made = {}

    def get(name, level):
        if name is None:
            return None
        if (name, level) not in made:
            made[(name, level)] = z.CDict(dict_bytes(name), level)
        return made[(name, level)]
    yield get
    for d in made.values():
        d.Dispose()


def context(level=3, entropy=False, index=(False, None, False), params=()):
    c = z.Compressor(level)
    for p, v in params:
        c.SetParameter(p, v)
    c.dict_entropy = entropy
    c.dict_index = index[0]
    if index[1] is not None:
        c.dict_index_strategy = index[1]
    c.dict_index_chain = index[2]
    return c


def yardstick(items, dicts, fresh=False, **kw):
    """per entry: RefCDict(its CDict) + the single call, Wrap, on a context made like the one under test.  fresh: a new context for
    every entry; else one context whose reference changes from entry to entry."""
    out, y = [], None
    for data, d in zip(items, dicts):
        if y is None:
            y = context(**kw)
        y.RefCDict(d)
        out.append(y.Wrap(data))
        y.RefCDict(None)
        if fresh:
            y.Dispose()
            y = None
    if y is not None:
        y.Dispose()
    return out


def raw_call(lib, c, items, dicts, caps=None, guard=16):
    """the C call with destinations side by side, `guard` bytes of 0xA5 behind each capacity -> (return value, dstSizes, outputs)"""
    import torch
    n, sizes = len(items), [len(x) for x in items]
    flat = torch.from_numpy(np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8).copy()).cuda()
    srcs, at = [], 0
    for s in sizes:
        srcs.append(flat.data_ptr() + at if s else None)
        at += s
    caps = list(caps) if caps is not None else [lib.ZSTD_compressBound(s) for s in sizes]
    starts, at = [], 0
    for cap in caps:
        starts.append(at)
        at += cap + guard
    out = torch.full((max(at, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    got = (ctypes.c_size_t * n)()
    handles = (ctypes.c_void_p * n)(*[d.handle if d is not None else None for d in dicts])
    torch.cuda.synchronize()
    r = lib.ZSTDMI_compressBatchCDicts(c.cctx, (ctypes.c_void_p * n)(*srcs), (ctypes.c_size_t * n)(*sizes), n,
                                       (ctypes.c_void_p * n)(*[out.data_ptr() + s for s in starts]), (ctypes.c_size_t * n)(*caps), got, handles)
    host = out.cpu().numpy().tobytes()
    for i in range(n):
        assert host[starts[i] + caps[i]:starts[i] + caps[i] + guard] == b"\xA5" * guard, f"entry {i}: written beyond its capacity"
    return r, list(got), [None if is_error(got[i]) else host[starts[i]:starts[i] + got[i]] for i in range(n)]


def decode_each(frames, items, names):
    """every frame decodes to its record under a decoder that holds its dictionary (None: none)"""
    decs = {}
    for f, data, name in zip(frames, items, names):
        if name not in decs:
            decs[name] = z.Decompressor()
            if name is not None:
                decs[name].LoadDictionary(dict_bytes(name))
        assert decs[name].Unwrap(f) == data, name
    for d in decs.values():
        d.Dispose()


# ---------------------------------------------------------------- 1. one pass, many dictionaries ----------------------------------------------------------------
@pytest.mark.parametrize("index", INDEX)
@pytest.mark.parametrize("entropy", [False, True], ids=["plain", "entropy"])
@pytest.mark.parametrize("level", [1, 3, 5])
def test_one_pass_many_dictionaries(gpu_lib, cdicts, level, entropy, index):
    """40 records, neighbours behind the three 112 640-byte golden dictionaries and the same three under other dictIDs: six CDicts, one
    tail length in tiles, one resolved parameter set -> ONE pass, every chunk in the set instances.  One case per finder (CDict level
    1, 3, 5; the context's own level is another) and per combination of the four dictionary switches."""
    names = list(BIG) + [f"{b}#{7000 + k}" for k, b in enumerate(BIG)]
    items = records()
    which = [names[i % 6] for i in range(len(items))]
    dicts = [cdicts(nm, level) for nm in which]
    want = yardstick(items, dicts, fresh=True, level=2, entropy=entropy, index=index)
    with context(level=2, entropy=entropy, index=index) as c:
        got = z.compress_batch(c, items, cdicts=dicts)
        alone, passes, chunks = gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx), gpu_lib.ZSTDMI_debugLastBatchPasses(c.cctx), gpu_lib.ZSTDMI_debugLastBatchSetChunks(c.cctx)
    print(f"level {level}: alone {alone}, passes {passes}, set chunks {chunks}, {sum(map(len, got))} B")
    assert [len(x) for x in got] == [len(x) for x in want]
    assert got == want
    assert alone == 0 and passes == 1 and chunks == len(items)
    with z.Decompressor() as d:
        d.SetParameter(z.ZSTD_d_refMultipleDDicts, 1)
        dds = [z.DDict(dict_bytes(nm)) for nm in names]
        for dd in dds:
            d.RefDDict(dd)
        assert z.decompress_batch(d, got, [len(x) for x in items]) == items
        d.RefDDict(None)
        for dd in dds:
            dd.Dispose()
    for f, nm in zip(got, which):
        assert z.get_dict_id_from_frame(f) == z.get_dict_id_from_dict(dict_bytes(nm))


# ---------------------------------------------------------------- 2. classes ----------------------------------------------------------------
# (name, CDict level); the context's own level is 3, which the entries without a CDict run at
MIXED = [(BIG[0], 1), (BIG[1], 1), (BIG[2], 3), (BIG[0], 3), ("trained_16k.dict", 1), (K8[0], 3), (K8[1], 3), ("rawcontent_6000.dict", 3), (None, 3)]


@pytest.mark.parametrize("index,passes,lone", [pytest.param((False, None, False), 5, 2, id="staged"), pytest.param((True, 2, False), 3, 1, id="index-strategy2")])
def test_classes(gpu_lib, cdicts, index, passes, lone):
    """Dictionaries of every kind and CDicts of two levels in one call.  Passes, by the rule of the header: entries share one when
    their chunk size (64 KiB minus the staged tail in whole 4 KiB tiles), indexed-ness and resolved parameters are equal.
    Staged: {json, text at level 1} and {zipf, json at level 3} stage 60 KiB; trained_16k at level 1 stages its content of under
    16 KiB, four tiles; the two 8 KiB dictionaries and the 6000 raw bytes stage two tiles each and share ONE pass at level 3; the
    entries without a dictionary are a pass of their own: 5.  Indexed (index on, strategy 2: levels 1 and 3 both look candidates up in
    the index, nothing is staged, every chunk is 64 KiB): all dictionaries of a level share a pass, plus the entries without: 3.
    lone: the kinds of MIXED whose pass holds one CDict (or none) and so runs the single-dictionary kernels: the entries without a
    dictionary, and, staged, trained_16k."""
    items = records(45)
    which = [MIXED[i % len(MIXED)] for i in range(len(items))]
    dicts = [cdicts(nm, lv) for nm, lv in which]
    for entropy in (False, True):
        want = yardstick(items, dicts, level=3, entropy=entropy, index=index)
        with context(level=3, entropy=entropy, index=index) as c:
            got = z.compress_batch(c, items, cdicts=dicts)
            n_passes, alone = gpu_lib.ZSTDMI_debugLastBatchPasses(c.cctx), gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx)
            chunks = gpu_lib.ZSTDMI_debugLastBatchSetChunks(c.cctx)
        print(f"entropy {entropy}: passes {n_passes}, alone {alone}, set chunks {chunks}")
        assert got == want
        assert alone == 0 and n_passes == passes
        assert chunks == len(items) - lone * (len(items) // len(MIXED))
        decode_each(got, items, [nm for nm, _ in which])


# ---------------------------------------------------------------- 3. several chunks per entry ----------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 3, 5])
def test_several_chunks_per_entry(gpu_lib, cdicts, level):
    """70 000 B and 200 000 B of text behind two different 112 640-byte dictionaries: 32 KiB chunks behind a 32 KiB tail, 3 + 7 of them"""
    items = [text(70000, 21), text(200000, 22)]
    names = [BIG[0], BIG[1]]
    dicts = [cdicts(nm, level) for nm in names]
    want = yardstick(items, dicts, level=3)
    with context(level=3) as c:
        got = z.compress_batch(c, items, cdicts=dicts)
        passes, chunks = gpu_lib.ZSTDMI_debugLastBatchPasses(c.cctx), gpu_lib.ZSTDMI_debugLastBatchSetChunks(c.cctx)
    assert got == want
    assert (passes, chunks) == (1, 3 + 7)
    decode_each(got, items, names)


@pytest.mark.parametrize("index", [pytest.param((True, None, True), id="index-chain"), pytest.param((False, None, False), id="staged")])
def test_dense_records_reach_the_region_kernel(gpu_lib, cdicts, index):
    """The dense record of README "Levels 5 and up" (15 592 bytes: a dense head, then slices of D between text) behind two raw
    dictionaries at level 5: its chunk leaves the tile loop for lz_region_kernel, whose set instance (the indexed one with index +
    chain on, the staged one without) reads the chunk's dictionary through the work list."""
    D = rand_dict()
    rec = dense_head() + D[1000:1700] + text(500, 11) + D[45000:45700] + text(500, 12) + D[20000:24000] + text(1000, 13)
    assert len(rec) == 15592
    items = [rec, rec[:9000] + text(6000, 14), rec, text(12000, 15)]
    names = ["D", "D2", "D2", "D"]
    dicts = [cdicts(nm, 5) for nm in names]
    want = yardstick(items, dicts, level=1, index=index)
    with context(level=1, index=index) as c:
        got = z.compress_batch(c, items, cdicts=dicts)
        region = gpu_lib.ZSTDMI_debugLastRegionChunks(c.cctx)
        passes, chunks = gpu_lib.ZSTDMI_debugLastBatchPasses(c.cctx), gpu_lib.ZSTDMI_debugLastBatchSetChunks(c.cctx)
    print(f"region chunks {region}; sizes {[len(x) for x in got]}")
    assert got == want
    assert region > 0
    assert (passes, chunks) == (1, 4)
    if index[0]:
        assert len(got[0]) + 4000 <= len(got[2])        # (the slices of D are found behind D, not behind D2)
    decode_each(got, items, names)


# ---------------------------------------------------------------- 4. edges ----------------------------------------------------------------
def test_edge_sizes(gpu_lib, cdicts):
    """empty, 1 byte, exactly one chunk (4096 B behind a 60 KiB tail) and a chunk plus one byte (then 32 KiB chunks: another class)"""
    items = [b"", b"x", pool("text")[:4096], pool("text")[:4097], pool("text")[100:400], b"", pool("zipf")[:4096]]
    names = [BIG[0], BIG[1], BIG[0], BIG[1], BIG[2], None, BIG[1]]
    dicts = [cdicts(nm, 3) for nm in names]
    want = yardstick(items, dicts, level=3)
    with context(level=3) as c:
        r, sizes, got = raw_call(gpu_lib, c, items, dicts)
        assert r == 0 and got == want
        assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 2          # (the empty entries)
        assert gpu_lib.ZSTDMI_debugLastBatchPasses(c.cctx) == 2 and gpu_lib.ZSTDMI_debugLastBatchSetChunks(c.cctx) == 4
    decode_each(got, items, names)


def test_one_entry_fails_alone(gpu_lib, cdicts):
    items = records(8)
    names = [BIG[i % 3] for i in range(8)]
    dicts = [cdicts(nm, 3) for nm in names]
    want = yardstick(items, dicts, level=3, entropy=True)
    caps = [gpu_lib.ZSTD_compressBound(len(x)) for x in items]
    caps[3] = len(want[3]) - 1
    with context(level=3, entropy=True) as c:
        r, sizes, got = raw_call(gpu_lib, c, items, dicts, caps)
    assert r == 0
    assert is_error(sizes[3]) and get_error_code(sizes[3]) == TOO_SMALL
    assert [g for i, g in enumerate(got) if i != 3] == [w for i, w in enumerate(want) if i != 3]


@pytest.mark.parametrize("params", [((ZSTD_c_dictIDFlag, 0),), ((ZSTD_c_checksumFlag, 1),)], ids=["no-dictid", "checksum"])
def test_frame_parameters(gpu_lib, cdicts, params):
    items = records(12)
    names = [(BIG + ("trained_16k.dict",))[i % 4] for i in range(12)]
    dicts = [cdicts(nm, 3) for nm in names]
    want = yardstick(items, dicts, level=3, params=params)
    with context(level=3, params=params) as c:
        got = z.compress_batch(c, items, cdicts=dicts)
    assert got == want
    if params[0][0] == ZSTD_c_dictIDFlag:
        assert all(z.get_dict_id_from_frame(f) == 0 for f in got)
    decode_each(got, items, names)


def test_a_cdict_under_8_bytes_is_no_dictionary(gpu_lib, cdicts):
    items = records(6)
    with z.CDict(b"abc", 3) as tiny:
        dicts = [tiny, cdicts(BIG[0], 3), None, tiny, cdicts(BIG[1], 3), tiny]
        want = yardstick(items, dicts, level=3)
        with context(level=3) as c:
            got = z.compress_batch(c, items, cdicts=dicts)
    assert got == want
    assert got[0] == yardstick(items[:1], [None], level=3)[0]
    decode_each(got, items, [None, BIG[0], None, None, BIG[1], None])


@pytest.mark.parametrize("order", ["none-first", "staged-first"])
@pytest.mark.parametrize("wlog", [10, 12, 15])
def test_small_windows_keep_plain_and_staged_entries_apart(gpu_lib, cdicts, wlog, order):
    """ZSTD_c_windowLog 10 .. 15: an entry of at most one window is one chunk of 1 << windowLog bytes with or without a dictionary, so
    entries without one (NULL, a CDict under 8 bytes), which run the plain finder, and entries behind staged tails are equal in chunk
    size, blocks per frame and parameters.  They must not share a pass, whichever kind comes first: each is written as the single
    call writes it.  (Entries above one window go alone.)"""
    items = records(24)
    with z.CDict(b"abc", 3) as tiny:
        kinds = [(None, None), (BIG[0], cdicts(BIG[0], 3)), (None, tiny), (K8[0], cdicts(K8[0], 3)), (BIG[1], cdicts(BIG[1], 3)), ("rawcontent_6000.dict", cdicts("rawcontent_6000.dict", 3))]
        if order == "staged-first":
            kinds = kinds[1:] + kinds[:1]
        names = [kinds[i % len(kinds)][0] for i in range(len(items))]
        dicts = [kinds[i % len(kinds)][1] for i in range(len(items))]
        params = ((ZSTD_c_windowLog, wlog),)
        want = yardstick(items, dicts, fresh=True, level=3, entropy=True, params=params)
        with context(level=3, entropy=True, params=params) as c:
            r, sizes, got = raw_call(gpu_lib, c, items, dicts)
            print(f"windowLog {wlog}: passes {gpu_lib.ZSTDMI_debugLastBatchPasses(c.cctx)}, alone {gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx)}, "
                  f"set chunks {gpu_lib.ZSTDMI_debugLastBatchSetChunks(c.cctx)}")
            assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == sum(len(x) > (1 << wlog) for x in items)
    assert r == 0 and got == want
    decode_each(got, items, names)


def test_one_cdict_for_all_is_the_plain_batch(gpu_lib, cdicts):
    """all entries behind one CDict: ZSTD_CCtx_refCDict + ZSTDMI_compressBatch, no set instance; and the context's own loaded
    dictionary and reference are what they were (a following plain Wrap writes what it wrote before)"""
    items = records(10)
    cd = cdicts(BIG[1], 3)
    with context(level=1) as c:
        c.LoadDictionary(dic("trained_16k.dict"))
        before = c.Wrap(items[0])
        got = z.compress_batch(c, items, cdicts=[cd] * len(items))
        assert gpu_lib.ZSTDMI_debugLastBatchSetChunks(c.cctx) == 0 and gpu_lib.ZSTDMI_debugLastBatchPasses(c.cctx) >= 1
        assert c.Wrap(items[0]) == before
        mixed = z.compress_batch(c, items, cdicts=[cd if i % 2 else cdicts(BIG[0], 3) for i in range(len(items))])
        assert gpu_lib.ZSTDMI_debugLastBatchSetChunks(c.cctx) == len(items)
        assert c.Wrap(items[0]) == before
        none = z.compress_batch(c, items, cdicts=[None] * len(items))
        assert c.Wrap(items[0]) == before
        other = cdicts(BIG[2], 3)
        c.RefCDict(other)
        held = c.Wrap(items[0])
        assert z.compress_batch(c, items, cdicts=[cd if i % 2 else None for i in range(len(items))])[1] == got[1]
        assert c.Wrap(items[0]) == held
        c.RefCDict(None)
    with context(level=1) as y:
        y.RefCDict(cd)
        assert z.compress_batch(y, items) == got
        y.RefCDict(None)
        assert z.compress_batch(y, items) == none
    assert mixed[1::2] == got[1::2]


def test_what_the_call_refuses(gpu_lib, cdicts):
    items = records(4)
    dicts = [cdicts(BIG[i % 2], 3) for i in range(4)]
    with context(level=3) as c:
        c.seek_table = True
        r, _, _ = raw_call(gpu_lib, c, items, dicts)
        assert is_error(r) and get_error_code(r) == UNSUPPORTED
        c.seek_table = False
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        r, _, _ = raw_call(gpu_lib, c, items, dicts)
        assert is_error(r) and get_error_code(r) == UNSUPPORTED
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, None, 0) == 0
        prefix = pool("text")[50000:58000]
        c.RefPrefix(prefix)
        r, _, _ = raw_call(gpu_lib, c, items, dicts)
        assert is_error(r) and get_error_code(r) == UNSUPPORTED
        with_prefix = c.Wrap(items[3])              # (still pending: this call consumes it)
        without = c.Wrap(items[3])
        assert with_prefix != without
        with z.Decompressor() as d:
            d.RefPrefix(prefix)
            assert d.Unwrap(with_prefix) == items[3]
        r, _, got = raw_call(gpu_lib, c, items, dicts)
        assert r == 0 and got == yardstick(items, dicts, level=3)


# ---------------------------------------------------------------- 5. unchanged paths ----------------------------------------------------------------
@pytest.mark.parametrize("index", INDEX)
def test_the_plain_batch_is_unchanged(gpu_lib, cdicts, index):
    """a context that never calls the new entry point: compress_batch behind one CDict writes what the single calls write, in one pass
    per class of resolved parameters (they follow the entry's size up to the next power of two), and no set instance runs"""
    items = records(16) + [text(70000, 31)]
    classes = len({(len(x) - 1).bit_length() for x in items})
    for level in (1, 3, 5):
        with context(level=2, entropy=True, index=index) as c:
            c.RefCDict(cdicts(BIG[0], level))
            got = z.compress_batch(c, items)
            assert gpu_lib.ZSTDMI_debugLastBatchSetChunks(c.cctx) == 0 and gpu_lib.ZSTDMI_debugLastBatchPasses(c.cctx) == classes
            assert got == [c.Wrap(x) for x in items]
            c.RefCDict(None)
