"""GPU tests of ZSTDMI_CCtx_setDictIndex: with the switch on, a dictionary is indexed once when it is uploaded and the fast finder
matches against ALL of it (its last 188 KiB) without staging a byte of it per chunk; a source of up to 64 KiB is one block in one
frame.  Every frame decodes under the oracle's dictionary decoder and under the GPU decoder, every entry point writes the same bytes,
and nothing outside "a dictionary at the fast strategy" moves by a byte."""
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import get_error_code, is_error

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_train as mgt  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZSTD_c_windowLog, ZSTD_c_strategy, ZSTD_c_enableLongDistanceMatching = 101, 107, 160
ZSTD_c_checksumFlag, ZSTD_c_dictIDFlag = 201, 202
K_FAR_MAX = 188 << 10


def golden_bytes(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


@functools.lru_cache(maxsize=None)
def rand_dict():
    return datagen.gen("rand", 112640, 4242)


def make_compressor(level, dic=None, index=True, params=(), entropy=False, setter_first=False):
    c = z.Compressor(level)
    for p, v in params:
        c.SetParameter(p, v)
    if setter_first:
        c.dict_index = index
    if dic is not None:
        c.LoadDictionary(dic)
    if not setter_first:
        c.dict_index = index
    if entropy:
        c.dict_entropy = True
    return c


def roundtrip(comps, recs, dic, oracle):
    for i, (cz, r) in enumerate(zip(comps, recs)):
        assert oracle.decompress(cz, len(r), dic) == r, (i, len(r))
    with z.Decompressor() as d:
        d.LoadDictionary(dic)
        back = z.decompress_batch(d, comps, [len(r) for r in recs])
        for i, (b, r) in enumerate(zip(back, recs)):
            assert bytes(b) == r, (i, len(r))


def frames_of(stream, oracle):
    out, pos = [], 0
    while pos < len(stream):
        n = oracle.lib().zso_findFrameCompressedSize(stream[pos:], len(stream) - pos)
        assert not oracle.is_error(n) and n > 0, (pos, len(stream))
        out.append(stream[pos:pos + n]); pos += n
    return out


# ---------------------------------------------------------------- 1. the whole dictionary is seen ----------------------------------------------------------------
VIS = [(a, n) for a in (0, 40000, 110592) for n in (300, 2048)]


def test_records_cut_from_anywhere_in_the_dictionary_are_found(gpu_lib, oracle):
    """D is 112 640 random bytes, so the only redundancy of D[a:a+n] is the dictionary itself.  On: at most n // 4 bytes (the oracle
    writes 18-19; a quarter separates "found" from "stored" whatever the tile parse cuts).  Off, in front of the staged 60 KiB tail:
    at least n bytes — the gap this switch closes, and the assertion that fails without it."""
    D = rand_dict()
    recs = [D[a:a + n] for a, n in VIS]
    with make_compressor(1, D, True) as c:
        on = [c.Wrap(r) for r in recs]
        assert gpu_lib.ZSTDMI_debugDictIndexed(c.cctx) == 112640
    with make_compressor(1, D, False) as c:
        off = [c.Wrap(r) for r in recs]
        assert gpu_lib.ZSTDMI_debugDictIndexed(c.cctx) == 0
    ref = [len(oracle.compress_dict(r, D, 1)) for r in recs]
    print("visibility (a, n) -> on / off / oracle:", [(an, len(x), len(y), o) for an, x, y, o in zip(VIS, on, off, ref)])
    roundtrip(on, recs, D, oracle)
    for (a, n), x, y in zip(VIS, on, off):
        assert len(x) <= n // 4, (a, n, len(x))
        if a in (0, 40000):
            assert len(y) >= n, (a, n, len(y))


def test_mixed_record_takes_three_far_matches(gpu_lib, oracle):
    D, f = rand_dict(), datagen.gen("rand", 300, 9)
    rec = D[1000:1700] + f[:100] + D[45000:45700] + f[100:200] + D[100000:100700]
    with make_compressor(1, D, True) as c:
        comp = c.Wrap(rec)
    ref = len(oracle.compress_dict(rec, D, 1))
    print(f"mixed record: GPU {len(comp)} B, oracle {ref} B")
    roundtrip([comp], [rec], D, oracle)
    assert len(comp) <= 200 + 2300 // 4, len(comp)


def test_index_covers_the_last_188_kib_of_a_long_dictionary(gpu_lib, oracle):
    big = datagen.gen("text", 262144, 31)
    recs = [datagen.gen("text", n, 32 + n) for n in (300, 5000, 70000)] + [big[:3000], big[262144 - K_FAR_MAX:262144 - K_FAR_MAX + 3000], big[-3000:]]
    with make_compressor(1, big, True) as c:
        comps = [c.Wrap(r) for r in recs]
        assert gpu_lib.ZSTDMI_debugDictIndexed(c.cctx) == K_FAR_MAX
    roundtrip(comps, recs, big, oracle)
    assert len(comps[4]) <= 3000 // 4 and len(comps[5]) <= 3000 // 4, (len(comps[4]), len(comps[5]))     # (the first and last indexed bytes)


# ---------------------------------------------------------------- 2. round trips ----------------------------------------------------------------
SIZES = [1, 7, 8, 300, 4095, 4096, 4097, 65535, 65536, 65537, 200000]
KINDS = ["text", "zipf", "rand", "zeros"]


@functools.lru_cache(maxsize=None)
def size_records():
    return tuple(datagen.gen(k, n, 600 + i) for i, k in enumerate(KINDS) for n in SIZES)


def dictionary(name):
    return rand_dict() if name == "D" else golden_bytes(name)


@pytest.mark.parametrize("name", ["rawcontent_6000.dict", "trained_16k.dict", "train_default_json.dict", "D"])
def test_round_trips(gpu_lib, oracle, name):
    dic, recs = dictionary(name), size_records()
    variants = [(-5, (), False), (1, (), False), (2, (), False), (1, ((ZSTD_c_checksumFlag, 1),), False),
                (1, ((ZSTD_c_dictIDFlag, 0),), False), (1, (), True)]
    sizes = {}
    for level, params, entropy in variants:
        with make_compressor(level, dic, True, params, entropy) as c:
            comps = z.compress_batch(c, recs)
            assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
        roundtrip(comps, recs, dic, oracle)
        for r, cz in zip(recs, comps):      # up to 64 KiB: one frame; above: independent 64 KiB frames
            assert len(frames_of(cz, oracle)) == (len(r) + 65535) // 65536, (level, len(r))
        sizes[(level, params, entropy)] = sum(map(len, comps))
    print(f"{name}: totals {sizes}")


# ---------------------------------------------------------------- 3. the dictionary's end ----------------------------------------------------------------
def test_dictionary_end_seam(gpu_lib, oracle):
    D = rand_dict()
    recs = [D[-64:] + datagen.gen("text", 500, 1), D[-200:] * 3, D[3:600], D[:16] + datagen.gen("rand", 40, 5) + D[5:400],
            D[-8:], D[-7:], D[-300:], datagen.gen("rand", 20, 6) + D[-40:] + D[:40]]
    for level in (1, -5):
        with make_compressor(level, D, True) as c:
            comps = z.compress_batch(c, recs)
            assert [c.Wrap(r) for r in recs] == comps
        roundtrip(comps, recs, D, oracle)
    assert len(comps) == len(recs)


# ---------------------------------------------------------------- 4. equal bytes from every entry point ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def door_records():
    r = np.random.default_rng(23)
    D = rand_dict()
    sizes = [1, 7, 8, 65535, 65536, 65537, 150000] + [int(np.exp(x)) for x in r.uniform(0, np.log(65536), 41)]
    pool = {"text": datagen.gen("text", 1 << 19, 901), "zipf": datagen.gen("zipf", 1 << 19, 902), "dict": D + D}
    kinds = ["text", "dict", "text", "zipf"]
    return tuple(pool[kinds[i % 4]][(at := int(r.integers(0, 200000 - n if n < 200000 else 1))):at + n] for i, n in enumerate(sizes))


def device_singles(lib, cctx, entries):
    import torch
    out = []
    room = torch.empty(lib.ZSTD_compressBound(max(len(e) for e in entries)) + 64, dtype=torch.uint8, device="cuda")
    for e in entries:
        src = torch.from_numpy(np.frombuffer(e, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        r = lib.ZSTDMI_compressDevice(cctx, room.data_ptr(), lib.ZSTD_compressBound(len(e)), src.data_ptr(), len(e))
        assert not is_error(r), (len(e), get_error_code(r))
        out.append(room[:r].cpu().numpy().tobytes())
    return out


@pytest.mark.parametrize("name", ["D", "trained_16k.dict"])
def test_every_entry_point_writes_the_same_bytes(gpu_lib, oracle, name):
    import torch
    dic, recs = dictionary(name), door_records()
    with make_compressor(1, dic, True) as c:
        singles = [c.Wrap(r) for r in recs]
        assert [c.Wrap(r) for r in recs] == singles                        # the same call twice
        assert device_singles(gpu_lib, c.cctx, recs) == singles
        batch = z.compress_batch(c, recs)
        assert batch == singles
        small = [r for r in recs if len(r) <= 65536]
        z.compress_batch(c, small)
        assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
        sizes = (ctypes.c_size_t * len(recs))(*[len(r) for r in recs])
        out = (ctypes.c_size_t * len(recs))()
        assert gpu_lib.ZSTDMI_debugCompressSamples(c.cctx, b"".join(recs), sizes, len(recs), out) == 0
        assert list(out) == [len(s) for s in singles]
    roundtrip(singles, recs, dic, oracle)
    with make_compressor(1, dic, True, setter_first=True) as c2:          # a fresh context, the setter before the dictionary
        assert [c2.Wrap(r) for r in recs] == singles
    with make_compressor(1, dic, True) as c3:                              # the streaming adapter, one flush per record
        sink = io.BytesIO()
        st = z.CompressionStream(sink, compressor=c3)
        for r, s in zip(recs, singles):
            at = sink.tell()
            st.Write(r); st.Flush()
            assert sink.getvalue()[at:] == s, len(r)
        st.Dispose()
    # two workers: device 0 and 1 when there are two, else device 0 listed twice (each worker has its own copy of the index)
    with make_compressor(1, dic, True) as c4:
        arr = (ctypes.c_int * 2)(0, 1 if torch.cuda.device_count() >= 2 else 0)
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c4.cctx, arr, 2) == 0
        for i in list(range(0, len(recs), 4)) + [4, 5, 6]:
            assert c4.Wrap(recs[i]) == singles[i], (i, len(recs[i]))


# ---------------------------------------------------------------- 5. nothing else moves ----------------------------------------------------------------
def both(level, dic, params=()):
    return make_compressor(level, dic, False, params), make_compressor(level, dic, True, params)


def test_switch_changes_nothing_where_promised(gpu_lib, oracle):
    recs = [datagen.gen("text", n, 70 + n) for n in (40, 300, 5000, 30000, 70000, 300000)]
    raw_dict, fmt_dict, D = golden_bytes("rawcontent_6000.dict"), golden_bytes("trained_16k.dict"), rand_dict()

    def same(off, on, items=recs, tag=None):
        with off, on:
            for r in items:
                assert on.Wrap(r) == off.Wrap(r), (tag, len(r))

    # no dictionary; a dictionary below 8 bytes
    same(*both(1, None), tag="none")
    same(*both(1, b"abcdefg"), tag="7 bytes")
    for dic in (raw_dict, fmt_dict, D):
        # levels whose finder is the dual-hash or the chain finder, by level and by strategy
        same(*both(3, dic), tag="level 3")
        same(*both(5, dic), tag="level 5")
        same(*both(1, dic, ((ZSTD_c_strategy, 2),)), tag="strategy 2")
        # windows below the block
        for wl in (10, 15):
            same(*both(1, dic, ((ZSTD_c_windowLog, wl),)), tag=f"windowLog {wl}")
        # ZSTD_compressCCtx uses no dictionary, loaded or not
        with make_compressor(1, dic, False) as off, make_compressor(1, dic, True) as on:
            for r in recs:
                cap = gpu_lib.ZSTD_compressBound(len(r))
                a, b = ctypes.create_string_buffer(cap), ctypes.create_string_buffer(cap)
                na = gpu_lib.ZSTD_compressCCtx(off.cctx, a, cap, r, len(r), 1)
                nb = gpu_lib.ZSTD_compressCCtx(on.cctx, b, cap, r, len(r), 1)
                assert not is_error(na) and na == nb and a.raw[:na] == b.raw[:nb], len(r)
        # on and off again = a context that never heard of the switch
        with make_compressor(1, dic, False) as fresh, make_compressor(1, dic, True) as back:
            changed = [back.Wrap(r) for r in recs]
            back.dict_index = False
            for r in recs:
                assert back.Wrap(r) == fresh.Wrap(r), len(r)
            assert any(ch != fresh.Wrap(r) for r, ch in zip(recs, changed))      # (the switch did something while it was on)
        # the refusals stay: long-distance matching above one block, one frame per call above one block
        for param, setup in ((ZSTD_c_enableLongDistanceMatching, None), (None, "single")):
            for index in (False, True):
                with make_compressor(1, dic, index, ((param, 1),) if param else ()) as c:
                    if setup:
                        c.single_frame = True
                    cap = gpu_lib.ZSTD_compressBound(len(recs[-1]))
                    buf = ctypes.create_string_buffer(cap)
                    r = gpu_lib.ZSTD_compress2(c.cctx, buf, cap, recs[-1], len(recs[-1]))
                    assert is_error(r) and get_error_code(r) == 40, (param, setup, index)      # parameter_unsupported
    # a referenced prefix, the short form (the path of a raw-content dictionary) and the long one
    for level in (1, 3):
        with make_compressor(level, None, False) as off, make_compressor(level, None, True) as on:
            for pfx, items in ((raw_dict, recs[:4]), (datagen.gen("text", 100000, 3), recs[2:5])):
                for r in items:
                    off.RefPrefix(pfx); on.RefPrefix(pfx)
                    assert on.Wrap(r) == off.Wrap(r), (level, len(pfx), len(r))


# ---------------------------------------------------------------- 6. the corpus the dictionary was trained for ----------------------------------------------------------------
def test_json_corpus_is_not_larger_with_the_index(gpu_lib, oracle):
    """Level 1, entropy switch on, 1000 held-out JSON records against the dictionary trained on their kind: the index offers the
    finder a superset of the dictionary candidates the staged tail offered, so the total must not grow (off: 75 352 B on record;
    the oracle: 71 256 B)."""
    recs, dic = mgt.json_records(2000, 77)[1000:], golden_bytes("train_default_json.dict")
    with make_compressor(1, dic, True, entropy=True) as c:
        comps = z.compress_batch(c, recs)
        on = sum(map(len, comps))
    with make_compressor(1, dic, False, entropy=True) as c:
        off = sum(map(len, z.compress_batch(c, recs)))
    ref = sum(len(oracle.compress_dict(r, dic, 1)) for r in recs)
    print(f"json corpus level 1, entropy on: index on {on} B, off {off} B, oracle {ref} B")
    roundtrip(comps, recs, dic, oracle)
    assert on <= off, (on, off)
