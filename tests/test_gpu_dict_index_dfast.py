"""GPU tests of ZSTDMI_CCtx_setDictIndexStrategy(2): the dictionary index (ZSTDMI_CCtx_setDictIndex) also serves the dual-hash finder,
that is level 3 — the default level — and every call that resolves to the doubleFast strategy.  "On" below means index on with the
setting at 2.  The dictionary is indexed once per upload under both of the finder's hashes, nothing of it is staged per chunk, a
source of up to 64 KiB is one block in one frame, every frame decodes under the oracle's dictionary decoder and under the GPU
decoder, every entry point writes the same bytes, and nothing outside "a dictionary at the dual-hash finder" moves by a byte.
Helpers and record sets are those of test_gpu_dict_index.py, extended with the setting."""
import ctypes
import io

import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import get_error_code, is_error

from test_gpu_dict_index import (K_FAR_MAX, VIS, device_singles, dictionary, door_records, frames_of, golden_bytes, mgt, rand_dict, roundtrip,
                                 size_records)

pytestmark = pytest.mark.gpu

ZSTD_c_windowLog, ZSTD_c_strategy, ZSTD_c_enableLongDistanceMatching = 101, 107, 160
ZSTD_c_checksumFlag, ZSTD_c_dictIDFlag = 201, 202
# the two ways to the dual-hash finder: by level, and by strategy on top of a level of the fast one
DUAL = [pytest.param(3, (), id="level3"), pytest.param(1, ((ZSTD_c_strategy, 2),), id="level1-strategy2")]


def make_compressor(level, dic=None, index=True, setting=2, params=(), entropy=False, order="dis"):
    """order: the three setup calls — d = LoadDictionary, i = dict_index, s = dict_index_strategy — in the order given"""
    c = z.Compressor(level)
    for p, v in params:
        c.SetParameter(p, v)
    for step in order:
        if step == "d" and dic is not None:
            c.LoadDictionary(dic)
        elif step == "i":
            c.dict_index = index
        elif step == "s":
            c.dict_index_strategy = setting
    if entropy:
        c.dict_entropy = True
    return c


# ---------------------------------------------------------------- 1. the whole dictionary is seen ----------------------------------------------------------------
@pytest.mark.parametrize("level,params", DUAL)
def test_records_cut_from_anywhere_in_the_dictionary_are_found(gpu_lib, oracle, level, params):
    """D is 112 640 random bytes, so the only redundancy of D[a:a+n] is the dictionary itself.  On: at most n // 4 bytes, the
    threshold of the level-1 test.  With the setting at 1 the dual finder sees the staged 60 KiB tail alone, and a record cut in
    front of it is stored, at least n bytes: the gap this setting closes, and the assertion that fails without it."""
    D = rand_dict()
    recs = [D[a:a + n] for a, n in VIS]
    with make_compressor(level, D, True, 2, params) as c:
        on = [c.Wrap(r) for r in recs]
        assert gpu_lib.ZSTDMI_debugDictIndexed(c.cctx) == 112640
    with make_compressor(level, D, True, 1, params) as c:
        one = [c.Wrap(r) for r in recs]
        assert gpu_lib.ZSTDMI_debugDictIndexed(c.cctx) == 112640
    with make_compressor(1, D, True, 1) as c:
        fast = [c.Wrap(r) for r in recs]
    print("visibility (a, n) -> setting 2 / setting 1 / level 1 index on:", [(an, len(x), len(y), len(f)) for an, x, y, f in zip(VIS, on, one, fast)])
    roundtrip(on, recs, D, oracle)
    roundtrip(one, recs, D, oracle)
    for (a, n), x, y in zip(VIS, on, one):
        assert len(x) <= n // 4, (a, n, len(x))
        if a in (0, 40000):
            assert len(y) >= n, (a, n, len(y))


@pytest.mark.parametrize("level,params", DUAL)
def test_mixed_record_takes_three_far_matches(gpu_lib, oracle, level, params):
    D, f = rand_dict(), datagen.gen("rand", 300, 9)
    rec = D[1000:1700] + f[:100] + D[45000:45700] + f[100:200] + D[100000:100700]
    with make_compressor(level, D, True, 2, params) as c:
        comp = c.Wrap(rec)
    with make_compressor(1, D, True, 1) as c:
        fast = c.Wrap(rec)
    print(f"mixed record: setting 2 {len(comp)} B, level 1 index on {len(fast)} B")
    roundtrip([comp], [rec], D, oracle)
    assert len(comp) <= 200 + 2300 // 4, len(comp)


@pytest.mark.parametrize("level,params", DUAL)
def test_index_covers_the_last_188_kib_of_a_long_dictionary(gpu_lib, oracle, level, params):
    big = datagen.gen("text", 262144, 31)
    first = 262144 - K_FAR_MAX
    recs = [big[first:first + 3000], big[-3000:], big[first - 3000:first], big[:3000]]
    with make_compressor(level, big, True, 2, params) as c:
        comps = [c.Wrap(r) for r in recs]
        assert gpu_lib.ZSTDMI_debugDictIndexed(c.cctx) == K_FAR_MAX
    print("long dictionary: first / last indexed 3000 B, 3000 B in front of the index, the dictionary's first:", [len(x) for x in comps])
    roundtrip(comps, recs, big, oracle)
    assert len(comps[0]) <= 3000 // 4 and len(comps[1]) <= 3000 // 4, (len(comps[0]), len(comps[1]))


# ---------------------------------------------------------------- 2. round trips ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["rawcontent_6000.dict", "trained_16k.dict", "train_default_json.dict", "D"])
def test_round_trips(gpu_lib, oracle, name):
    dic, recs = dictionary(name), size_records()
    variants = [(3, (), False), (3, ((ZSTD_c_checksumFlag, 1),), False), (3, ((ZSTD_c_dictIDFlag, 0),), False), (3, (), True),
                (1, ((ZSTD_c_strategy, 2),), False)]
    sizes = {}
    for level, params, entropy in variants:
        with make_compressor(level, dic, True, 2, params, entropy) as c:
            comps = z.compress_batch(c, recs)
            assert gpu_lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
        roundtrip(comps, recs, dic, oracle)
        for r, cz in zip(recs, comps):      # up to 64 KiB: one frame; above: independent 64 KiB frames
            assert len(frames_of(cz, oracle)) == (len(r) + 65535) // 65536, (level, len(r))
        sizes[(level, params, entropy)] = sum(map(len, comps))
    print(f"{name}: totals {sizes}")


# ---------------------------------------------------------------- 3. the dictionary's seams ----------------------------------------------------------------
@pytest.mark.parametrize("level,params", DUAL)
def test_dictionary_seams(gpu_lib, oracle, level, params):
    D = rand_dict()
    recs = [D[-64:] + datagen.gen("text", 500, 1), D[-200:] * 3, D[3:600], D[:16] + datagen.gen("rand", 40, 5) + D[5:400],
            D[-8:], D[-7:], D[-300:], datagen.gen("rand", 20, 6) + D[-40:] + D[:40]]
    with make_compressor(level, D, True, 2, params) as c:
        comps = z.compress_batch(c, recs)
        assert [c.Wrap(r) for r in recs] == comps
    roundtrip(comps, recs, D, oracle)
    assert len(comps) == len(recs)


@pytest.mark.parametrize("level,params", DUAL)
@pytest.mark.parametrize("size", [8, 12, 15])
def test_dictionaries_of_one_hashable_position_or_a_few(gpu_lib, oracle, level, params, size):
    tiny = datagen.gen("rand", size, 50 + size)
    recs = [tiny, tiny * 5, tiny[1:] + tiny, datagen.gen("text", 700, 2) + tiny + datagen.gen("text", 300, 3), datagen.gen("rand", 100, 4), tiny[:7]]
    with make_compressor(level, tiny, True, 2, params) as c:
        comps = z.compress_batch(c, recs)
        assert gpu_lib.ZSTDMI_debugDictIndexed(c.cctx) == size
        assert [c.Wrap(r) for r in recs] == comps
    roundtrip(comps, recs, tiny, oracle)


# ---------------------------------------------------------------- 4. equal bytes from every entry point ----------------------------------------------------------------
@pytest.mark.parametrize("level,params", DUAL)
@pytest.mark.parametrize("name", ["D", "trained_16k.dict"])
def test_every_entry_point_writes_the_same_bytes(gpu_lib, oracle, name, level, params):
    import torch
    dic, recs = dictionary(name), door_records()
    with make_compressor(level, dic, True, 2, params) as c:
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
    with make_compressor(level, dic, True, 1, params) as c1:               # (the setting does something here)
        assert any(c1.Wrap(r) != s for r, s in zip(recs[:12], singles))
    for order in ("sid", "isd", "ids", "dsi"):                             # fresh contexts, the three setup calls in other orders
        with make_compressor(level, dic, True, 2, params, order=order) as c2:
            assert [c2.Wrap(r) for r in recs] == singles, order
    with make_compressor(level, dic, True, 2, params) as c3:               # the streaming adapter, one flush per record
        sink = io.BytesIO()
        st = z.CompressionStream(sink, compressor=c3)
        for r, s in zip(recs, singles):
            at = sink.tell()
            st.Write(r); st.Flush()
            assert sink.getvalue()[at:] == s, len(r)
        st.Dispose()
    # two workers: device 0 and 1 when there are two, else device 0 listed twice (each worker has its own copy of the three tables)
    with make_compressor(level, dic, True, 2, params) as c4:
        arr = (ctypes.c_int * 2)(0, 1 if torch.cuda.device_count() >= 2 else 0)
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c4.cctx, arr, 2) == 0
        for i in list(range(0, len(recs), 4)) + [4, 5, 6]:
            assert c4.Wrap(recs[i]) == singles[i], (i, len(recs[i]))


@pytest.mark.parametrize("name", ["D", "trained_16k.dict"])
def test_level_changes_need_no_new_dictionary_load(gpu_lib, oracle, name):
    """One context at level 1, then 3, then 1, then doubleFast by ZSTD_c_strategy, the dictionary loaded once: an upload at setting 2
    builds the fast finder's table beside the dual finder's two, so each level writes what a fresh context at that level writes."""
    dic, recs = dictionary(name), door_records()[::3]
    fresh = {}
    for level in (1, 3):
        with make_compressor(level, dic, True, 2) as c:
            fresh[level] = [c.Wrap(r) for r in recs]
    assert fresh[1] != fresh[3]
    with make_compressor(1, dic, True, 2) as c:
        for level in (1, 3, 1):
            c.Level = level
            assert [c.Wrap(r) for r in recs] == fresh[level], level
        c.SetParameter(ZSTD_c_strategy, 2)
        with make_compressor(1, dic, True, 2, ((ZSTD_c_strategy, 2),)) as f2:
            assert [c.Wrap(r) for r in recs] == [f2.Wrap(r) for r in recs]
    roundtrip(fresh[3], recs, dic, oracle)


# ---------------------------------------------------------------- 5. nothing else moves ----------------------------------------------------------------
def both(level, dic, index, params=()):
    return make_compressor(level, dic, index, 1, params), make_compressor(level, dic, index, 2, params)


def test_setting_changes_nothing_where_promised(gpu_lib, oracle):
    recs = [datagen.gen("text", n, 70 + n) for n in (40, 300, 5000, 30000, 70000, 300000)]
    raw_dict, fmt_dict, D = golden_bytes("rawcontent_6000.dict"), golden_bytes("trained_16k.dict"), rand_dict()

    def same(one, two, items=recs, tag=None):
        with one, two:
            for r in items:
                assert two.Wrap(r) == one.Wrap(r), (tag, len(r))

    # no dictionary; a dictionary below 8 bytes
    same(*both(3, None, True), tag="none")
    same(*both(3, b"abcdefg", True), tag="7 bytes")
    for dic in (raw_dict, fmt_dict, D):
        # the setting alone, the index off
        for level in (1, 3, 5):
            same(*both(level, dic, False), tag=f"index off, level {level}")
        # the chain finder; the fast finder, whose instance the setting does not touch
        same(*both(5, dic, True), tag="level 5")
        same(*both(1, dic, True), tag="level 1")
        same(*both(-5, dic, True), tag="level -5")
        # windows below the block
        for wl in (10, 15):
            same(*both(3, dic, True, ((ZSTD_c_windowLog, wl),)), tag=f"windowLog {wl}")
        # ZSTD_compressCCtx uses no dictionary, loaded or not
        with make_compressor(3, dic, True, 1) as one, make_compressor(3, dic, True, 2) as two:
            for r in recs:
                cap = gpu_lib.ZSTD_compressBound(len(r))
                a, b = ctypes.create_string_buffer(cap), ctypes.create_string_buffer(cap)
                na = gpu_lib.ZSTD_compressCCtx(one.cctx, a, cap, r, len(r), 3)
                nb = gpu_lib.ZSTD_compressCCtx(two.cctx, b, cap, r, len(r), 3)
                assert not is_error(na) and na == nb and a.raw[:na] == b.raw[:nb], len(r)
        # to 2 and back to 1 = a context that never heard of the setting
        with make_compressor(3, dic, True, 1, order="di") as fresh, make_compressor(3, dic, True, 2) as back:
            changed = [back.Wrap(r) for r in recs]
            back.dict_index_strategy = 1
            for r in recs:
                assert back.Wrap(r) == fresh.Wrap(r), len(r)
            assert any(ch != fresh.Wrap(r) for r, ch in zip(recs, changed))      # (the setting did something while it was 2)
        # the refusals stay: long-distance matching above one block, one frame per call above one block
        for param, setup in ((ZSTD_c_enableLongDistanceMatching, None), (None, "single")):
            for setting in (1, 2):
                with make_compressor(3, dic, True, setting, ((param, 1),) if param else ()) as c:
                    if setup:
                        c.single_frame = True
                    cap = gpu_lib.ZSTD_compressBound(len(recs[-1]))
                    buf = ctypes.create_string_buffer(cap)
                    r = gpu_lib.ZSTD_compress2(c.cctx, buf, cap, recs[-1], len(recs[-1]))
                    assert is_error(r) and get_error_code(r) == 40, (param, setup, setting)      # parameter_unsupported
    # a referenced prefix, the short form (the path of a raw-content dictionary) and the long one
    with make_compressor(3, None, True, 1) as one, make_compressor(3, None, True, 2) as two:
        for pfx, items in ((raw_dict, recs[:4]), (datagen.gen("text", 100000, 3), recs[2:5])):
            for r in items:
                one.RefPrefix(pfx); two.RefPrefix(pfx)
                assert two.Wrap(r) == one.Wrap(r), (len(pfx), len(r))


# ---------------------------------------------------------------- 6. the corpus the dictionary was trained for ----------------------------------------------------------------
@pytest.mark.parametrize("entropy", [False, True], ids=["entropy-off", "entropy-on"])
def test_json_corpus_is_not_larger_with_the_index(gpu_lib, oracle, entropy):
    """Level 3, 1000 held-out JSON records against the dictionary trained on their kind (112 640 bytes, of which the staged tail
    holds 60 KiB): the index shows the finder the whole dictionary, so the total must not grow against the setting at 1."""
    recs, dic = mgt.json_records(2000, 77)[1000:], golden_bytes("train_default_json.dict")
    with make_compressor(3, dic, True, 2, entropy=entropy) as c:
        comps = z.compress_batch(c, recs)
        on = sum(map(len, comps))
    with make_compressor(3, dic, True, 1, entropy=entropy) as c:
        one = sum(map(len, z.compress_batch(c, recs)))
    with make_compressor(1, dic, True, 1, entropy=entropy) as c:
        fast = sum(map(len, z.compress_batch(c, recs)))
    print(f"json corpus level 3, entropy {'on' if entropy else 'off'}: setting 2 {on} B, setting 1 {one} B; level 1 index on {fast} B")
    roundtrip(comps, recs, dic, oracle)
    assert on <= one, (on, one)
