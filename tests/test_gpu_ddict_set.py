"""GPU tests of ZSTD_d_refMultipleDDicts (include/zstd_mi355x.h "many dictionaries, one context"): a context whose ZSTD_DCtx_refDDict
calls collect a SET of DDicts decodes every frame behind the DDict its header names.  The yardstick is never the set path: it is the
original data, and each frame decoded alone by a fresh single-DDict context (RefDDict(its DDict) + the single call) — error codes
included.  ZSTDMI_debugLastSetFrames counts the frames whose dictionary was found in the set by dictID."""
import ctypes
import functools
import hashlib
import io
import os
import random
import struct

import numpy as np
import pytest

import datagen
import forge_cases
import oracle_lib
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIVE = ("train_default_json.dict", "train_default_text.dict", "train_default_zipf.dict", "trained_16k.dict", "train_d8_f20_a1_k50_4k.dict")
RAW = "rawcontent_6000.dict"
WRONG = ZSTD_ErrorCode.ZSTD_error_dictionary_wrong
UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_parameter_unsupported


@functools.lru_cache(maxsize=None)
def dic(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def with_id(d, dict_id):
    """a formatted dictionary's bytes under another dictID (bytes 4..7)"""
    return d[:4] + struct.pack("<I", dict_id) + d[8:]


def gpu_frame(data, dictionary, level=1, entropy=False, dict_id_flag=1, content_size=1):
    with z.Compressor(level) as c:
        c.dict_entropy = entropy
        c.SetParameter(202, dict_id_flag)           # ZSTD_c_dictIDFlag
        c.SetParameter(200, content_size)           # ZSTD_c_contentSizeFlag
        c.LoadDictionary(dictionary)
        return c.Wrap(data)


@functools.lru_cache(maxsize=None)
def records():
    """((data, frame, index into FIVE), ...): 40 records of 300 B to 4 KiB, neighbours behind different dictionaries, levels 1 and 3,
    the dictionary's entropy tables on for every other one (treeless literals, repeated sequence tables)"""
    sizes = (300, 777, 1500, 4096, 2049, 3333, 512, 4000)
    out = []
    comps = {}
    pool = {"text": datagen.gen("text", 120000, 500), "zipf": datagen.gen("zipf", 120000, 501)}       # (one generator call per kind: records are slices)
    for i in range(40):
        k, level, entropy = i % 5, 1 if i % 2 else 3, i % 4 < 2
        data = pool["zipf" if k == 2 else "text"][2500 * i:2500 * i + sizes[i % len(sizes)]]
        key = (k, level, entropy)
        if key not in comps:
            c = z.Compressor(level)
            c.dict_entropy = entropy
            c.LoadDictionary(dic(FIVE[k]))
            comps[key] = c
        out.append((data, comps[key].Wrap(data), k))
    for c in comps.values():
        c.Dispose()
    for data, frame, k in out:
        assert z.get_dict_id_from_frame(frame) == z.get_dict_id_from_dict(dic(FIVE[k]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def long_frames():
    """two multi-block frames: libzstd's dict_fmt_200000_l3.zst behind trained_16k.dict (content known by its SHA-256), and 200 000
    bytes of text in one frame of the oracle's behind train_default_json.dict -> ((content or None, frame, index into FIVE, size), ...)"""
    golden = open(os.path.join(GOLDEN, "dict_fmt_200000_l3.zst"), "rb").read()
    text = datagen.gen("text", 200000, 91)
    own = oracle_lib.compress_dict(text, dic(FIVE[0]), 1)         # (the oracle compresses behind a dictionary at levels 1-2)
    assert isinstance(own, bytes) and z.get_dict_id_from_frame(own) == z.get_dict_id_from_dict(dic(FIVE[0]))
    return ((None, golden, 3, 200000), (text, own, 0, 200000))


GOLDEN_200000_SHA = "cbecf35f24e6941592e80d49585fe9c7b733dba7ccc0b831fa016f433a3c6863"


@pytest.fixture(scope="module")
def ddicts(gpu_lib):
    """the five formatted DDicts and the raw-content one, made once"""
    dd = {name: z.DDict(dic(name)) for name in FIVE + (RAW,)}
    assert len({d.dict_id for d in dd.values()}) == 6 and dd[RAW].dict_id == 0
    yield dd
    for d in dd.values():
        d.Dispose()


def set_context(dds, current=None, lit=0, waves=0, overlap=0, long_frames_mode=0):
    """a context with the parameter on that has referenced every DDict of dds, `current` (default: the last) last"""
    d = z.Decompressor()
    d.SetParameter(z.ZSTD_d_refMultipleDDicts, 1)
    for dd in dds:
        d.RefDDict(dd)
    if current is not None:
        d.RefDDict(current)
    lib = d._lib
    assert lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, lit) == 0 and lib.ZSTDMI_DCtx_setExecWaves(d.dctx, waves) == 0
    assert lib.ZSTDMI_DCtx_setOverlap(d.dctx, overlap) == 0 and lib.ZSTDMI_DCtx_setLongFrames(d.dctx, long_frames_mode) == 0
    return d


def raw_call(lib, d, blob, room):
    out = ctypes.create_string_buffer(max(room, 1) + 8)
    ctypes.memset(ctypes.addressof(out) + room, 0xA5, 8)
    r = lib.ZSTD_decompressDCtx(d.dctx, out, room, blob, len(blob))
    assert out.raw[room:room + 8] == b"\xA5" * 8, "written beyond the capacity"
    return r, (b"" if is_error(r) else out.raw[:r])


def device_call(lib, d, blob, room):
    import torch
    src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    out = torch.full((max(room, 1) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), room, src.data_ptr(), len(blob))
    host = out.cpu().numpy().tobytes()
    assert host[room:room + 8] == b"\xA5" * 8, "written beyond the capacity"
    return r, (b"" if is_error(r) else host[:r])


def alone(lib, dd, blob, room):
    """the yardstick: the single call of a fresh context that references this one DDict (None: no dictionary)"""
    with z.Decompressor() as y:
        if dd is not None:
            y.RefDDict(dd)
        r = raw_call(lib, y, blob, room)
        assert lib.ZSTDMI_debugLastSetFrames(y.dctx) == 0
        y.RefDDict(None)
    return r


def batch_raw(lib, d, blobs, caps):
    """ZSTDMI_decompressBatch over device buffers with 16 canary bytes behind every capacity -> [(value, bytes), ...]"""
    import torch
    n = len(blobs)
    src = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
    starts, at = [], 0
    for c in caps:
        starts.append(at)
        at += c + 16
    out = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    srcs, p = [], src.data_ptr()
    for b in blobs:
        srcs.append(p)
        p += len(b)
    got = (ctypes.c_size_t * n)()
    torch.cuda.synchronize()
    r = lib.ZSTDMI_decompressBatch(d.dctx, (ctypes.c_void_p * n)(*srcs), (ctypes.c_size_t * n)(*[len(b) for b in blobs]), n,
                                   (ctypes.c_void_p * n)(*[out.data_ptr() + s for s in starts]), (ctypes.c_size_t * n)(*caps), got)
    assert r == 0, get_error_code(r)
    host = out.cpu().numpy().tobytes()
    res = []
    for i in range(n):
        assert host[starts[i] + caps[i]:starts[i] + caps[i] + 16] == b"\xA5" * 16, f"entry {i} wrote beyond its capacity"
        res.append((got[i], b"" if is_error(got[i]) else host[starts[i]:starts[i] + got[i]]))
    return res


def code_of(result):
    return get_error_code(result[0]) if is_error(result[0]) else None


# ---------------------------------------------------------------- 1. a mixed concatenation in one call ----------------------------------------------------------------
@pytest.mark.parametrize("lit", [0, 1, 2, 3])
def test_mixed_concatenation_in_one_call(gpu_lib, ddicts, lit):
    recs, longs = records(), long_frames()
    five = [ddicts[name] for name in FIVE]
    golden_content = alone(gpu_lib, five[3], longs[0][1], 200000)
    assert golden_content[0] == 200000 and hashlib.sha256(golden_content[1]).hexdigest() == GOLDEN_200000_SHA
    parts = [(data, frame) for data, frame, _ in recs[:20]] + [(golden_content[1], longs[0][1])] + \
            [(data, frame) for data, frame, _ in recs[20:]] + [(longs[1][0], longs[1][1])]
    stream, data = b"".join(f for _, f in parts), b"".join(d for d, _ in parts)
    n_frames = len(parts)
    for waves in (1, 4, 16):
        for overlap in (1, 2):
            with set_context(five, lit=lit, waves=waves, overlap=overlap) as d:
                for call in (raw_call, device_call):
                    r = call(gpu_lib, d, stream, len(data))
                    assert r[0] == len(data) and r[1] == data, (lit, waves, overlap, call.__name__)
                    assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == n_frames
                    assert gpu_lib.ZSTDMI_debugLastDictTableBlocks(d.dctx) > 0
                assert gpu_lib.ZSTDMI_debugDictUploadsD(d.dctx) == 0
                d.RefDDict(None)


# ---------------------------------------------------------------- 2. the batch ----------------------------------------------------------------
def first_block(frame):
    """-> (type of the frame's first block, offset of its body)"""
    fhd = frame[4]
    single, did, fcs = (fhd >> 5) & 1, (0, 1, 2, 4)[fhd & 3], fhd >> 6
    at = 5 + (0 if single else 1) + did + ((1 if single else 0) if fcs == 0 else (1 << fcs))
    bh = frame[at] | (frame[at + 1] << 8) | (frame[at + 2] << 16)
    return (bh >> 1) & 3, at + 3


def own_tree(frame):
    """the frame's first block is compressed and its literals section is Huffman-coded with a tree of its own"""
    btype, body = first_block(frame)
    return btype == 2 and frame[body] & 3 == 2


def huffman_damaged(frame):
    """the frame with a byte inside its first block's last Huffman stream changed"""
    assert own_tree(frame)
    body = first_block(frame)[1]
    lhl = (frame[body] >> 2) & 3
    lhc = int.from_bytes(frame[body:body + 5], "little")
    lh, csize = (3, (lhc >> 14) & 0x3FF) if lhl < 2 else (4, (lhc >> 18) & 0x3FFF) if lhl == 2 else (5, (lhc >> 22) & 0x3FFFF)
    pos = body + lh + csize - 3
    out = bytearray(frame)
    out[pos] ^= 0x5A
    return bytes(out)


def test_batch_entries_equal_their_single_decodes(gpu_lib, ddicts):
    recs = records()
    five = [ddicts[name] for name in FIVE]
    victim = next(i for i, (data, frame, k) in enumerate(recs) if len(data) >= 1500 and own_tree(frame))
    foreign_dict = with_id(dic(FIVE[4]), 0x5EED5EED)
    foreign = gpu_frame(recs[3][0], foreign_dict)
    unsized_data = datagen.gen("text", 3000, 17)
    unsized = gpu_frame(unsized_data, dic(FIVE[1]), content_size=0)
    assert z.get_dict_id_from_frame(unsized) == ddicts[FIVE[1]].dict_id
    blobs = [frame for _, frame, _ in recs]
    owner = [five[k] for _, _, k in recs]
    caps = [len(data) for data, _, _ in recs]
    extra = [(huffman_damaged(recs[victim][1]), owner[victim], caps[victim]), (recs[7][1][:-6], owner[7], caps[7]),
             (foreign, five[4], len(recs[3][0])), (unsized, five[1], 3000)]
    # interleave the four special entries with intact neighbours
    for j, (b, o, c) in enumerate(extra):
        at = 5 + 9 * j
        blobs.insert(at, b); owner.insert(at, o); caps.insert(at, c)
    with set_context(five, current=five[4]) as d:
        got = batch_raw(gpu_lib, d, blobs, caps)
        n_set = gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx)
        alone_entries = gpu_lib.ZSTDMI_debugLastBatchAloneD(d.dctx)
        for i, (b, o, c) in enumerate(zip(blobs, owner, caps)):
            want = alone(gpu_lib, o, b, c)
            assert got[i] == want, (i, code_of(got[i]), code_of(want))
        d.RefDDict(None)
    specials = {5 + 9 * j for j in range(4)}
    assert all(not is_error(got[i][0]) for i in range(len(blobs)) if i not in specials)
    assert is_error(got[14][0]), "a truncated frame"
    assert code_of(got[23]) == WRONG, "a dictID that is not in the set"
    assert got[32] == (3000, unsized_data) and alone_entries == 1, "a frame without a content size goes alone and still selects by dictID"
    # every entry whose frames were listed was found in the set (the damaged and the unsized one included); the truncated and the foreign
    # one end in the walk and are not counted
    assert n_set == len(blobs) - 2, n_set


# ---------------------------------------------------------------- 3. the rule ----------------------------------------------------------------
def test_frames_without_a_dict_id_use_the_current_ddict(gpu_lib, ddicts):
    a, b = ddicts[FIVE[3]], ddicts[FIVE[0]]
    data = [datagen.gen("text", 2000 + 100 * i, 40 + i) for i in range(3)]
    anon = [gpu_frame(x, dic(FIVE[3]), level=3, entropy=True, dict_id_flag=0) for x in data]
    assert all(z.get_dict_id_from_frame(f) == 0 for f in anon)
    named_data, named, _ = next(r for r in records() if r[2] == 3)
    for current in (a, b):
        want = [alone(gpu_lib, current, f, len(x)) for f, x in zip(anon, data)]
        if current is a:
            assert [w[1] for w in want] == data
        else:
            assert all(w[1] != x for w, x in zip(want, data)), "behind B the frames give an error or other bytes"
        with set_context([a, b], current=current) as d:
            for f, x, w in zip(anon, data, want):
                assert raw_call(gpu_lib, d, f, len(x)) == w
            # a neighbour that names A changes nothing, in one call and in one batch
            if not any(is_error(w[0]) for w in want):
                stream = named + anon[0] + named + anon[1]
                expect = named_data + want[0][1] + named_data + want[1][1]
                assert raw_call(gpu_lib, d, stream, len(expect)) == (len(expect), expect)
                assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 2
            got = batch_raw(gpu_lib, d, [named, anon[0], named, anon[1], anon[2]], [len(named_data), len(data[0]), len(named_data), len(data[1]), len(data[2])])
            assert got == [(len(named_data), named_data), want[0], (len(named_data), named_data), want[1], want[2]]
            d.RefDDict(None)


def test_an_equal_dict_id_replaces_the_entry(gpu_lib, ddicts):
    content1, content2 = datagen.gen("text", 6000, 1), datagen.gen("text", 6000, 2)
    sample = datagen.gen("text", 20000, 3)
    d1, d2 = oracle_lib.make_dictionary(content1, sample, 777), oracle_lib.make_dictionary(content2, sample, 777)
    data = content1[1000:3000] + content1[4000:5500] + datagen.gen("text", 500, 4)
    frame = oracle_lib.compress_dict(data, d1, 1)
    assert z.get_dict_id_from_frame(frame) == 777
    other = ddicts[FIVE[0]]
    with z.DDict(d1) as dd1, z.DDict(d2) as dd2:
        w1, w2 = alone(gpu_lib, dd1, frame, len(data)), alone(gpu_lib, dd2, frame, len(data))
        assert w1 == (len(data), data) and w2 != w1
        with set_context([dd1, other]) as d:
            assert raw_call(gpu_lib, d, frame, len(data)) == w1 and gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 1
            d.RefDDict(dd2)             # replaces 777; it is current now
            d.RefDDict(other)
            assert raw_call(gpu_lib, d, frame, len(data)) == w2 and gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 1
            d.RefDDict(dd1)
            d.RefDDict(other)
            assert raw_call(gpu_lib, d, frame, len(data)) == w1
            d.RefDDict(None)


def test_clearing_the_current_ddict_leaves_the_set(gpu_lib, ddicts):
    five = [ddicts[name] for name in FIVE]
    recs = records()
    (da, fa, _), (db, fb, _) = next(r for r in recs if r[2] == 0), next(r for r in recs if r[2] == 1)
    with z.Decompressor() as none:
        no_dict = raw_call(gpu_lib, none, fa, len(da))
        assert code_of(no_dict) == WRONG
    with set_context(five[:3]) as d:
        assert raw_call(gpu_lib, d, fa + fb, len(da) + len(db)) == (len(da) + len(db), da + db)
        d.RefDDict(None)                                        # no dictionary; the set stays
        assert raw_call(gpu_lib, d, fa, len(da)) == no_dict and gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 0
        d.RefDDict(five[2])                                     # ... and is found again
        assert raw_call(gpu_lib, d, fa + fb, len(da) + len(db)) == (len(da) + len(db), da + db)
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 2
        d.LoadDictionary(dic(FIVE[1]))                          # clears the current DDict only: a single loaded dictionary now
        assert raw_call(gpu_lib, d, fb, len(db)) == (len(db), db) and code_of(raw_call(gpu_lib, d, fa, len(da))) == WRONG
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 0
        d.RefDDict(five[2])
        assert raw_call(gpu_lib, d, fa, len(da)) == (len(da), da)
        d.RefPrefix(dic(RAW))                                   # clears the current DDict only; serves one call
        assert code_of(raw_call(gpu_lib, d, fa, len(da))) == WRONG
        d.RefDDict(five[2])
        assert raw_call(gpu_lib, d, fa, len(da)) == (len(da), da) and gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 1
        # the parameter back at 0 with the set present: a single-DDict context with its current DDict
        d.SetParameter(z.ZSTD_d_refMultipleDDicts, 0)
        (dc, fc, _) = next(r for r in recs if r[2] == 2)
        assert raw_call(gpu_lib, d, fc, len(dc)) == alone(gpu_lib, five[2], fc, len(dc)) == (len(dc), dc)
        assert raw_call(gpu_lib, d, fa, len(da)) == alone(gpu_lib, five[2], fa, len(da)) and code_of(raw_call(gpu_lib, d, fa, len(da))) == WRONG
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 0
        d.SetParameter(z.ZSTD_d_refMultipleDDicts, 1)
        assert raw_call(gpu_lib, d, fa, len(da)) == (len(da), da)
        d.RefDDict(None)


def test_a_raw_content_ddict_as_the_current_one(gpu_lib, ddicts):
    raw = ddicts[RAW]
    a = ddicts[FIVE[3]]
    da, fa, _ = next(r for r in records() if r[2] == 3)
    piece = dic(RAW)[1000:3000] + datagen.gen("text", 800, 5)
    raw_frame = oracle_lib.compress_dict(piece, dic(RAW), 1)
    assert z.get_dict_id_from_frame(raw_frame) == 0
    with set_context([a, ddicts[FIVE[0]]], current=raw) as d:
        assert raw_call(gpu_lib, d, raw_frame, len(piece)) == alone(gpu_lib, raw, raw_frame, len(piece)) == (len(piece), piece)
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 0
        stream = raw_frame + fa + raw_frame
        assert raw_call(gpu_lib, d, stream, 2 * len(piece) + len(da)) == (2 * len(piece) + len(da), piece + da + piece)
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 1, "the frame naming a set member selects it; the raw-content DDict is never selected"
        d.RefDDict(None)


def test_using_ddict_ignores_the_set(gpu_lib, ddicts):
    five = [ddicts[name] for name in FIVE]
    recs = records()
    (da, fa, _), (db, fb, _) = next(r for r in recs if r[2] == 0), next(r for r in recs if r[2] == 1)
    with set_context(five[:3]) as d:
        out = ctypes.create_string_buffer(len(da) + len(db))
        r = gpu_lib.ZSTD_decompress_usingDDict(d.dctx, out, len(da), fa, len(fa), five[1].handle)
        assert is_error(r) and get_error_code(r) == WRONG, "ONE call behind that DDict alone"
        r = gpu_lib.ZSTD_decompress_usingDDict(d.dctx, out, len(db), fb, len(fb), five[1].handle)
        assert r == len(db) and out.raw[:r] == db and gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 0
        assert d.GetParameter(z.ZSTD_d_refMultipleDDicts) == 1
        assert raw_call(gpu_lib, d, fa + fb, len(da) + len(db)) == (len(da) + len(db), da + db), "the set is as it was found"
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 2
        d.RefDDict(None)


def test_a_frame_of_five_blocks_between_set_frames(gpu_lib, ddicts):
    """more blocks than a lane of block_link_small takes: block_link's set instance links them.  The frame is forged, has no dictID (the
    current DDict's) and repeats its first block's Huffman table in its last; its content is what zstd_forge's own executor regenerates"""
    five, content = next(c[2] for c in forge_cases.CASES if c[0] == "huf_treeless_gap_s4")()
    data, frame, k = records()[0]
    with set_context([ddicts[FIVE[k]], ddicts[FIVE[(k + 1) % 5]]]) as d:
        stream, expect = frame + five + frame, data + content + data
        assert raw_call(gpu_lib, d, stream, len(expect)) == (len(expect), expect)
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 2
        assert batch_raw(gpu_lib, d, [frame, five, frame], [len(data), len(content), len(data)]) == [(len(data), data), (len(content), content), (len(data), data)]
        d.RefDDict(None)


# ---------------------------------------------------------------- 4. the lookup at scale ----------------------------------------------------------------
def test_three_hundred_ddicts_in_one_batch(gpu_lib, ddicts):
    base = dic(FIVE[4])
    real_ids = {ddicts[name].dict_id for name in FIVE}
    ids = [1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF, 255, 256, 65535, 65536]
    rng = random.Random(9)
    while len(ids) < 295:
        v = rng.randrange(3, 1 << 32)
        if v not in ids and v not in real_ids:
            ids.append(v)
    copies = [z.DDict(with_id(base, i)) for i in ids]
    try:
        # a copy's frames differ from another copy's in the header's dictID only: compressed once behind one copy whose ID takes the
        # 4-byte field, which is then rewritten (a small ID in a wide field is valid, and one more case for the lookup)
        entries = []                                            # (data, frame, its DDict)
        pool = datagen.gen("text", 320 * len(ids), 2000)
        datas = [pool[320 * n:320 * n + 300 + n % 7] for n in range(len(ids))]
        with z.Compressor(1) as c:
            c.dict_entropy = True
            c.LoadDictionary(with_id(base, 0x12345678))
            frames = z.compress_batch(c, datas)
        for data, frame, i, dd in zip(datas, frames, ids, copies):
            at = frame.index(struct.pack("<I", 0x12345678))
            assert frame[4] & 3 == 3 and at in (5, 6)
            frame = frame[:at] + struct.pack("<I", i) + frame[at + 4:]
            assert z.get_dict_id_from_frame(frame) == i == dd.dict_id
            entries.append((data, frame, dd))
        for k, name in enumerate(FIVE):
            data, frame, _ = next(r for r in records() if r[2] == k)
            entries.append((data, frame, ddicts[name]))
        order = list(copies) + [ddicts[name] for name in FIVE]
        rng.shuffle(order)
        rng.shuffle(entries)
        with set_context(order) as d:
            got = batch_raw(gpu_lib, d, [f for _, f, _ in entries], [len(x) for x, _, _ in entries])
            assert [g[1] for g in got] == [x for x, _, _ in entries]
            assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == len(entries) == 300
            assert gpu_lib.ZSTDMI_debugDictUploadsD(d.dctx) == 0
            for data, frame, dd in entries[:6]:
                assert alone(gpu_lib, dd, frame, len(data)) == (len(data), data)
            d.RefDDict(None)
    finally:
        for dd in copies:
            dd.Dispose()


# ---------------------------------------------------------------- 5. origin pointers ----------------------------------------------------------------
def test_a_long_frame_between_short_ones_on_the_origin_path(gpu_lib, ddicts):
    a_bytes = dic(FIVE[1])
    tail = a_bytes[-60000:]                                     # (the content of a formatted dictionary is its end)
    rng = random.Random(3)
    head = b"".join(tail[o:o + 200] for o in (rng.randrange(0, len(tail) - 200) for _ in range(328)))[:65536]
    big = head + datagen.gen("text", (1 << 20) + 4096 - len(head), 77)
    assert len(big) == (1 << 20) + 4096
    big_frame = oracle_lib.compress_dict(big, a_bytes, 1)
    assert isinstance(big_frame, bytes) and z.get_dict_id_from_frame(big_frame) == ddicts[FIVE[1]].dict_id
    assert len(oracle_lib.compress_dict(head, a_bytes, 1)) < len(oracle_lib.compress(head, 1)) // 2, "the first 64 KiB hold matches into the dictionary"
    recs = records()
    (db, fb, _), (dc, fc, _) = next(r for r in recs if r[2] == 0), next(r for r in recs if r[2] == 3)
    stream, data = fb + big_frame + fc + fb, db + big + dc + db
    five = [ddicts[name] for name in FIVE]
    assert alone(gpu_lib, five[1], big_frame, len(big)) == (len(big), big)
    results = []
    for mode in (1, 2):
        with set_context(five, current=five[4], long_frames_mode=mode) as d:
            r = device_call(gpu_lib, d, stream, len(data))
            assert r[0] == len(data) and r[1] == data, mode
            assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 4
            results.append(r)
            d.RefDDict(None)
    assert results[0] == results[1]


# ---------------------------------------------------------------- 6. ranges and streams ----------------------------------------------------------------
def make_table(entries):
    """the seek table of `entries` = [(cSize, dSize), ...] (as tests/test_gpu_ranges.py writes it)"""
    body = b"".join(struct.pack("<II", c, d) for c, d in entries)
    foot = struct.pack("<IBI", len(entries), 0, 0x8F92EAB1)
    return struct.pack("<II", 0x184D2A5E, len(body) + 9) + body + foot


class Pieces:
    """a readable stream that hands out at most 1000 bytes a read"""
    def __init__(self, blob):
        self.blob, self.at = blob, 0

    def read(self, n=-1):
        n = 1000 if n is None or n < 0 else min(n, 1000)
        out = self.blob[self.at:self.at + n]
        self.at += len(out)
        return out


def test_ranges_and_streams_across_dictionary_changes(gpu_lib, ddicts):
    recs = [r for r in records() if r[2] in (0, 1, 3)][:15]
    assert {k for _, _, k in recs} == {0, 1, 3}
    frames, data = b"".join(f for _, f, _ in recs), b"".join(x for x, _, _ in recs)
    pack = frames + make_table([(len(f), len(x)) for x, f, _ in recs])
    three = [ddicts[FIVE[k]] for k in (0, 1, 3)]
    first = len(recs[0][0])
    ranges = [(0, len(data)), (first - 10, 3000), (first + 5, 1), (len(data) - 5000, 5000), (700, 9000), (len(data) - 1, 10)]
    with set_context(three) as d:
        for off, length in ranges:
            assert d.unwrap_range(pack, off, length) == data[off:off + length], (off, length)
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 1
        assert d.unwrap_range(pack, 0, len(data)) == data and gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == len(recs)
        assert d.unwrap_ranges(pack, ranges) == [data[o:o + n] for o, n in ranges]
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == len(recs)
        import torch
        dev = torch.from_numpy(np.frombuffer(pack, dtype=np.uint8).copy()).cuda()
        assert [t.cpu().numpy().tobytes() for t in d.unwrap_ranges(dev, ranges[1:4])] == [data[o:o + n] for o, n in ranges[1:4]]
        assert z.DecompressionStream(Pieces(frames), decompressor=d, segment=0).ReadToEnd() == data
        assert gpu_lib.ZSTDMI_debugDictUploadsD(d.dctx) == 0
        d.RefDDict(None)


# ---------------------------------------------------------------- 7. refusals and the unchanged path ----------------------------------------------------------------
def test_refusals(gpu_lib, ddicts):
    five = [ddicts[name] for name in FIVE]
    data, frame, k = records()[0]
    arr = (ctypes.c_int * 2)(0, 0)
    # several device workers
    with set_context(five[:2]) as d:
        assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, arr, 2) == 0
        assert code_of(raw_call(gpu_lib, d, frame, len(data))) == UNSUPPORTED
        with pytest.raises(z.ZstdException) as ei:
            z.decompress_batch(d, [frame], [len(data)])
        assert ei.value.code == UNSUPPORTED
        d.RefDDict(None)
    # a set of ONE with several device workers: the single-DDict path, private upload included
    with set_context([five[k]]) as d:
        assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, arr, 2) == 0
        assert raw_call(gpu_lib, d, frame, len(data)) == (len(data), data)
        assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 0 and gpu_lib.ZSTDMI_debugDictUploadsD(d.dctx) > 0
        d.RefDDict(None)
    # a stream segment
    with set_context(five[:2], current=five[k]) as d:
        d.stream_segment = 1
        with pytest.raises(z.ZstdException) as ei:
            z.DecompressionStream(io.BytesIO(frame), decompressor=d).ReadToEnd()
        assert ei.value.code == UNSUPPORTED
        d.stream_segment = 0
        assert z.DecompressionStream(io.BytesIO(frame), decompressor=d).ReadToEnd() == data
        d.RefDDict(None)
    # a set of one in segments: as before this parameter existed
    with set_context([five[k]]) as d:
        d.stream_segment = 1
        assert z.DecompressionStream(io.BytesIO(frame), decompressor=d).ReadToEnd() == data
        d.stream_segment = 0
        d.RefDDict(None)


def test_a_ddict_on_another_device_is_refused(gpu_lib, ddicts):
    if gpu_lib.ZSTDMI_deviceCount() < 2:
        pytest.skip("one device")
    data, frame, k = records()[0]
    with z.DDict(dic(FIVE[(k + 1) % 5]), device=1) as far:
        with set_context([far, ddicts[FIVE[k]]]) as d:
            assert code_of(raw_call(gpu_lib, d, frame, len(data))) == UNSUPPORTED
            d.RefDDict(None)


def test_a_set_of_one_and_no_parameter_are_the_single_ddict_path(gpu_lib, ddicts):
    recs = records()
    for k, name in enumerate(FIVE):
        mine = [(x, f) for x, f, kk in recs if kk == k]
        other = next(f for _, f, kk in recs if kk != k)
        stream, data = b"".join(f for _, f in mine), b"".join(x for x, _ in mine)
        want, want_other = alone(gpu_lib, ddicts[name], stream, len(data)), alone(gpu_lib, ddicts[name], other, 5000)
        assert want == (len(data), data) and code_of(want_other) == WRONG
        with set_context([ddicts[name]]) as one, z.Decompressor() as never:
            never.RefDDict(ddicts[name])
            for d in (one, never):
                assert raw_call(gpu_lib, d, stream, len(data)) == want and device_call(gpu_lib, d, stream, len(data)) == want
                assert raw_call(gpu_lib, d, other, 5000) == want_other
                assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 0 and gpu_lib.ZSTDMI_debugDictUploadsD(d.dctx) == 0
                d.RefDDict(None)


def test_contexts_and_sets_come_and_go(gpu_lib, ddicts):
    five = [ddicts[name] for name in FIVE]
    recs = records()
    rng = random.Random(5)
    live = []
    for i in range(200):
        live.append(set_context(rng.sample(five, 2 + i % 4)))
        if i % 3 == 2:
            live.pop(rng.randrange(len(live))).Dispose()
    rng.shuffle(live)
    for d in live:
        d.Dispose()
    stream, data = b"".join(f for _, f, _ in recs[:10]), b"".join(x for x, _, _ in recs[:10])
    with set_context(five) as d:
        assert raw_call(gpu_lib, d, stream, len(data)) == (len(data), data) and gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 10
        d.RefDDict(None)
