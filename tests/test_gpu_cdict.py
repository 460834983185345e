"""GPU tests of ZSTD_CDict (include/zstd_mi355x.h "digested dictionaries"): a dictionary digested once, referenced by any number of
contexts and threads, switched without an upload.  The yardstick of every comparison is the same context with ZSTD_c_compressionLevel =
the CDict's level and ZSTD_CCtx_loadDictionary(the same bytes): a referencing context writes exactly its bytes through every entry
point, and ZSTDMI_debugDictUploads shows that it uploaded nothing.  The decoder's side is tests/test_gpu_ddict.py."""
import ctypes
import functools
import io
import os
import threading

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZSTD_c_compressionLevel, ZSTD_c_enableLongDistanceMatching, ZSTD_c_checksumFlag = 100, 160, 201
UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
CORRUPTED = ZSTD_ErrorCode.ZSTD_error_dictionary_corrupted

DICTS = ("rawcontent_6000.dict", "train_default_json.dict", "trained_16k.dict", "7 bytes")
LEVELS = (-5, 1, 3, 5)
# (entropy, index, index strategy, index chain)
SWITCHES = {"none": (0, 0, 1, 0), "entropy": (1, 0, 1, 0), "index": (0, 1, 1, 0), "index+strategy2": (0, 1, 2, 0), "index+chain": (0, 1, 1, 1),
            "all": (1, 1, 2, 1)}


@functools.lru_cache(maxsize=None)
def dictionary(name):
    return b"7 bytes" if name == "7 bytes" else open(os.path.join(GOLDEN, name), "rb").read()


@functools.lru_cache(maxsize=None)
def inputs():
    """0, 1, 300 and 5 000 bytes, and 70 000: a second chunk behind the dictionary"""
    return tuple(datagen.gen("text", n, 60 + i) for i, n in enumerate((0, 1, 300, 5000, 70000)))


def compressor(level, switches="none"):
    """a context at `level` with a switch set — set BEFORE any dictionary, so that the yardstick uploads its dictionary once"""
    e, i, s, ch = SWITCHES[switches]
    c = z.Compressor(level)
    c.dict_entropy, c.dict_index, c.dict_index_strategy, c.dict_index_chain = bool(e), bool(i), s, bool(ch)
    return c


def yardstick(level, dic, switches="none"):
    c = compressor(level, switches)
    c.LoadDictionary(dic)
    return c


def device_call(lib, cctx, data):
    import torch
    room = torch.empty(lib.ZSTD_compressBound(len(data)) + 64, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if data else None
    torch.cuda.synchronize()
    r = lib.ZSTDMI_compressDevice(cctx, room.data_ptr(), lib.ZSTD_compressBound(len(data)), src.data_ptr() if data else None, len(data))
    assert not is_error(r), (len(data), get_error_code(r))
    return room[:r].cpu().numpy().tobytes()


def sample_sizes(lib, cctx, recs):
    recs = [r for r in recs if r]
    sizes = (ctypes.c_size_t * len(recs))(*[len(r) for r in recs])
    out = (ctypes.c_size_t * len(recs))()
    assert lib.ZSTDMI_debugCompressSamples(cctx, b"".join(recs), sizes, len(recs), out) == 0
    return list(out)


def stream_session(c, recs):
    sink = io.BytesIO()
    with z.CompressionStream(sink, compressor=c) as s:
        for r in recs:
            s.Write(r)
    return sink.getvalue()


def code_of(call):
    try:
        call()
    except ZstdException as e:
        return e.code
    return None


# ---------------------------------------------------------------- 1. bytes equal to the loaded dictionary ----------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", DICTS)
def test_single_calls_write_the_loaded_dictionarys_bytes(gpu_lib, name, level):
    """ZSTD_compress2 (twice) and ZSTDMI_compressDevice under every switch set; the context's own level is another one"""
    dic, recs = dictionary(name), inputs()
    with z.CDict(dic, level) as cd:
        assert cd.dict_id == z.get_dict_id_from_dict(dic) and cd.sizeof >= len(dic)
        for sw in SWITCHES:
            with yardstick(level, dic, sw) as y, compressor(9, sw) as c:
                c.RefCDict(cd)
                for r in recs:
                    want = y.Wrap(r)
                    assert c.Wrap(r) == want, (sw, len(r))
                    assert c.Wrap(r) == want, (sw, len(r), "second call")
                    assert device_call(gpu_lib, c.cctx, r) == want, (sw, len(r), "device call")
                assert gpu_lib.ZSTDMI_debugDictIndexed(c.cctx) == gpu_lib.ZSTDMI_debugDictIndexed(y.cctx), sw
                assert gpu_lib.ZSTDMI_debugDictUploads(c.cctx) == 0, sw
                assert c.GetParameter(ZSTD_c_compressionLevel) == 9
                c.RefCDict(None)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", DICTS)
def test_batch_pack_samples_and_stream_write_the_loaded_dictionarys_bytes(gpu_lib, name, level):
    dic, recs = dictionary(name), list(inputs())
    with z.CDict(dic, level) as cd:
        for sw in SWITCHES:
            with yardstick(level, dic, sw) as y, compressor(9, sw) as c:
                c.RefCDict(cd)
                assert z.compress_batch(c, recs) == z.compress_batch(y, recs), sw
                assert z.compress_pack(c, recs) == z.compress_pack(y, recs), sw
                assert sample_sizes(gpu_lib, c.cctx, recs) == sample_sizes(gpu_lib, y.cctx, recs), sw
                assert stream_session(c, recs) == stream_session(y, recs), sw
                assert gpu_lib.ZSTDMI_debugDictUploads(c.cctx) == 0, sw
                c.RefCDict(None)


# ---------------------------------------------------------------- 2. ZSTD_compress_usingCDict ----------------------------------------------------------------
@pytest.mark.parametrize("name", DICTS)
def test_using_cdict_is_one_call_and_leaves_the_context(gpu_lib, name):
    dic, other, recs = dictionary(name), dictionary("rawcontent_6000.dict")[:3000], inputs()
    with z.CDict(dic, 1) as cd, yardstick(1, dic, "all") as y, compressor(9, "all") as c:
        c.SetParameter(ZSTD_c_checksumFlag, 1)
        c.LoadDictionary(other)
        before = [c.Wrap(r) for r in recs]
        for r in recs:
            assert c.WrapUsingCDict(r, cd) == y.Wrap(r), len(r)
        assert [c.Wrap(r) for r in recs] == before
        # a device destination and source, as ZSTD_compress2 takes them
        import torch
        r = recs[3]
        src = torch.from_numpy(np.frombuffer(r, dtype=np.uint8).copy()).cuda()
        room = torch.empty(gpu_lib.ZSTD_compressBound(len(r)), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n = gpu_lib.ZSTD_compress_usingCDict(c.cctx, room.data_ptr(), room.numel(), src.data_ptr(), len(r), cd.handle)
        assert not is_error(n) and room[:n].cpu().numpy().tobytes() == y.Wrap(r)
        # a pending prefix stays pending: the next Wrap consumes it
        with compressor(9, "all") as p:
            p.SetParameter(ZSTD_c_checksumFlag, 1)
            p.RefPrefix(other)
            want = p.Wrap(recs[2])
        c.RefPrefix(other)
        assert c.WrapUsingCDict(recs[2], cd) == y.Wrap(recs[2])
        assert c.Wrap(recs[2]) == want


# ---------------------------------------------------------------- 3. shared and switched ----------------------------------------------------------------
def test_one_cdict_on_two_contexts_and_four_threads(gpu_lib):
    dic, recs = dictionary("trained_16k.dict"), inputs()
    with yardstick(3, dic, "all") as y:
        want = [y.Wrap(r) for r in recs]
        assert gpu_lib.ZSTDMI_debugDictUploads(y.cctx) == 1
    with z.CDict(dic, 3) as cd:
        with compressor(3, "all") as a, compressor(3, "all") as b:
            a.RefCDict(cd)
            b.RefCDict(cd)
            for _ in range(3):
                for i, r in enumerate(recs):
                    assert a.Wrap(r) == want[i] and b.Wrap(r) == want[i]
            assert gpu_lib.ZSTDMI_debugDictUploads(a.cctx) == 0 and gpu_lib.ZSTDMI_debugDictUploads(b.cctx) == 0
            a.RefCDict(None)
            b.RefCDict(None)
        got, uploads = [None] * 4, [None] * 4

        def work(k):
            with compressor(3, "all") as c:
                c.RefCDict(cd)
                got[k] = [[c.Wrap(r) for r in recs] for _ in range(4)]
                uploads[k] = gpu_lib.ZSTDMI_debugDictUploads(c.cctx)
                c.RefCDict(None)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert got == [[want] * 4] * 4 and uploads == [0] * 4


def test_two_cdicts_alternated_and_the_level_that_counts(gpu_lib):
    d1, d2, recs = dictionary("trained_16k.dict"), dictionary("train_default_json.dict"), inputs()[1:4]
    with yardstick(1, d1, "all") as y1, yardstick(5, d2, "all") as y2, compressor(3, "all") as plain:
        w1, w2, w0 = [y1.Wrap(r) for r in recs], [y2.Wrap(r) for r in recs], [plain.Wrap(r) for r in recs]
    with z.CDict(d1, 1) as c1, z.CDict(d2, 5) as c2, compressor(3, "all") as c:
        for _ in range(10):
            c.RefCDict(c1)
            assert [c.Wrap(r) for r in recs] == w1
            c.RefCDict(c2)
            assert [c.Wrap(r) for r in recs] == w2
        assert gpu_lib.ZSTDMI_debugDictUploads(c.cctx) == 0
        # the context's level is ignored while a CDict is in force ...
        c.Level = 12
        assert [c.Wrap(r) for r in recs] == w2 and c.GetParameter(ZSTD_c_compressionLevel) == 12
        # ... and counts again afterwards
        c.Level = 3
        c.RefCDict(None)
        assert [c.Wrap(r) for r in recs] == w0


# ---------------------------------------------------------------- 4. precedence ----------------------------------------------------------------
def test_precedence_of_load_reference_and_prefix(gpu_lib):
    # (d2: raw content that holds a part of each record, so that it changes what is written for both)
    d1, d2, recs = dictionary("trained_16k.dict"), inputs()[3][1000:4000] + inputs()[2], inputs()[2:4]
    with yardstick(3, d1) as y1, yardstick(3, d2) as y2, compressor(3) as plain:
        w1, w2, w0 = [y1.Wrap(r) for r in recs], [y2.Wrap(r) for r in recs], [plain.Wrap(r) for r in recs]
        plain.RefPrefix(d2)
        wp = plain.Wrap(recs[0])
        assert w1 != w0 and w2 != w0 and wp != w0[0]
    with z.CDict(d1, 3) as cd, compressor(3) as c:
        c.RefCDict(cd)
        c.LoadDictionary(d2)                            # the later call wins
        assert [c.Wrap(r) for r in recs] == w2
        c.RefCDict(cd)
        assert [c.Wrap(r) for r in recs] == w1
        c.LoadDictionary(None)                          # NULL included
        assert [c.Wrap(r) for r in recs] == w0
        c.RefPrefix(d2)
        c.RefCDict(cd)                                  # cancels the pending prefix
        assert [c.Wrap(r) for r in recs] == w1
        c.RefPrefix(d2)                                 # the next call ignores the CDict, the one after it has no dictionary
        assert c.Wrap(recs[0]) == wp
        assert [c.Wrap(r) for r in recs] == w0
        c.RefCDict(cd)
        out = ctypes.create_string_buffer(gpu_lib.ZSTD_compressBound(len(recs[1])))
        n = gpu_lib.ZSTD_compressCCtx(c.cctx, out, len(out), recs[1], len(recs[1]), 3)
        assert not is_error(n) and out.raw[:n] == w0[1]         # ZSTD_compressCCtx ignores the reference
        assert [c.Wrap(r) for r in recs] == w1
        c.RefCDict(None)


@pytest.mark.parametrize("name", ["rawcontent_6000.dict", "trained_16k.dict"])
def test_what_a_loaded_dictionary_is_refused_stays_refused(gpu_lib, name):
    dic, big = dictionary(name), inputs()[4]
    with z.CDict(dic, 3) as cd, compressor(3) as c, yardstick(3, dic) as y:
        c.RefCDict(cd)
        for ctx in (c, y):
            ctx.SetParameter(ZSTD_c_enableLongDistanceMatching, 1)
        assert code_of(lambda: y.Wrap(big)) == UNSUPPORTED and code_of(lambda: c.Wrap(big)) == UNSUPPORTED     # LDM above one block
        assert c.Wrap(inputs()[3]) == y.Wrap(inputs()[3])
        for ctx in (c, y):
            ctx.SetParameter(ZSTD_c_enableLongDistanceMatching, 0)
            ctx.single_frame = True
        assert code_of(lambda: y.Wrap(big)) == UNSUPPORTED and code_of(lambda: c.Wrap(big)) == UNSUPPORTED     # one frame above 64 KiB
        assert c.Wrap(inputs()[3]) == y.Wrap(inputs()[3])
        c.RefCDict(None)


# ---------------------------------------------------------------- 5. where the digest cannot be shared ----------------------------------------------------------------
def test_device_workers_make_a_private_upload(gpu_lib):
    dic, recs = dictionary("trained_16k.dict"), inputs()
    with yardstick(3, dic, "all") as y:
        want = [y.Wrap(r) for r in recs]
    arr = (ctypes.c_int * 2)(0, 0)
    with z.CDict(dic, 3) as cd, compressor(9, "all") as c:
        c.RefCDict(cd)
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, arr, 2) == 0
        assert [c.Wrap(r) for r in recs] == want
        assert gpu_lib.ZSTDMI_debugDictUploads(c.cctx) > 0
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, arr, 1) == 0         # back to one device: shared again
        before = gpu_lib.ZSTDMI_debugDictUploads(c.cctx)
        assert [c.Wrap(r) for r in recs] == want
        assert gpu_lib.ZSTDMI_debugDictUploads(c.cctx) == before
        c.RefCDict(None)
    with z.CDict(dic, 3) as cd, compressor(9, "all") as c:      # the other order: the workers first
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, arr, 2) == 0
        c.RefCDict(cd)
        assert [c.Wrap(r) for r in recs] == want and gpu_lib.ZSTDMI_debugDictUploads(c.cctx) > 0
        c.RefCDict(None)
    with z.CDict(dic, 3) as cd, yardstick(3, dic, "all") as y2, compressor(9, "all") as c:
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, arr, 2) == 0
        c.LoadDictionary(dictionary("rawcontent_6000.dict"))
        before = [c.Wrap(r) for r in recs]
        assert [c.WrapUsingCDict(r, cd) for r in recs] == [y2.Wrap(r) for r in recs]
        assert [c.Wrap(r) for r in recs] == before


# ---------------------------------------------------------------- 6. refusals ----------------------------------------------------------------
def damaged_dictionaries():
    """trained_16k.dict with a truncated header, and with a damaged NCount (the offset-code table's accuracy log above its maximum)"""
    good = dictionary("trained_16k.dict")
    # the Huffman table's header byte says how long its description is; the offset-code NCount follows it
    hb = good[8]
    of_at = 8 + 1 + (hb if hb < 128 else (hb - 127 + 1) // 2)
    broken = bytearray(good)
    broken[of_at] = (broken[of_at] & 0xF0) | 0x0F        # accuracy log 5 + 15 = 20: above every table's maximum
    return {"truncated header": good[:40], "damaged NCount": bytes(broken)}


def test_a_dictionary_that_is_refused_never_becomes_a_digest(gpu_lib):
    for what, dic in damaged_dictionaries().items():
        assert not gpu_lib.ZSTD_createCDict(dic, len(dic), 3), what
        assert not gpu_lib.ZSTD_createDDict(dic, len(dic)), what
        with pytest.raises(ValueError):
            z.CDict(dic)
        with pytest.raises(ValueError):
            z.DDict(dic)
        with z.Compressor(3) as c, z.Decompressor() as d:
            assert code_of(lambda: c.LoadDictionary(dic)) == CORRUPTED, what
            assert code_of(lambda: d.LoadDictionary(dic)) == CORRUPTED, what


# ---------------------------------------------------------------- 8. lifetime ----------------------------------------------------------------
def test_contexts_and_digests_come_and_go(gpu_lib):
    dic, recs = dictionary("trained_16k.dict"), inputs()[1:4]
    with yardstick(3, dic, "all") as y:
        want = [y.Wrap(r) for r in recs]
    for _ in range(3):
        cd = z.CDict(dic, 3)
        c = compressor(3, "all")
        c.RefCDict(cd)
        assert [c.Wrap(r) for r in recs] == want
        c.Dispose()                 # the context first, then its CDict
        cd.Dispose()
    import torch
    dev = torch.from_numpy(np.frombuffer(dic, dtype=np.uint8).copy()).cuda()       # device memory in: the bytes are copied
    torch.cuda.synchronize()
    h = gpu_lib.ZSTD_createCDict(dev.data_ptr(), dev.numel(), 0)                   # level 0 means 3
    assert h
    del dev
    with compressor(9, "all") as c:
        assert gpu_lib.ZSTD_CCtx_refCDict(c.cctx, h) == 0
        assert [c.Wrap(r) for r in recs] == want
        assert gpu_lib.ZSTD_CCtx_refCDict(c.cctx, None) == 0
    assert gpu_lib.ZSTD_sizeof_CDict(h) > len(dic) and gpu_lib.ZSTD_freeCDict(h) == 0
    on0 = gpu_lib.ZSTDMI_createCDictOnDevice(dic, len(dic), 3, 0)
    assert on0 and gpu_lib.ZSTD_freeCDict(on0) == 0
    assert not gpu_lib.ZSTDMI_createCDictOnDevice(dic, len(dic), 3, gpu_lib.ZSTDMI_deviceCount())      # no such device
