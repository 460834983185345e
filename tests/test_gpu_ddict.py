"""GPU tests of ZSTD_DDict (include/zstd_mi355x.h "digested dictionaries").  The yardstick is a context after ZSTD_DCtx_loadDictionary(the
same bytes): a context that references a DDict returns the same bytes and the same values — error codes included — from every decode
entry point, uploads nothing (ZSTDMI_debugDictUploadsD), and takes the sequence tables of every block that repeats the dictionary's from
the DDict's ready-made set (ZSTDMI_debugLastDictTableBlocks; seq_decode_kernel's instance for it, decode_seq.hip).  The frames: the
libzstd-made dict_fmt_* / dict_raw_* goldens and this compressor's own, with ZSTDMI_CCtx_setDictEntropy on (their first blocks repeat
the dictionary's tables) and off."""
import ctypes
import functools
import io
import os
import struct

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

from test_gpu_dict_entropy import any_repeat, blocks_of, frames_of, parse_block

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DICTS = ("rawcontent_6000.dict", "train_default_json.dict", "trained_16k.dict", "7 bytes")


@functools.lru_cache(maxsize=None)
def dictionary(name):
    return b"7 bytes" if name == "7 bytes" else open(os.path.join(GOLDEN, name), "rb").read()


@functools.lru_cache(maxsize=None)
def own_frames(name):
    """[(content, stream)] of this compressor behind the dictionary: 0, 1, 300, 5 000 and 70 000 bytes at levels 1 and 3, with the
    dictionary's entropy tables on and off (and the index on for half of them)"""
    out = []
    recs = [datagen.gen("text", n, 60 + i) for i, n in enumerate((0, 1, 300, 5000, 70000))]
    for level in (1, 3):
        for entropy in (True, False):
            with z.Compressor(level) as c:
                c.dict_entropy, c.dict_index = entropy, level == 1
                c.LoadDictionary(dictionary(name))
                out += [(r, c.Wrap(r)) for r in recs]
    return tuple(out)


def golden_frames(golden_dict, name):
    return [(None, c["blob"], c["n"]) for c in golden_dict if c.get("dict") == name]


def cases(golden_dict, name):
    """[(stream, content size)]"""
    return [(blob, n) for _, blob, n in golden_frames(golden_dict, name)] + [(s, len(r)) for r, s in own_frames(name)]


def repeat_blocks(stream, oracle):
    """compressed blocks of a stream of one-block frames that have sequences and at least one repeat-mode table"""
    n = 0
    for f in frames_of(stream, oracle):
        blocks = blocks_of(f)
        assert len(blocks) == 1             # (behind a dictionary this compressor's frames have one block: "repeat" means the dictionary's)
        btype, body = blocks[0]
        if btype == 2:
            _, nb_seq, modes = parse_block(body)
            n += bool(nb_seq) and any_repeat(modes)
    return n


def raw_call(lib, d, blob, room, ddict=None):
    """-> (return value, bytes) of ZSTD_decompressDCtx / ZSTD_decompress_usingDDict on host buffers"""
    out = ctypes.create_string_buffer(max(room, 1))
    r = lib.ZSTD_decompressDCtx(d.dctx, out, room, blob, len(blob)) if ddict is None else \
        lib.ZSTD_decompress_usingDDict(d.dctx, out, room, blob, len(blob), ddict.handle)
    return r, (b"" if is_error(r) else out.raw[:r])


def device_call(lib, d, blob, room):
    import torch
    src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    out = torch.empty(max(room, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), room, src.data_ptr(), len(blob))
    return r, (b"" if is_error(r) else out[:r].cpu().numpy().tobytes())


def loaded(dic, mode=0):
    d = z.Decompressor()
    d.LoadDictionary(dic)
    assert d._lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, mode) == 0
    return d


def referencing(dd, mode=0):
    d = z.Decompressor()
    d.RefDDict(dd)
    assert d._lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, mode) == 0
    return d


# ---------------------------------------------------------------- the same bytes and values ----------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("name", DICTS)
def test_single_calls_equal_the_loaded_dictionary(gpu_lib, golden_dict, oracle, name, mode):
    dic = dictionary(name)
    with z.DDict(dic) as dd, loaded(dic, mode) as y, referencing(dd, mode) as d, z.Decompressor() as u:
        assert dd.dict_id == z.get_dict_id_from_dict(dic) and dd.sizeof >= len(dic)
        assert gpu_lib.ZSTDMI_DCtx_setLiteralDecoder(u.dctx, mode) == 0
        u.LoadDictionary(dictionary("rawcontent_6000.dict")[:2000])         # (what ZSTD_decompress_usingDDict must leave alone)
        for blob, n in cases(golden_dict, name):
            want = raw_call(gpu_lib, y, blob, n)
            assert not is_error(want[0]) and want[0] == n
            assert gpu_lib.ZSTDMI_debugLastDictTableBlocks(y.dctx) == 0
            assert raw_call(gpu_lib, d, blob, n) == want, n
            assert device_call(gpu_lib, d, blob, n) == want, n
            assert raw_call(gpu_lib, u, blob, n, dd) == want, n
            small = raw_call(gpu_lib, y, blob, n - 1) if n else None
            assert small is None or raw_call(gpu_lib, d, blob, n - 1) == small
        assert gpu_lib.ZSTDMI_debugDictUploadsD(d.dctx) == 0 and gpu_lib.ZSTDMI_debugDictUploadsD(u.dctx) <= 1
        assert gpu_lib.ZSTDMI_debugDictUploadsD(y.dctx) == 1
        d.RefDDict(None)


@pytest.mark.parametrize("name", DICTS)
def test_batch_range_and_stream_equal_the_loaded_dictionary(gpu_lib, golden_dict, oracle, name):
    dic = dictionary(name)
    cs = [c for c in cases(golden_dict, name) if c[1]]
    with z.DDict(dic) as dd, loaded(dic) as y, referencing(dd) as d:
        # ZSTDMI_decompressBatch
        want = z.decompress_batch(y, [b for b, _ in cs], [n for _, n in cs])
        assert z.decompress_batch(d, [b for b, _ in cs], [n for _, n in cs]) == want
        # ZSTDMI_decompressRange(s) on a pack written behind the dictionary
        recs = [r for r, _ in own_frames(name)[:5]]
        with z.Compressor(1) as c:
            c.dict_entropy = True
            c.LoadDictionary(dic)
            pack = z.compress_pack(c, recs)
        total = sum(len(r) for r in recs)
        for off, length in ((0, total), (5000, 3000), (total - 70000, 70000), (0, 1)):
            w = y.unwrap_range(pack, off, length)
            assert w == b"".join(recs)[off:off + length] and d.unwrap_range(pack, off, length) == w
        assert d.unwrap_ranges(pack, z.pack_ranges([len(r) for r in recs])) == recs
        # ZSTD_decompressStream, whole frames and a segment per block
        for blob, n in cs:
            for segment in (0, 1):
                w = z.DecompressionStream(io.BytesIO(blob), decompressor=y, segment=segment).ReadToEnd()
                assert len(w) == n and z.DecompressionStream(io.BytesIO(blob), decompressor=d, segment=segment).ReadToEnd() == w, (n, segment)
        assert gpu_lib.ZSTDMI_debugDictUploadsD(d.dctx) == 0
        d.RefDDict(None)


# ---------------------------------------------------------------- the ready-made tables ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["train_default_json.dict", "trained_16k.dict"])
def test_blocks_that_repeat_the_dictionary_copy_its_tables(gpu_lib, oracle, name):
    dic = dictionary(name)
    frames = own_frames(name)
    expect = [repeat_blocks(s, oracle) for _, s in frames]
    assert sum(expect) >= 4, expect                                 # (the entropy-on records do repeat the dictionary's tables)
    with z.DDict(dic) as dd, referencing(dd) as d, loaded(dic) as y:
        for (r, s), k in zip(frames, expect):
            assert raw_call(gpu_lib, d, s, len(r)) == (len(r), r)
            assert gpu_lib.ZSTDMI_debugLastDictTableBlocks(d.dctx) == k, (len(r), k)
            assert raw_call(gpu_lib, y, s, len(r)) == (len(r), r)
            assert gpu_lib.ZSTDMI_debugLastDictTableBlocks(y.dctx) == 0
        full = [(r, s) for r, s in frames if r]                     # (an empty frame has no compressed block)
        back = z.decompress_batch(d, [s for _, s in full], [len(r) for r, _ in full])
        assert back == [r for r, _ in full] and gpu_lib.ZSTDMI_debugLastDictTableBlocks(d.dctx) == sum(expect)
        d.RefDDict(None)
    raw = dictionary("rawcontent_6000.dict")
    with z.DDict(raw) as dd, referencing(dd) as d:
        for r, s in own_frames("rawcontent_6000.dict"):
            assert raw_call(gpu_lib, d, s, len(r)) == (len(r), r)
            assert gpu_lib.ZSTDMI_debugLastDictTableBlocks(d.dctx) == 0
        d.RefDDict(None)


def test_damaged_frames_give_the_loaded_dictionarys_errors(gpu_lib, oracle):
    dic = dictionary("trained_16k.dict")
    r, s = next((r, s) for r, s in own_frames("trained_16k.dict") if len(r) == 5000 and repeat_blocks(s, oracle) == 1)
    flipped = bytearray(s)
    flipped[-3] ^= 0x10                     # a bit in the sequence bitstream, which ends the block
    damaged = {"bit flip": bytes(flipped), "truncated": s[:-5], "truncated to the header": s[:9]}
    with z.DDict(dic) as dd, referencing(dd) as d, loaded(dic) as y:
        for what, blob in damaged.items():
            want = raw_call(gpu_lib, y, blob, len(r))
            got = raw_call(gpu_lib, d, blob, len(r))
            print(what, "->", get_error_code(want[0]) if is_error(want[0]) else want[0])
            assert got == want and raw_call(gpu_lib, y, blob, len(r), dd) == want, what
        assert is_error(raw_call(gpu_lib, y, damaged["truncated"], len(r))[0])
        d.RefDDict(None)


def test_a_foreign_dict_id_is_dictionary_wrong(gpu_lib, golden_dict):
    t16, js = dictionary("trained_16k.dict"), dictionary("train_default_json.dict")
    assert z.get_dict_id_from_dict(t16) != z.get_dict_id_from_dict(js)
    wrong = ZSTD_ErrorCode.ZSTD_error_dictionary_wrong
    blob, n = cases(golden_dict, "trained_16k.dict")[2]
    assert z.get_dict_id_from_frame(blob) == z.get_dict_id_from_dict(t16)
    with z.DDict(js) as dd, referencing(dd) as d, loaded(js) as y, z.Decompressor() as u:
        want = raw_call(gpu_lib, y, blob, n)
        assert is_error(want[0]) and get_error_code(want[0]) == wrong
        assert raw_call(gpu_lib, d, blob, n) == want and raw_call(gpu_lib, u, blob, n, dd) == want
        d.RefDDict(None)


# ---------------------------------------------------------------- precedence, fallback, lifetime ----------------------------------------------------------------
def test_precedence_of_load_reference_and_prefix(gpu_lib, golden_dict):
    t16, raw = dictionary("trained_16k.dict"), dictionary("rawcontent_6000.dict")
    fb, fn = cases(golden_dict, "trained_16k.dict")[1]
    rb, rn = cases(golden_dict, "rawcontent_6000.dict")[0]
    with loaded(t16) as y1, loaded(raw) as y2:
        wf, wr = raw_call(gpu_lib, y1, fb, fn), raw_call(gpu_lib, y2, rb, rn)
        cross = raw_call(gpu_lib, y2, fb, fn)                       # the formatted frame behind the raw dictionary: refused or other bytes
        assert not is_error(wf[0]) and not is_error(wr[0]) and cross != wf
    with z.DDict(t16) as dd, z.Decompressor() as d, z.Decompressor() as none:
        d.RefDDict(dd)
        d.LoadDictionary(raw)                                       # the later call wins
        assert raw_call(gpu_lib, d, rb, rn) == wr and raw_call(gpu_lib, d, fb, fn) == cross
        d.RefDDict(dd)
        assert raw_call(gpu_lib, d, fb, fn) == wf
        d.RefPrefix(raw)                                            # cancels the DDict: this call decodes behind the prefix, the next one behind nothing
        assert raw_call(gpu_lib, d, rb, rn) == wr
        assert raw_call(gpu_lib, d, fb, fn) == raw_call(gpu_lib, none, fb, fn)
        d.RefPrefix(raw)
        d.RefDDict(dd)                                              # cancels the pending prefix
        assert raw_call(gpu_lib, d, fb, fn) == wf
        d.RefDDict(None)
        assert raw_call(gpu_lib, d, fb, fn) == raw_call(gpu_lib, none, fb, fn)


def test_device_workers_make_a_private_upload(gpu_lib, golden_dict):
    dic = dictionary("trained_16k.dict")
    cs = cases(golden_dict, "trained_16k.dict")
    arr = (ctypes.c_int * 2)(0, 0)
    with z.DDict(dic) as dd, loaded(dic) as y, referencing(dd) as d:
        assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, arr, 2) == 0
        for blob, n in cs:
            assert raw_call(gpu_lib, d, blob, n) == raw_call(gpu_lib, y, blob, n), n
        assert gpu_lib.ZSTDMI_debugDictUploadsD(d.dctx) > 0 and gpu_lib.ZSTDMI_debugLastDictTableBlocks(d.dctx) == 0
        d.RefDDict(None)


def test_contexts_and_digests_come_and_go(gpu_lib, golden_dict):
    dic = dictionary("trained_16k.dict")
    blob, n = cases(golden_dict, "trained_16k.dict")[3]
    with loaded(dic) as y:
        want = raw_call(gpu_lib, y, blob, n)
    for _ in range(3):
        dd = z.DDict(dic)
        d = referencing(dd)
        assert raw_call(gpu_lib, d, blob, n) == want
        d.Dispose()                 # the context first, then its DDict
        dd.Dispose()
    import torch
    dev = torch.from_numpy(np.frombuffer(dic, dtype=np.uint8).copy()).cuda()       # device memory in: the bytes are copied
    torch.cuda.synchronize()
    h = gpu_lib.ZSTD_createDDict(dev.data_ptr(), dev.numel())
    assert h and gpu_lib.ZSTD_getDictID_fromDDict(h) == struct.unpack_from("<I", dic, 4)[0]
    del dev
    with z.Decompressor() as d:
        assert gpu_lib.ZSTD_DCtx_refDDict(d.dctx, h) == 0
        assert raw_call(gpu_lib, d, blob, n) == want
        assert gpu_lib.ZSTD_DCtx_refDDict(d.dctx, None) == 0
    assert gpu_lib.ZSTD_sizeof_DDict(h) > len(dic) and gpu_lib.ZSTD_freeDDict(h) == 0
    assert not gpu_lib.ZSTDMI_createDDictOnDevice(dic, len(dic), gpu_lib.ZSTDMI_deviceCount())     # no such device
