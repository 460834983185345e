"""GPU tests of content-defined cuts (include/zstd_mi355x.h "Content-defined cuts"): the device's cuts against the numpy restatement of
the rule (tests/content_cuts_cases.py) at the sizes and planted edges where the kernels change path; the bytes of a cut call against the
pieces compressed one by one and against ZSTDMI_compressPack of the pieces; shared frames after an edit; the bound; every refusal; and
that a context with the switch on and off again writes what a fresh one writes."""
import ctypes
import functools
import os

import numpy as np
import pytest

import content_cuts_cases as cc
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = ZSTD_ErrorCode
UNSUPPORTED, TOO_SMALL = E.ZSTD_error_parameter_unsupported, E.ZSTD_error_dstSize_tooSmall
ZSTD_c_windowLog, ZSTD_c_enableLongDistanceMatching, ZSTD_c_checksumFlag = 101, 160, 201


def golden_bytes(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def on_device(data, shift=0):
    """the bytes in device memory, `shift` bytes behind an allocation's start"""
    import torch
    t = torch.empty(len(data) + shift + 8, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return t[shift:shift + len(data)]


def sizes_for(avg_log):
    mn = cc.min_of(avg_log)
    return sorted({0, 1, 63, 64, 65, mn - 1, mn, mn + 1, 16383, 16384, 16385, 65535, 65536, 65537, 200000, 1 << 20})


@functools.lru_cache(maxsize=None)
def want_sizes(kind, n, avg_log):
    return cc.piece_sizes(cc.base(kind)[:n], avg_log)


# ---- the cuts ----
@pytest.mark.parametrize("avg_log", cc.AVG_LOGS)
@pytest.mark.parametrize("kind", ["rand", "text", "zipf", "flat"])
def test_cuts_equal_the_restatement(gpu_lib, kind, avg_log):
    with z.Compressor(1) as c:
        for i, n in enumerate(sizes_for(avg_log)):
            data = cc.base(kind)[:n]
            want = want_sizes(kind, n, avg_log)
            # device memory at every alignment (the mark kernel loads words from an aligned source, bytes otherwise), and host memory
            got = z.content_cuts(c, on_device(data, i % 4), avg_log)
            assert got == want, (kind, avg_log, n, "device", i % 4)
            if n in (0, 65, 65537, 200000):
                assert z.content_cuts(c, data, avg_log) == want, (kind, avg_log, n, "host")


@pytest.mark.parametrize("name", cc.PLANTED)
def test_planted_edges(gpu_lib, name):
    data = cc.planted(name)
    with z.Compressor(1) as c:
        assert z.content_cuts(c, on_device(data), 12) == cc.piece_sizes(data, 12)


def test_chunker_capacity_and_switch_independence(gpu_lib):
    data = cc.base("text")[:100000]
    want = want_sizes("text", 100000, 12)
    with z.Compressor(1) as c:
        c.content_cuts = 16             # (the chunker takes its own avgLog)
        sizes, got = (ctypes.c_size_t * len(want))(*([7] * len(want))), ctypes.c_size_t(0)
        r = gpu_lib.ZSTDMI_contentCuts(c.cctx, data, len(data), 12, sizes, len(want) - 1, ctypes.byref(got))
        assert get_error_code(r) == TOO_SMALL and got.value == len(want) and list(sizes) == [7] * len(want)
        assert gpu_lib.ZSTDMI_contentCuts(c.cctx, data, len(data), 12, sizes, len(want), ctypes.byref(got)) == 0
        assert list(sizes) == want and got.value == len(want)
        assert gpu_lib.ZSTDMI_debugLastContentCuts(c.cctx) == 0         # (no call was cut)


# ---- the bytes ----
def make_compressor(level, dic=None, index=False, checksum=False):
    c = z.Compressor(level)
    if dic is not None:
        c.LoadDictionary(golden_bytes(dic))
    if index:
        c.dict_index = True
    if checksum:
        c.SetParameter(ZSTD_c_checksumFlag, 1)
    return c


def pieces_of(data, avg_log):
    out, at = [], 0
    for s in cc.piece_sizes(data, avg_log):
        out.append(data[at:at + s])
        at += s
    return out


def wrap(c, data, device):
    """Wrap through host buffers, or ZSTDMI_compressDevice over device buffers with a canary behind the capacity"""
    if not device:
        return c.Wrap(data)
    import torch
    lib = z._ffi.load()
    cap = c._wrap_bound(len(data))
    src, dst = on_device(data, 1), torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, src.data_ptr() if len(data) else None, len(data))
    assert not is_error(r), lib.ZSTD_getErrorName(r)
    out = dst.cpu().numpy()
    assert (out[cap:] == 0xA5).all()
    return out[:r].tobytes()


def check_cut_stream(data, avg_log, device, **config):
    pieces = pieces_of(data, avg_log)
    with make_compressor(**config) as fresh:
        want = b"".join(fresh.Wrap(p) for p in pieces)
        pack = z.compress_pack(fresh, pieces)
    with make_compressor(**config) as c:
        c.content_cuts = avg_log
        got = wrap(c, data, device)
        assert z._ffi.load().ZSTDMI_debugLastContentCuts(c.cctx) == len(pieces)
        assert got == want
        c.seek_table = True
        seekable = wrap(c, data, device)
        assert seekable == pack and seekable[:len(want)] == want
    rows, table_bytes = z.read_seek_table(seekable)
    assert table_bytes == len(seekable) - len(want) and sum(d for _, d in rows) == len(data)
    with z.Decompressor() as d:
        if config.get("dic"):
            d.LoadDictionary(golden_bytes(config["dic"]))
        assert d.Unwrap(got, maxDecompressedSize=len(data) + 1) == data
        assert d.Unwrap(seekable, maxDecompressedSize=len(data) + 1) == data
        # single pieces through the table (the first, the last, and every seventh)
        starts = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).tolist()
        pick = sorted(set(range(0, len(pieces), 7)) | {len(pieces) - 1})
        back = d.unwrap_ranges(seekable, [(starts[i], len(pieces[i])) for i in pick])
        assert [bytes(b) for b in back] == [pieces[i] for i in pick]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("avg_log", [12, 16])
@pytest.mark.parametrize("level", [1, 3, 5])
@pytest.mark.parametrize("kind", ["text", "mixed"])
def test_bytes_are_the_pieces_one_by_one(gpu_lib, kind, level, avg_log, device):
    check_cut_stream(cc.base(kind)[:256 << 10], avg_log, device, level=level)


def test_bytes_with_a_dictionary_and_its_index(gpu_lib):
    check_cut_stream(cc.base("text")[:256 << 10], 12, False, level=1, dic="train_default_json.dict", index=True)


def test_bytes_with_a_checksum(gpu_lib):
    check_cut_stream(cc.base("mixed")[:256 << 10], 14, True, level=3, checksum=True)


def test_bytes_with_a_cdict(gpu_lib):
    data = cc.base("text")[:256 << 10]
    pieces = pieces_of(data, 12)
    dic = golden_bytes("train_default_json.dict")
    with z.CDict(dic, 3) as cd:
        with z.Compressor(1) as fresh:
            want = b"".join(fresh.WrapUsingCDict(p, cd) for p in pieces)
            fresh.RefCDict(cd)
            want_ref = b"".join(fresh.Wrap(p) for p in pieces)
        with z.Compressor(1) as c:
            c.content_cuts = 12
            assert c.WrapUsingCDict(data, cd) == want                   # ZSTD_compress_usingCDict
            assert gpu_lib.ZSTDMI_debugLastContentCuts(c.cctx) == len(pieces)
            c.RefCDict(cd)
            assert c.Wrap(data) == want_ref                             # ZSTD_CCtx_refCDict + ZSTD_compress2
    with z.Decompressor() as d:
        d.LoadDictionary(dic)
        assert d.Unwrap(want, maxDecompressedSize=len(data) + 1) == data


def test_empty_source(gpu_lib):
    with z.Compressor(3) as c:
        c.content_cuts = 12
        assert c.Wrap(b"") == b""                                       # an empty source has no piece
        c.seek_table = True
        with z.Compressor(3) as fresh:
            assert c.Wrap(b"") == z.compress_pack(fresh, []) and len(c.Wrap(b"")) == 17     # the pack's empty table
        c.content_cuts = 0
        c.seek_table = False
        assert len(c.Wrap(b"")) > 0                                     # (without the switch: the one empty frame)


# ---- shared frames after an edit ----
def frames_of(lib, blob):
    out, at = [], 0
    buf = ctypes.create_string_buffer(blob, len(blob))
    while at < len(blob):
        n = lib.ZSTD_findFrameCompressedSize(ctypes.addressof(buf) + at, len(blob) - at)
        assert not is_error(n) and n > 0
        out.append(blob[at:at + n])
        at += n
    return out


@pytest.mark.parametrize("kind", ["rand", "text", "zipf"])
def test_streams_of_edited_inputs_share_their_frames(gpu_lib, kind):
    data = cc.base(kind)
    edited = cc.insert_edit(data)
    a, b = cc.piece_sizes(data, 12), cc.piece_sizes(edited, 12)
    ia, ib = cc.resync(a, b)
    assert ia <= 8 and ib <= 8          # (tests/test_content_cuts_cpu.py holds the restatement to this)
    with z.Compressor(1) as c:
        c.content_cuts = 12
        fa, fb = frames_of(gpu_lib, c.Wrap(data)), frames_of(gpu_lib, c.Wrap(edited))
    assert len(fa) == len(a) and len(fb) == len(b)
    assert fa[ia:] == fb[ib:] and len(fa) - ia > 100
    assert fa[:ia] != fb[:ib]


# ---- bound and capacity ----
@pytest.mark.parametrize("kind,avg_log", [("rand", 12), ("text", 14), ("flat", 12)])
def test_bound_suffices_and_one_byte_less_than_needed_does_not(gpu_lib, kind, avg_log):
    import torch
    data = cc.base(kind)[:300000]
    src = on_device(data)
    bound = gpu_lib.ZSTDMI_contentCutsBound(len(data), avg_log)
    with z.Compressor(1) as c:
        c.content_cuts = avg_log
        c.seek_table = True
        dst = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        size = gpu_lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), bound, src.data_ptr(), len(data))
        assert not is_error(size) and size <= bound
        assert (dst[bound:] == 0xA5).all()
        whole = dst[:size].cpu().numpy().tobytes()
        for cap in (size - 1, size - 17, 100, 0):
            dst.fill_(0xA5)
            torch.cuda.synchronize()
            assert get_error_code(gpu_lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, src.data_ptr(), len(data))) == TOO_SMALL, cap
            assert (dst[cap:] == 0xA5).all(), cap
        dst.fill_(0xA5)
        torch.cuda.synchronize()
        assert gpu_lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), size, src.data_ptr(), len(data)) == size
        assert dst[:size].cpu().numpy().tobytes() == whole and (dst[size:] == 0xA5).all()
        # host destination: the same answers
        out = ctypes.create_string_buffer(b"\xA5" * (size + 8), size + 8)
        assert get_error_code(gpu_lib.ZSTD_compress2(c.cctx, out, size - 1, data, len(data))) == TOO_SMALL
        assert out.raw[size - 1:] == b"\xA5" * 9
        assert gpu_lib.ZSTD_compress2(c.cctx, out, size, data, len(data)) == size and out.raw[:size] == whole


# ---- refusals, and the switch off again ----
def test_refusals(gpu_lib):
    import torch
    lib = gpu_lib
    data = cc.base("text")[:100000]
    src = on_device(data)
    cap = lib.ZSTDMI_contentCutsBound(len(data), 12)
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    code = lambda r: get_error_code(r) if is_error(r) else None

    def untouched():
        torch.cuda.synchronize()
        return bool((dst == 0xA5).all())

    with z.Compressor(1) as c:
        c.content_cuts = 12
        one_v, one_s = (ctypes.c_void_p * 1), (ctypes.c_size_t * 1)
        got = one_s()
        # the stream, the batch, the pack, the enqueued calls and their prepares, the sample pass
        out = ctypes.create_string_buffer(1 << 17)
        ob = ZSTD_outBuffer(ctypes.cast(out, ctypes.c_void_p).value, len(out), 0)
        ib = ZSTD_inBuffer(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value, 1000, 0)
        for end_op in (0, 1, 2):
            assert code(lib.ZSTD_compressStream2(c.cctx, ctypes.byref(ob), ctypes.byref(ib), end_op)) == UNSUPPORTED
        assert ib.pos == 0 and ob.pos == 0
        assert code(lib.ZSTDMI_compressBatch(c.cctx, one_v(src.data_ptr()), one_s(1000), 1, one_v(dst.data_ptr()), one_s(2000), got)) == UNSUPPORTED
        cd = z.CDict(golden_bytes("train_default_json.dict"), 1)
        assert code(lib.ZSTDMI_compressBatchCDicts(c.cctx, one_v(src.data_ptr()), one_s(1000), 1, one_v(dst.data_ptr()), one_s(2000), got, one_v(cd.handle))) == UNSUPPORTED
        assert code(lib.ZSTDMI_compressPack(c.cctx, dst.data_ptr(), cap, one_v(src.data_ptr()), one_s(1000), 1)) == UNSUPPORTED
        assert code(lib.ZSTDMI_CCtx_prepareBatchAsync(c.cctx, 4, 4096)) == UNSUPPORTED
        lim = z._ffi.CBatchLimits(4, 100000, 0)
        assert code(lib.ZSTDMI_CCtx_prepareBatchAsyncLimits(c.cctx, ctypes.byref(lim))) == UNSUPPORTED
        c.content_cuts = 0
        assert lib.ZSTDMI_CCtx_prepareBatchAsync(c.cctx, 4, 4096) == 0
        c.content_cuts = 12
        words = torch.zeros(8, dtype=torch.int64, device="cuda")
        w = words.data_ptr()
        assert code(lib.ZSTDMI_compressBatchAsync(c.cctx, w, w + 8, 1, w + 16, w + 24, w + 32)) == UNSUPPORTED
        assert code(lib.ZSTDMI_compressPackAsync(c.cctx, dst.data_ptr(), cap, w, w + 8, 1, w + 16, None)) == UNSUPPORTED
        assert code(lib.ZSTDMI_debugCompressSamples(c.cctx, data, one_s(1000), 1, got)) == UNSUPPORTED
        assert untouched()

        call = lambda: lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, src.data_ptr(), len(data))
        good = call()
        assert not is_error(good)
        dst.fill_(0xA5)
        # several device workers
        assert lib.ZSTDMI_CCtx_setDevices(c.cctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        assert code(call()) == UNSUPPORTED and code(lib.ZSTD_compress2(c.cctx, out, len(out), data, 1000)) == UNSUPPORTED
        assert lib.ZSTDMI_CCtx_setDevices(c.cctx, None, 0) == 0
        # a pending prefix stays pending: refused again, and consumed by the first call with the switch off
        prefix = cc.base("text")[200000:300000]
        c.RefPrefix(prefix)
        assert code(call()) == UNSUPPORTED and code(call()) == UNSUPPORTED
        assert code(lib.ZSTD_compress2(c.cctx, out, len(out), data, 1000)) == UNSUPPORTED
        assert code(lib.ZSTD_compress_usingCDict(c.cctx, out, len(out), data, 1000, cd.handle)) == UNSUPPORTED
        c.content_cuts = 0
        delta = c.Wrap(data)
        with z.Compressor(1) as other:
            other.RefPrefix(prefix)
            assert delta == other.Wrap(data)
            assert delta != other.Wrap(data)        # (the prefix is gone)
        c.content_cuts = 12
        assert call() == good
        dst.fill_(0xA5)
        # one frame per call, long-distance matching, small windows
        c.single_frame = True
        assert code(call()) == UNSUPPORTED
        c.single_frame = False
        c.SetParameter(ZSTD_c_enableLongDistanceMatching, 1)
        assert code(call()) == UNSUPPORTED
        c.SetParameter(ZSTD_c_enableLongDistanceMatching, 0)
        for wlog in (10, 12, 15):
            c.SetParameter(ZSTD_c_windowLog, wlog)
            assert code(call()) == UNSUPPORTED, wlog
        c.SetParameter(ZSTD_c_windowLog, 0)
        assert untouched()
        # a source of 2^32 bytes or more (no byte of it is read)
        assert code(lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, src.data_ptr(), 1 << 32)) == UNSUPPORTED
        assert code(lib.ZSTD_compress2(c.cctx, out, len(out), data, 1 << 32)) == UNSUPPORTED
        assert untouched()
        assert call() == good
        # ZSTD_compressCCtx ignores the switch
        a, b = ctypes.create_string_buffer(len(out)), ctypes.create_string_buffer(len(out))
        with z.Compressor(1) as other:
            na = lib.ZSTD_compressCCtx(c.cctx, a, len(a), data, 50000, 1)
            nb = lib.ZSTD_compressCCtx(other.cctx, b, len(b), data, 50000, 1)
        assert not is_error(na) and na == nb and a.raw[:na] == b.raw[:nb]
        cd.Dispose()


@pytest.mark.parametrize("config", [dict(level=1), dict(level=3), dict(level=5), dict(level=1, dic="train_default_json.dict", index=True)],
                         ids=["level1", "level3", "level5", "dictionary"])
def test_switch_on_and_off_again_writes_what_a_fresh_context_writes(gpu_lib, config):
    data = cc.base("mixed")[:600000]
    with make_compressor(**config) as fresh:
        want, want_small = fresh.Wrap(data), fresh.Wrap(data[:3000])
        fresh.seek_table = True
        want_seek = fresh.Wrap(data)
    with make_compressor(**config) as c:
        c.content_cuts = 12
        assert c.Wrap(data) != want
        c.content_cuts = 0
        assert c.Wrap(data) == want and c.Wrap(data[:3000]) == want_small
        c.seek_table = True
        assert c.Wrap(data) == want_seek
        assert z._ffi.load().ZSTDMI_debugLastContentCuts(c.cctx) == len(cc.piece_sizes(data, 12))      # (still the last call that was cut)
