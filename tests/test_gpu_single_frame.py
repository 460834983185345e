"""GPU tests of ZSTDMI_CCtx_setSingleFrame: a call of more than 64 KiB, and a stream session, is exactly ONE zstd frame —
with the header the reference writes, Last_Block on the last block only, one checksum over the whole content — whose bytes do not
depend on how the call is cut into passes; a context that leaves the switch off writes what it wrote before.  Everything goes through
the C ABI; every stream is decoded by the oracle's decoder and by the GPU decoder in both long-frame modes."""
import ctypes
import functools
import io

import pytest

import datagen
import oracle_lib
import zstdsharp_amd as z
from zstdsharp_amd.compressor import ZSTD_c_enableLongDistanceMatching as ZSTD_c_ldm
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer, ZSTD_e_continue, ZSTD_e_end, ZSTD_e_flush

pytestmark = pytest.mark.gpu

ZSTD_c_windowLog, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 101, 200, 201
KiB, MiB = 1 << 10, 1 << 20
UNKNOWN = (1 << 64) - 1             # ZSTD_CONTENTSIZE_UNKNOWN
UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_parameter_unsupported
CB = {-1: 64 * KiB, 1: 64 * KiB, 3: 48 * KiB, 5: 32 * KiB, 9: 32 * KiB}      # block size of the level's single-frame framing
KINDS = {"text": "text", "zipf": "zipf", "mixed": "mixed", "runs": "runs", "zeros": "zeros", "random": "rand"}


@functools.lru_cache(maxsize=None)
def corpus(kind, n=3 * MiB + 7):
    """one buffer per kind, made once; the tests take prefixes of it"""
    return datagen.gen(KINDS[kind], n, 11)


def new_cctx(lib, level, single=None, params=None, pass_chunks=None):
    c = lib.ZSTD_createCCtx()
    assert not is_error(lib.ZSTD_CCtx_setParameter(c, 100, level))
    for k, v in (params or {}).items():
        assert not is_error(lib.ZSTD_CCtx_setParameter(c, k, v)), (k, v)
    if single is not None:
        assert lib.ZSTDMI_CCtx_setSingleFrame(c, single) == 0
    if pass_chunks:
        assert lib.ZSTDMI_CCtx_setPassChunks(c, pass_chunks) == 0
    return c


def compress2(lib, c, data):
    """ZSTD_compress2 -> bytes, or the negative error code"""
    cap = lib.ZSTD_compressBound(len(data))
    out = ctypes.create_string_buffer(max(cap, 1))
    r = lib.ZSTD_compress2(c, out, cap, data, len(data))
    return -get_error_code(r) if is_error(r) else out.raw[:r]


def compress(lib, level, data, single=None, params=None, pass_chunks=None):
    c = new_cctx(lib, level, single, params, pass_chunks)
    try:
        return compress2(lib, c, data)
    finally:
        lib.ZSTD_freeCCtx(c)


def is_one_frame(lib, blob):
    return lib.ZSTD_findFrameCompressedSize(blob, len(blob)) == len(blob)


def decodes_everywhere(lib, blob, data):
    # (Unwrap sizes its buffer from the header; a frame without a content size makes it ask for the frame's upper bound)
    assert oracle_lib.decompress(blob, len(data)) == data, "the oracle's decoder must restore the input"
    for mode in (1, 2):
        with z.Decompressor() as d:
            assert lib.ZSTDMI_DCtx_setLongFrames(d.dctx, mode) == 0
            assert d.Unwrap(blob, maxDecompressedSize=1 << 30) == data, f"the GPU decoder (long frames {mode}) must restore the input"


# ---- 1. shape and round trip ----
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("level", [-1, 1, 3, 5, 9])
def test_one_frame_holds_the_whole_input(gpu_lib, level, kind):
    lib, cb = gpu_lib, CB[level]
    for n in (64 * KiB + 1, 2 * cb, 2 * cb + 1, 300000, MiB + 12345):
        data = corpus(kind)[:n]
        blob = compress(lib, level, data, single=1)
        assert isinstance(blob, bytes), (n, blob)
        assert is_one_frame(lib, blob), f"n = {n}: more than one frame (or none)"
        assert lib.ZSTD_getFrameContentSize(blob, len(blob)) == n
        assert len(blob) <= lib.ZSTD_compressBound(n)
        decodes_everywhere(lib, blob, data)


# ---- 2. the bytes do not depend on the passes; one checksum over the whole content ----
@pytest.mark.parametrize("checksum", [0, 1])
@pytest.mark.parametrize("kind", ["text", "mixed"])
@pytest.mark.parametrize("level", [1, 3, 5])
def test_bytes_do_not_depend_on_the_pass_size(gpu_lib, level, kind, checksum):
    lib = gpu_lib
    for n in (4 * CB[level] + 1, 3 * MiB + 7):
        data = corpus(kind)[:n]
        params = {ZSTD_c_checksumFlag: checksum}
        whole = compress(lib, level, data, single=1, params=params)
        assert isinstance(whole, bytes) and is_one_frame(lib, whole)
        for chunks in (4, 5):
            assert compress(lib, level, data, single=1, params=params, pass_chunks=chunks) == whole, f"n = {n}, {chunks} chunks per pass"
        decodes_everywhere(lib, whole, data)        # (with the checksum flag set, both decoders verify it)
        if checksum:
            assert whole[4] & 4
            # the frame of a copy with one content byte flipped, under the original's checksum
            other = bytearray(data); other[n // 2] ^= 0x10
            forged = compress(lib, level, bytes(other), single=1, params=params, pass_chunks=4)[:-4] + whole[-4:]
            assert oracle_lib.decompress(forged, n) == -ZSTD_ErrorCode.ZSTD_error_checksum_wrong
            with z.Decompressor() as d, pytest.raises(ZstdException) as e:
                d.Unwrap(forged, maxDecompressedSize=n)
            assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_checksum_wrong


# ---- 3. header forms ----
def stream_decode(lib, blob, segment):
    """ZSTD_decompressStream with ZSTDMI_DCtx_setStreamSegment -> bytes, or the negative error code"""
    d = lib.ZSTD_createDCtx()
    try:
        assert lib.ZSTDMI_DCtx_setStreamSegment(d, segment) == 0
        src = ctypes.create_string_buffer(blob, len(blob))
        inb = ZSTD_inBuffer(ctypes.addressof(src), len(blob), 0)
        out, room = bytearray(), ctypes.create_string_buffer(2 * MiB)
        while True:
            ob = ZSTD_outBuffer(ctypes.addressof(room), 2 * MiB, 0)
            r = lib.ZSTD_decompressStream(d, ctypes.byref(ob), ctypes.byref(inb))
            if is_error(r):
                return -get_error_code(r)
            out += room.raw[:ob.pos]
            if r == 0 and inb.pos == inb.size:
                return bytes(out)
            assert ob.pos or inb.pos < inb.size or r, "no progress"
    finally:
        lib.ZSTD_freeDCtx(d)


def test_window_descriptor_beside_the_content_size(gpu_lib):
    """srcSize above 2^windowLog: a descriptor for exactly that window AND the content size; the segmented stream decoder refuses an
    offset beyond the declared window, so decoding there shows that no match reaches further than the header says"""
    lib, n = gpu_lib, MiB
    data = corpus("text")[:n]
    blob = compress(lib, 1, data, single=1, params={ZSTD_c_windowLog: 18})
    assert is_one_frame(lib, blob)
    assert blob[4] == 0x80, "FHD: a 4-byte content size, no single segment, no checksum, no dictID"
    assert blob[5] == (18 - 10) << 3
    assert int.from_bytes(blob[6:10], "little") == n and lib.ZSTD_getFrameContentSize(blob, len(blob)) == n
    assert stream_decode(lib, blob, 1) == data
    decodes_everywhere(lib, blob, data)


def test_level_window_single_segment_and_no_content_size(gpu_lib):
    lib = gpu_lib
    data = corpus("text")[:200000]
    blob = compress(lib, 3, data, single=1)
    assert is_one_frame(lib, blob) and blob[4] & 0x20, "200 000 bytes fit level 3's window: a single segment"
    assert lib.ZSTD_getFrameContentSize(blob, len(blob)) == 200000
    # the level's own window: level 1 resolves to 2^19 for 1 MiB + 12345 bytes
    big = corpus("text")[:MiB + 12345]
    blob = compress(lib, 1, big, single=1)
    assert blob[4] == 0x80 and blob[5] == (19 - 10) << 3 and int.from_bytes(blob[6:10], "little") == len(big)
    for level, n in ((3, 200000), (1, MiB + 12345)):
        data = corpus("text")[:n]
        blob = compress(lib, level, data, single=1, params={ZSTD_c_contentSizeFlag: 0})
        assert is_one_frame(lib, blob)
        assert blob[4] == 0 and blob[5] >> 3 >= 8, "a window descriptor alone"
        assert (1 << (10 + (blob[5] >> 3))) >= min(n, 1 << 19)
        assert lib.ZSTD_getFrameContentSize(blob, len(blob)) == UNKNOWN
        decodes_everywhere(lib, blob, data)


# ---- 4. nothing else moves ----
@pytest.mark.parametrize("level", [1, 3, 5])
def test_switch_off_writes_the_same_bytes(gpu_lib, level):
    lib = gpu_lib
    for n in (0, 1, 65536, MiB):
        data = corpus("text")[:n]
        fresh = compress(lib, level, data)
        assert isinstance(fresh, bytes)
        assert compress(lib, level, data, single=0) == fresh
        c = new_cctx(lib, level, single=1)
        assert lib.ZSTDMI_CCtx_setSingleFrame(c, 0) == 0
        assert compress2(lib, c, data) == fresh, "switched on, then off"
        lib.ZSTD_freeCCtx(c)
        if n <= 65536:
            assert compress(lib, level, data, single=1) == fresh, "at most 64 KiB: the bytes of the switch off"
        else:
            assert not is_one_frame(lib, fresh) and is_one_frame(lib, compress(lib, level, data, single=1))


def test_compressCCtx_and_refPrefix_ignore_the_switch(gpu_lib):
    lib = gpu_lib
    data = corpus("text")[:300000]
    outs = []
    for single in (0, 1):
        c = new_cctx(lib, 5, single=single)
        cap = lib.ZSTD_compressBound(len(data))
        out = ctypes.create_string_buffer(cap)
        r = lib.ZSTD_compressCCtx(c, out, cap, data, len(data), 3)
        assert not is_error(r)
        prefix = corpus("text")[MiB:MiB + 200000]
        assert lib.ZSTD_CCtx_refPrefix(c, prefix, len(prefix)) == 0
        outs.append((out.raw[:r], compress2(lib, c, data)))
        lib.ZSTD_freeCCtx(c)
    assert outs[0] == outs[1]
    assert not is_one_frame(lib, outs[0][0]) and is_one_frame(lib, outs[0][1])


# ---- 5. refusals ----
def test_what_one_frame_cannot_be_is_refused_and_the_context_stays_usable(gpu_lib):
    lib = gpu_lib
    data = corpus("text")[:300000]
    good = compress(lib, 3, data, single=1)

    def refused_then_fine(c, undo):
        assert compress2(lib, c, data) == -UNSUPPORTED
        undo()
        out = compress2(lib, c, data)
        assert isinstance(out, bytes) and is_one_frame(lib, out) and oracle_lib.decompress(out, len(data)) == data
        lib.ZSTD_freeCCtx(c)
        return out

    for wl in (10, 15, 17):
        c = new_cctx(lib, 3, single=1, params={ZSTD_c_windowLog: wl})
        assert refused_then_fine(c, lambda: lib.ZSTD_CCtx_setParameter(c, ZSTD_c_windowLog, 0)) == good
    c = new_cctx(lib, 3, single=1)
    assert lib.ZSTDMI_CCtx_setSeekTable(c, 1) == 0
    assert refused_then_fine(c, lambda: lib.ZSTDMI_CCtx_setSeekTable(c, 0)) == good
    c = new_cctx(lib, 3, single=1)
    assert lib.ZSTDMI_CCtx_setDevices(c, (ctypes.c_int * 2)(0, 0), 2) == 0
    assert refused_then_fine(c, lambda: lib.ZSTDMI_CCtx_setDevices(c, None, 0)) == good
    c = new_cctx(lib, 3, single=1)
    dic = corpus("text")[2 * MiB:2 * MiB + 20000]
    assert lib.ZSTD_CCtx_loadDictionary(c, dic, len(dic)) == 0
    small = compress2(lib, c, data[:30000])
    assert isinstance(small, bytes) and oracle_lib.decompress(small, 30000, dic) == data[:30000], "one block behind a dictionary is no refusal"
    assert refused_then_fine(c, lambda: lib.ZSTD_CCtx_loadDictionary(c, None, 0)) == good
    # long-distance matching: one of its frames is one frame already (bytes unchanged); more than one frame is refused
    ldm_params = {ZSTD_c_ldm: 1, ZSTD_c_windowLog: 18}
    assert compress(lib, 3, data[:200000], single=1, params=ldm_params) == compress(lib, 3, data[:200000], params=ldm_params)
    c = new_cctx(lib, 3, single=1, params=ldm_params)
    refused_then_fine(c, lambda: lib.ZSTD_CCtx_setParameter(c, ZSTD_c_ldm, 0))


# ---- 6. streams ----
def stream_session(lib, c, pieces, flush_every=None, final_call_carries_input=True):
    """ZSTD_compressStream2 over the pieces, a ZSTD_e_flush whenever flush_every more bytes have gone in, ZSTD_e_end at the end -> bytes"""
    room = ctypes.create_string_buffer(lib.ZSTD_CStreamOutSize())
    out, since = bytearray(), 0

    def call(piece, op):
        keep = ctypes.create_string_buffer(piece, len(piece)) if piece else None
        inb = ZSTD_inBuffer(ctypes.addressof(keep) if piece else None, len(piece), 0)
        while True:
            ob = ZSTD_outBuffer(ctypes.addressof(room), len(room), 0)
            r = lib.ZSTD_compressStream2(c, ctypes.byref(ob), ctypes.byref(inb), op)
            assert not is_error(r), get_error_code(r)
            out.extend(room.raw[:ob.pos])
            if (inb.pos == inb.size) if op == ZSTD_e_continue else (r == 0):
                return

    for i, p in enumerate(pieces):
        last = i == len(pieces) - 1
        if last and final_call_carries_input:
            call(p, ZSTD_e_end)
            return bytes(out)
        call(p, ZSTD_e_continue)
        since += len(p)
        if flush_every and since >= flush_every:
            call(b"", ZSTD_e_flush)
            since = 0
    call(b"", ZSTD_e_flush)            # nothing is buffered when the session ends
    call(b"", ZSTD_e_end)
    return bytes(out)


def odd_pieces(data):
    sizes, out, at, k = (1, 7001, 130001, 65536, 333, 250007), [], 0, 0
    while at < len(data):
        out.append(data[at:at + sizes[k % len(sizes)]])
        at += len(out[-1]); k += 1
    return out


@pytest.mark.parametrize("checksum", [0, 1])
@pytest.mark.parametrize("level", [1, 3, 5])
def test_a_stream_session_is_one_frame(gpu_lib, level, checksum):
    lib = gpu_lib
    data = corpus("text")[:3 * MiB]
    c = new_cctx(lib, level, single=1, params={ZSTD_c_checksumFlag: checksum})
    blob = stream_session(lib, c, odd_pieces(data), flush_every=700000)
    assert is_one_frame(lib, blob), "several batches, one frame"
    assert lib.ZSTD_getFrameContentSize(blob, len(blob)) == UNKNOWN and (blob[4] >> 2) & 1 == checksum
    assert oracle_lib.decompress(blob, len(data)) == data           # (with the flag set the oracle verifies the checksum)
    with z.DecompressionStream(io.BytesIO(blob)) as ds:
        assert ds.ReadToEnd() == data
    if checksum:
        bad = blob[:-1] + bytes([blob[-1] ^ 1])
        assert oracle_lib.decompress(bad, len(data)) == -ZSTD_ErrorCode.ZSTD_error_checksum_wrong
    # the context starts another session: an ZSTD_e_end that carries no input, behind an earlier flush, writes an empty last block
    again = stream_session(lib, c, odd_pieces(data[:900000]), flush_every=400000, final_call_carries_input=False)
    assert is_one_frame(lib, again) and oracle_lib.decompress(again, 900000) == data[:900000]
    tail = again[-7:] if checksum else again[-3:]
    assert tail[:3] == b"\x01\x00\x00", "an empty raw last block"
    with z.DecompressionStream(io.BytesIO(again)) as ds:
        assert ds.ReadToEnd() == data[:900000]
    # an empty session: the empty frame, as with the switch off
    empty = stream_session(lib, c, [b""])
    off = new_cctx(lib, level, params={ZSTD_c_checksumFlag: checksum})
    assert empty == stream_session(lib, off, [b""]) and oracle_lib.decompress(empty, 0) == b""
    lib.ZSTD_freeCCtx(off)
    lib.ZSTD_freeCCtx(c)


def test_compression_stream_mirror_writes_one_frame(gpu_lib):
    lib = gpu_lib
    data = corpus("mixed")[:3 * MiB]
    sink = io.BytesIO()
    with z.CompressionStream(sink, level=3, single_frame=True) as cs:
        for p in odd_pieces(data):
            cs.Write(p)
    blob = sink.getvalue()
    assert is_one_frame(lib, blob) and lib.ZSTD_getFrameContentSize(blob, len(blob)) == UNKNOWN
    assert oracle_lib.decompress(blob, len(data)) == data
    with z.DecompressionStream(io.BytesIO(blob)) as ds:
        assert ds.ReadToEnd() == data
    sink = io.BytesIO()
    with z.CompressionStream(sink, level=3) as cs:
        cs.Write(data)
    assert not is_one_frame(lib, sink.getvalue()), "the default stays a run of frames"


def test_a_stream_session_refuses_what_one_frame_cannot_be(gpu_lib):
    lib = gpu_lib
    c = new_cctx(lib, 3, single=1, params={ZSTD_c_windowLog: 16})
    room, piece = ctypes.create_string_buffer(1 << 18), ctypes.create_string_buffer(corpus("text")[:1000], 1000)
    ob, inb = ZSTD_outBuffer(ctypes.addressof(room), len(room), 0), ZSTD_inBuffer(ctypes.addressof(piece), 1000, 0)
    assert get_error_code(lib.ZSTD_compressStream2(c, ctypes.byref(ob), ctypes.byref(inb), ZSTD_e_end)) == UNSUPPORTED
    assert inb.pos == 0 and ob.pos == 0, "nothing was taken"
    assert not is_error(lib.ZSTD_CCtx_setParameter(c, ZSTD_c_windowLog, 0))
    blob = stream_session(lib, c, [corpus("text")[:1000]])
    assert is_one_frame(lib, blob) and oracle_lib.decompress(blob, 1000) == corpus("text")[:1000]
    lib.ZSTD_freeCCtx(c)


# ---- 7. batch ----
@pytest.mark.parametrize("level", [1, 3])
def test_batch_entries_equal_the_single_call(gpu_lib, level):
    import random
    import torch
    lib = gpu_lib
    rng = random.Random(level)
    sizes = [1, 65536, 65537, 400000] + [rng.choice((rng.randrange(1, 3000), rng.randrange(3000, 65537), rng.randrange(65537, 400001))) for _ in range(36)]
    kinds = list(KINDS)
    items = [corpus(kinds[i % len(kinds)])[i * 1000:i * 1000 + s] for i, s in enumerate(sizes)]
    c = new_cctx(lib, level, single=1)
    singles = [compress2(lib, c, it) for it in items]
    flat = torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).cuda()
    caps = [lib.ZSTD_compressBound(s) for s in sizes]
    out = torch.empty(sum(caps), dtype=torch.uint8, device="cuda")
    srcs, dsts, a, b = [], [], 0, 0
    for s, cap in zip(sizes, caps):
        srcs.append(flat.data_ptr() + a); dsts.append(out.data_ptr() + b)
        a += s; b += cap
    got = (ctypes.c_size_t * len(sizes))()
    torch.cuda.synchronize()
    r = lib.ZSTDMI_compressBatch(c, (ctypes.c_void_p * len(sizes))(*srcs), (ctypes.c_size_t * len(sizes))(*sizes), len(sizes),
                                 (ctypes.c_void_p * len(sizes))(*dsts), (ctypes.c_size_t * len(sizes))(*caps), got)
    assert r == 0
    assert lib.ZSTDMI_debugLastBatchAlone(c) == sum(1 for s in sizes if s > 65536)
    host, b = out.cpu().numpy().tobytes(), 0
    for i, cap in enumerate(caps):
        assert not is_error(got[i]) and got[i] == len(singles[i]), i
        assert host[b:b + got[i]] == singles[i], i
        if sizes[i] > 65536:
            assert is_one_frame(lib, singles[i])
        b += cap
    lib.ZSTD_freeCCtx(c)


# ---- 8. size ----
@pytest.mark.parametrize("level", [3, 5])
def test_one_frame_is_not_larger_than_the_run_of_frames(gpu_lib, level):
    """the same blocks with more history in front of them and fewer headers: structural, not a measured bound"""
    lib = gpu_lib
    data = corpus("text")[:MiB]
    one, run = compress(lib, level, data, single=1), compress(lib, level, data)
    ref = oracle_lib.compress(data, level)
    print(f"level {level}: 1 MiB text, one frame {len(one)}, default {len(run)}, the oracle's one frame {len(ref)}")
    assert len(one) <= len(run)


def test_level_1_sizes_are_recorded_not_bounded(gpu_lib):
    """level 1 cuts differently with the switch on (64 KiB blocks with far candidates against the small call's 16 KiB blocks): the sizes
    are printed for the README; only the round trip is asserted"""
    lib = gpu_lib
    data = corpus("text")[:MiB]
    one, run = compress(lib, 1, data, single=1), compress(lib, 1, data)
    print(f"level 1: 1 MiB text, one frame {len(one)}, default {len(run)}, the oracle's one frame {len(oracle_lib.compress(data, 1))}")
    decodes_everywhere(lib, one, data)
