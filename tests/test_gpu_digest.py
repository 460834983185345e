"""GPU tests of piece digests (include/zstd_mi355x.h "Piece digests"; digest.hip): the device's XXH64 and SHA-256 of many pieces against
the oracle's XXH64 and hashlib at the lengths, alignments and piece counts where the kernels change path; the fused cut-and-digest call
against ZSTDMI_contentCuts and ZSTDMI_digestPieces, with the chunker's host waits; the frame checksum zstd writes as the first four
bytes of the XXH64 digest; digests of a pack's frames; digests shared again behind an edit; and a context that the calls leave alone."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import content_cuts_cases as cc
import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

pytestmark = pytest.mark.gpu

E = ZSTD_ErrorCode
KINDS = ["xxh64", "sha256"]
ZSTD_c_checksumFlag = 201


def on_device(data, shift=0):
    """the bytes in device memory, `shift` bytes behind an allocation's start"""
    import torch
    t = torch.empty(len(data) + shift + 8, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return t[shift:shift + len(data)]


def want_one(kind, piece, oracle):
    if kind == "sha256":
        return hashlib.sha256(piece).digest()
    return int(oracle.lib().zso_xxh64(piece, len(piece), 0)).to_bytes(8, "little")


def pieces_of(data, sizes):
    out, at = [], 0
    for s in sizes:
        out.append(data[at:at + s])
        at += s
    return out


def want_all(kind, data, sizes, oracle):
    return [want_one(kind, p, oracle) for p in pieces_of(data, sizes)]


def frames_of(lib, blob):
    out, at = [], 0
    buf = ctypes.create_string_buffer(blob, len(blob))
    while at < len(blob):
        n = lib.ZSTD_findFrameCompressedSize(ctypes.addressof(buf) + at, len(blob) - at)
        assert not is_error(n) and n > 0
        out.append(blob[at:at + n])
        at += n
    return out


# ---- 1. length and alignment edges ----
EDGE_SIZES = [0, 1, 3, 4, 7, 8, 31, 32, 33, 55, 56, 63, 64, 65, 95, 96, 119, 120, 127, 128, 129, 1023, 4096, 65535, 65536, 65537, 0, 1]


@pytest.mark.parametrize("kind", KINDS)
def test_length_and_alignment_edges(gpu_lib, oracle, kind):
    data = datagen.gen("rand", 256 << 10, 3)
    starts = np.concatenate([[0], np.cumsum(EDGE_SIZES)[:-1]])
    assert {int(s) % 8 for s in starts} == set(range(8)) and sum(EDGE_SIZES) <= len(data)
    want = want_all(kind, data, EDGE_SIZES, oracle)
    with z.Compressor(1) as c:
        assert z.piece_digests(c, data, EDGE_SIZES, kind) == want                   # host memory, staged
        assert z.piece_digests(c, on_device(data), EDGE_SIZES, kind) == want
        assert z.piece_digests(c, on_device(data, 1), EDGE_SIZES, kind) == want     # (every start one residue further)
        assert z.piece_digests(c, data, EDGE_SIZES, {"xxh64": 1, "sha256": 2}[kind]) == want


# ---- 2. piece counts around wave and workgroup sizes ----
@pytest.mark.parametrize("kind", KINDS)
def test_piece_counts(gpu_lib, oracle, kind):
    data = datagen.gen("mixed", 1 << 20, 4)
    src = on_device(data)
    rng = np.random.default_rng(9)
    with z.Compressor(1) as c:
        for n in (1, 63, 64, 65, 257, 4097):
            sizes = [int(x) for x in rng.integers(0, 301, n)]
            assert z.piece_digests(c, src, sizes, kind) == want_all(kind, data, sizes, oracle), n


# ---- 3. one long piece ----
@pytest.mark.parametrize("kind", KINDS)
def test_one_long_piece(gpu_lib, oracle, kind):
    data = datagen.gen("text", (1 << 20) + 8, 5)
    sizes = [(1 << 20) + 5, 3]
    with z.Compressor(1) as c:
        assert z.piece_digests(c, on_device(data), sizes, kind) == want_all(kind, data, sizes, oracle)


# ---- 4. the fused call ----
@functools.lru_cache(maxsize=None)
def fused_inputs(name):
    """1 MiB of the shared inputs, or of the constant byte that has no candidate end"""
    return cc.base("flat" if name == "const" else name)


def host_waits_of(lib, c, call):
    """the waits of the second of two calls (the first allocates)"""
    call()
    before = lib.ZSTDMI_debugHostWaits(c.cctx)
    call()
    return lib.ZSTDMI_debugHostWaits(c.cctx) - before


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("avg_log", [12, 16])
@pytest.mark.parametrize("name", ["text", "rand", "zipf", "const"])
def test_fused_call(gpu_lib, oracle, name, avg_log, kind):
    data = fused_inputs(name)
    with z.Compressor(1) as c:
        for src in (data, on_device(data)):
            sizes = z.content_cuts(c, src, avg_log)
            got_sizes, got = z.content_cuts_digests(c, src, avg_log, kind)
            assert got_sizes == sizes and sum(sizes) == len(data)
            if name == "const":
                assert sizes == [65536] * 16        # every cut forced
            assert got == z.piece_digests(c, src, sizes, kind)
            assert got == want_all(kind, data, sizes, oracle)
            alone = host_waits_of(gpu_lib, c, lambda: z.content_cuts(c, src, avg_log))
            fused = host_waits_of(gpu_lib, c, lambda: z.content_cuts_digests(c, src, avg_log, kind))
            assert fused == alone and alone > 0


def test_fused_call_capacities(gpu_lib):
    data = cc.base("text")[:100000]
    lib = gpu_lib
    with z.Compressor(1) as c:
        want = z.content_cuts(c, data, 12)
        n = len(want)
        sizes, got = (ctypes.c_size_t * n)(*([7] * n)), ctypes.c_size_t(0)
        out = ctypes.create_string_buffer(b"\xA5" * (32 * n), 32 * n)
        call = lambda cap, dcap: lib.ZSTDMI_contentCutsDigests(c.cctx, data, len(data), 12, 2, sizes, cap, ctypes.byref(got), out, dcap)
        for cap, dcap in ((n - 1, 32 * n), (n, 32 * n - 1), (0, 0)):
            got.value = 0
            assert get_error_code(call(cap, dcap)) == E.ZSTD_error_dstSize_tooSmall and got.value == n
            assert list(sizes) == [7] * n and out.raw == b"\xA5" * (32 * n)
        assert call(n, 32 * n) == 0 and list(sizes) == want and got.value == n
        # an empty source has no piece
        assert z.content_cuts_digests(c, b"", 12, "xxh64") == ([], [])


# ---- 5. the checksum field is the digest ----
def test_checksum_field_is_the_xxh64_digest(gpu_lib):
    data = cc.base("text")
    with z.Compressor(1) as c:      # (level 1: a frame holds up to 64 KiB, so every piece is one frame)
        sizes, digests = z.content_cuts_digests(c, data, 12, "xxh64")
        c.content_cuts = 12
        c.SetParameter(ZSTD_c_checksumFlag, 1)
        frames = frames_of(gpu_lib, c.Wrap(data))
    assert len(frames) == len(sizes) and max(sizes) <= 65536
    for i, f in enumerate(frames):
        assert f[-4:] == digests[i][:4], i


# ---- 6. digests of compressed frames ----
@pytest.mark.parametrize("kind", KINDS)
def test_digests_of_a_packs_frames(gpu_lib, oracle, kind):
    data = cc.base("mixed")[:300000]
    items = pieces_of(data, cc.piece_sizes(data, 12))
    with z.Compressor(1) as c:
        stream = z.compress_pack(c, items)
        rows, table_bytes = z.read_seek_table(stream)
        sizes = [comp for comp, _ in rows]
        assert table_bytes > 0 and sum(sizes) == len(stream) - table_bytes and len(sizes) >= len(items)
        assert z.piece_digests(c, on_device(stream), sizes, kind) == want_all(kind, stream, sizes, oracle)


# ---- 7. an insertion ----
def test_digests_are_shared_again_behind_an_insertion(gpu_lib):
    data = cc.base("text")
    edited = cc.insert_edit(data)
    with z.Compressor(1) as c:
        sa, da = z.content_cuts_digests(c, on_device(data), 12, "sha256")
        sb, db = z.content_cuts_digests(c, on_device(edited), 12, "sha256")
    assert len(da) > 100 and da[3:] == db[3:]           # from the fourth piece on
    assert da[:2] == db[:2] and da[2] != db[2] and sa[3:] == sb[3:]


def test_store_flow_compresses_the_new_pieces_only(gpu_lib):
    """the README's flow: cut and digest, look the keys up, pack the pieces the store does not hold"""
    data = cc.base("text")
    edited = cc.insert_edit(data)
    with z.Compressor(1) as c, z.Decompressor() as d:
        sizes, keys = z.content_cuts_digests(c, data, 12, "sha256")
        store = set(keys)
        sizes_b, keys_b = z.content_cuts_digests(c, edited, 12, "sha256")
        new = [i for i, k in enumerate(keys_b) if k not in store]
        assert new == [2]                               # the piece that holds the insertion
        starts = np.concatenate([[0], np.cumsum(sizes_b)]).tolist()
        items = [edited[starts[i]:starts[i] + sizes_b[i]] for i in new]
        stream = z.compress_pack(c, items)
        assert d.Unwrap(stream, maxDecompressedSize=1 << 20) == b"".join(items)


# ---- 8. the context is left alone ----
def test_context_is_left_alone(gpu_lib, oracle):
    import torch
    lib = gpu_lib
    data = cc.base("text")[:100000]
    prefix = cc.base("text")[200000:300000]
    with z.Compressor(1) as fresh:
        want = fresh.Wrap(data)
        fresh.RefPrefix(prefix)
        want_delta = fresh.Wrap(data)
        assert want_delta != want

    def digest_calls(c):
        for kind in KINDS:
            sizes, dg = z.content_cuts_digests(c, data, 14, kind)
            assert z.piece_digests(c, on_device(data), sizes, kind) == dg

    with z.Compressor(1) as c:
        assert c.Wrap(data) == want
        digest_calls(c)
        assert c.Wrap(data) == want
        assert lib.ZSTDMI_debugLastContentCuts(c.cctx) == 0
        # a pending prefix is neither consumed nor refused
        c.RefPrefix(prefix)
        digest_calls(c)
        delta = c.Wrap(data)
        assert delta == want_delta
        with z.Decompressor() as d:
            d.RefPrefix(prefix)
            assert d.Unwrap(delta, maxDecompressedSize=len(data) + 1) == data
        assert c.Wrap(data) == want                     # (the prefix is gone)
        # the last cut call's piece count stays
        c.content_cuts = 12
        c.Wrap(data)
        pieces = lib.ZSTDMI_debugLastContentCuts(c.cctx)
        assert pieces == len(cc.piece_sizes(data, 12))
        digest_calls(c)
        assert lib.ZSTDMI_debugLastContentCuts(c.cctx) == pieces
        c.content_cuts = 0
        # a prepare made before the digest calls is still valid behind them
        c.PrepareBatchAsync(4, 4096)
        digest_calls(c)
        src = on_device(data[:8192])
        dst = torch.empty(4 * 8192, dtype=torch.uint8, device="cuda")
        srcs = torch.tensor([src.data_ptr() + 2048 * i for i in range(4)], dtype=torch.int64, device="cuda")
        dsts = torch.tensor([dst.data_ptr() + 8192 * i for i in range(4)], dtype=torch.int64, device="cuda")
        sizes = torch.full((4,), 2048, dtype=torch.int64, device="cuda")
        caps = torch.full((4,), 8192, dtype=torch.int64, device="cuda")
        out = torch.zeros(4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        assert lib.ZSTDMI_CCtx_setStream(c.cctx, stream.cuda_stream or z.batch._HIP_STREAM_LEGACY) == 0
        assert lib.ZSTDMI_compressBatchAsync(c.cctx, srcs.data_ptr(), sizes.data_ptr(), 4, dsts.data_ptr(), caps.data_ptr(), out.data_ptr()) == 0
        torch.cuda.synchronize()
        assert (out > 0).all()
    # several device workers: refused before a byte is read
    with z.Compressor(1) as c:
        assert lib.ZSTDMI_CCtx_setDevices(c.cctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        with pytest.raises(z.ZstdException) as e:
            z.piece_digests(c, data, [100], "xxh64")
        assert e.value.code == E.ZSTD_error_parameter_unsupported
        assert lib.ZSTDMI_CCtx_setDevices(c.cctx, None, 0) == 0
        assert z.piece_digests(c, data, [100], "xxh64") == [want_one("xxh64", data[:100], oracle)]


# ---- 9. stage names ----
@pytest.mark.parametrize("kind", KINDS)
def test_stage_names(gpu_lib, kind):
    lib = gpu_lib
    data = cc.base("text")[:200000]

    def stages(c):
        ms, names = (ctypes.c_float * 24)(), (ctypes.c_char_p * 24)()
        k = lib.ZSTDMI_CCtx_getStageTimes(c.cctx, ms, names, 24)
        return [names[i].decode() for i in range(k)]

    with z.Compressor(1) as c:
        assert lib.ZSTDMI_CCtx_setProfiling(c.cctx, 1) == 0
        sizes, _ = z.content_cuts_digests(c, data, 12, kind)
        got = stages(c)
        assert "cut_mark" in got and "cut_select" in got and "digest_" + kind in got
        z.piece_digests(c, data, sizes, kind)
        assert stages(c) == ["digest_" + kind]
