"""GPU tests for the literal encoder (huf_encode_kernel): 16 symbols per lane, tiles of 1024 symbols; whole tiles run a body
without a test per symbol, the ragged end of a stream (or a stream shorter than a tile) the general one.  The inputs put streams
at, one below and one above a tile, fill whole tiles with the longest codes, and make many lanes share a dword; the check is the
entropy stage's contract, byte identity with the oracle's restatement of ZSTD_entropyCompressSeqStore.
"""
import ctypes

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd import _ffi

pytestmark = pytest.mark.gpu

ZIPF_SIZES = (255, 256, 257, 511, 1024, 2047, 2048, 2049, 4092, 4093, 4095, 4096, 4097, 4100, 8191, 8192, 8193, 8196, 16384, 32767,
              65533, 65535, 65536)


@pytest.fixture(scope="module")
def ctxs(gpu_lib):
    c, d = z.Compressor(1), z.Decompressor()
    yield c, d
    c.Dispose(); d.Dispose()


def _choice(seed, n, p):
    return np.random.default_rng(seed).choice(len(p), n, p=p).astype(np.uint8).tobytes()


def _long_codes_run():
    """tableLog 11 and 240 symbols of 11 bits: stream 1 holds 4608 of them in a row — whole tiles at the 11 264-bit maximum
    wherever the tiles fall."""
    a = np.random.default_rng(3).choice(4, 65536, p=[.5, .25, .125, .125])
    a[20000:24608] = 4 + np.arange(4608) % 240
    return a.astype(np.uint8).tobytes()


def _cases():
    # (name, literals, size of the oracle's block or None)
    cases = [("long_codes_run", _long_codes_run(), 23427),
             # 1-bit codes: 32 lanes' worth of symbols per dword pair, every tile total = 0 mod 32
             ("bits_1_65536", np.random.default_rng(11).choice(2, 65536).astype(np.uint8).tobytes(), 8210),
             ("bits_1_40000", np.random.default_rng(12).choice(2, 40000).astype(np.uint8).tobytes(), 5018),
             ("bits_122_65536", _choice(13, 65536, [.5, .25, .25]), 12276),
             # odd carries and an unequal last stream
             ("bits_1233_50001", _choice(14, 50001, [.5, .25, .125, .125]), 10937)]
    zipf = datagen.zipf_bytes(65536, 21).tobytes()
    # a stream one below, at and one above a 512- and a 1024-symbol tile; the last stream 0 to 3 symbols short; streams that
    # start at odd addresses; 255: a single stream
    cases += [(f"zipf_{n}", zipf[:n], None) for n in ZIPF_SIZES]
    return cases


def test_literal_only_blocks_are_byte_identical_to_oracle(gpu_lib, ctxs, oracle):
    """nbSeq = 0: the block is its literals section.  Every case is Huffman-coded, so every case goes through the encoder."""
    c, _ = ctxs
    cases = _cases()
    assert len(cases) == 5 + 23
    for name, lits, size in cases:
        n = len(lits)
        want = oracle.entropy_block([], lits, n, 1)
        assert not isinstance(want, int), (name, want)
        assert want and want[0] & 3 == 2, f"{name}: the oracle does not Huffman-code these literals"
        if size is not None:
            assert len(want) == size, (name, len(want), size)
        arr = (_ffi.ZSTDMI_Seq * 1)()
        out = ctypes.create_string_buffer(n + 1024)
        r = gpu_lib.ZSTDMI_debugEntropyBlock(c.cctx, out, n + 1024, arr, 0, lits, n, n)
        assert r < (1 << 63), (name, r)
        print(f"{name}: n {n} oracle {len(want)} B, gpu {r} B")
        assert out.raw[:r] == want, (name, n, r, len(want))


def _chunk_nb_seq(lib, cctx, idx):
    seqs = (_ffi.ZSTDMI_Seq * 16)()
    lits = ctypes.create_string_buffer(16)
    ns, ls = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.ZSTDMI_debugGetChunk(cctx, idx, seqs, 16, ctypes.byref(ns), lits, 16, ctypes.byref(ls)) == 0
    return ns.value


def test_unaligned_device_source_gives_the_same_bytes(gpu_lib, ctxs):
    """A chunk without sequences reads its literals from the caller's source (ChunkMeta::litFromSrc): the encoder's 16-byte
    loads meet every alignment."""
    import torch
    c, d = ctxs
    n = 3 * 65536 + 1000
    data = datagen.zipf_bytes(n, 5)
    cap = gpu_lib.ZSTD_compressBound(n)
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    host = torch.from_numpy(data.copy())
    assert gpu_lib.ZSTDMI_CCtx_setHistory(c.cctx, 0, 0) == 0       # independent 64 KiB chunks, as a large call gets them
    try:
        outs = []
        for shift in (0, 1, 3, 8, 15):
            buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[shift:shift + n] = host.cuda()
            torch.cuda.synchronize()
            r = gpu_lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, buf.data_ptr() + shift, n)
            assert r < (1 << 63), (shift, r)
            outs.append(bytes(dst[:r].cpu().numpy()))
            free = [_chunk_nb_seq(gpu_lib, c.cctx, i) == 0 for i in range(4)]
            assert any(free), "no sequence-free chunk in this input: pick another seed"
        for shift, out in zip((1, 3, 8, 15), outs[1:]):
            assert out == outs[0], f"source shifted by {shift} bytes compresses differently"
        assert d.Unwrap(outs[0]) == data.tobytes()
    finally:
        assert gpu_lib.ZSTDMI_CCtx_setHistory(c.cctx, -1, 0) == 0
