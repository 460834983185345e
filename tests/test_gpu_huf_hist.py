"""GPU tests for the literal histograms (huf_hist_kernel): lane-private byte counters that are summed and zeroed again
before a counter can pass 255.  The inputs are built to break a counter or a flush boundary; the check is the entropy
stage's contract, byte identity with the oracle's restatement of ZSTD_entropyCompressSeqStore.
"""
import ctypes

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(gpu_lib):
    c, d = z.Compressor(1), z.Decompressor()
    yield c, d
    c.Dispose(); d.Dispose()


def _lane_constant(k):
    i = np.arange(65536, dtype=np.uint32)
    return (((i >> 4) & 63) % k).astype(np.uint8).tobytes()


def _one_in_257():
    a = np.full(65536, 0x41, dtype=np.uint8)
    a[::257] = 0x7A
    return a.tobytes()


def _cases():
    cases = [(f"repeat_{n}", bytes([0x55]) * n) for n in (64, 255, 256, 1020, 65280, 65535, 65536)]
    # every aligned 16-byte piece holds one symbol: a lane feeds a single counter 256 times per 16 KiB stream
    cases += [(f"lane_constant_{k}", _lane_constant(k)) for k in (2, 3, 64)]
    cases.append(("one_in_257", _one_in_257()))
    zipf = datagen.zipf_bytes(65536, 21).tobytes()
    cases += [(f"zipf_{n}", zipf[:n]) for n in (65, 257, 1023, 4099, 16385, 40961, 65535)]
    return cases


def test_literal_only_blocks_are_byte_identical_to_oracle(gpu_lib, ctxs, oracle):
    """nbSeq = 0: the block is its literals section, so every histogram error shows in the bytes (wrong code lengths, wrong
    stream sizes or a wrong raw / RLE / compressed verdict)."""
    c, _ = ctxs
    cases = _cases()
    assert len(cases) == 18
    empty = []
    for name, lits in cases:
        n = len(lits)
        want = oracle.entropy_block([], lits, n, 1)
        assert not isinstance(want, int), (name, want)
        arr = (_ffi.ZSTDMI_Seq * 1)()
        out = ctypes.create_string_buffer(n + 1024)
        r = gpu_lib.ZSTDMI_debugEntropyBlock(c.cctx, out, n + 1024, arr, 0, lits, n, n)
        assert r < (1 << 63), (name, r)
        print(f"{name}: n {n} oracle {len(want)} B, gpu {r} B")
        assert out.raw[:r] == want, (name, n, r, len(want))
        if not want:
            empty.append(name)
    assert len(empty) <= 1, empty            # "store raw" says nothing about the histogram: only zipf_65 may


def _chunk_nb_seq(lib, cctx, idx):
    seqs = (_ffi.ZSTDMI_Seq * 16)()
    lits = ctypes.create_string_buffer(16)
    ns, ls = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.ZSTDMI_debugGetChunk(cctx, idx, seqs, 16, ctypes.byref(ns), lits, 16, ctypes.byref(ls)) == 0
    return ns.value


def test_unaligned_device_source_gives_the_same_bytes(gpu_lib, ctxs):
    """A chunk without sequences reads its literals from the caller's source (ChunkMeta::litFromSrc): the counting loop
    meets a base address that is not 16-byte aligned."""
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
            if shift:
                free = [_chunk_nb_seq(gpu_lib, c.cctx, i) == 0 for i in range(4)]
                assert any(free), "no sequence-free chunk in this input: pick another seed"
        for shift, out in zip((1, 3, 8, 15), outs[1:]):
            assert out == outs[0], f"source shifted by {shift} bytes compresses differently"
        assert d.Unwrap(outs[0]) == data.tobytes()
    finally:
        assert gpu_lib.ZSTDMI_CCtx_setHistory(c.cctx, -1, 0) == 0
