"""GPU tests of long-distance matching (ZSTD_c_enableLongDistanceMatching, zstdsharp_amd/csrc/ldm.hip): repeats megabytes apart are
found, the LDM parameters and the window are honoured, the output is deterministic, and a context that leaves the switch at auto or
disable writes exactly what it wrote before.  Every stream is checked under the GPU decoder and the oracle's decoder."""
import ctypes
import random

import numpy as np
import pytest

import datagen
import oracle_lib
import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.compressor import (ZSTD_c_enableLongDistanceMatching as LDM, ZSTD_c_ldmHashRateLog, ZSTD_c_ldmMinMatch,
                                      ZSTD_ps_auto, ZSTD_ps_disable, ZSTD_ps_enable)
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer

pytestmark = pytest.mark.gpu

ZSTD_c_windowLog, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag, ZSTD_d_windowLogMax = 101, 200, 201, 100
MiB = 1 << 20


def rand(n, seed):
    return datagen.gen("rand", n, seed)


def compress(level, data, ldm=None, params=None):
    with z.Compressor(level) as c:
        if ldm is not None:
            c.SetParameter(LDM, ldm)
        for k, v in (params or {}).items():
            c.SetParameter(k, v)
        return c.Wrap(data)


def round_trip(comp, data):
    assert oracle_lib.decompress(comp, len(data)) == data, "the oracle's decoder must restore the input"
    with z.Decompressor() as d:
        assert d.Unwrap(comp, maxDecompressedSize=len(data)) == data, "the GPU decoder must restore the input"


def frames(lib, comp):
    """content size (or None) of every frame of a concatenation"""
    out, pos = [], 0
    while pos < len(comp):
        fsz = lib.ZSTD_findFrameCompressedSize(comp[pos:], len(comp) - pos)
        assert not is_error(fsz)
        cs = lib.ZSTD_getFrameContentSize(comp[pos:pos + fsz], fsz)
        out.append(cs)
        pos += fsz
    return out


def stream_decode(lib, comp, window_log_max=None):
    """ZSTD_decompressStream over the whole input -> bytes, or the error code"""
    d = lib.ZSTD_createDCtx()
    try:
        if window_log_max is not None:
            assert lib.ZSTD_DCtx_setParameter(d, ZSTD_d_windowLogMax, window_log_max) == 0
        src = ctypes.create_string_buffer(comp, len(comp))
        inb = ZSTD_inBuffer(ctypes.cast(src, ctypes.c_void_p), len(comp), 0)
        out, chunk = bytearray(), ctypes.create_string_buffer(8 * MiB)
        while True:
            ob = ZSTD_outBuffer(ctypes.cast(chunk, ctypes.c_void_p), 8 * MiB, 0)
            r = lib.ZSTD_decompressStream(d, ctypes.byref(ob), ctypes.byref(inb))
            if is_error(r):
                return -get_error_code(r)
            out += chunk.raw[:ob.pos]
            if r == 0 and inb.pos == inb.size:
                return bytes(out)
            assert ob.pos or inb.pos < inb.size or r, "no progress"
    finally:
        lib.ZSTD_freeDCtx(d)


@pytest.mark.parametrize("level", [1, 3, 5])
def test_gain_on_a_repeat_far_beyond_the_block_finders(gpu_lib, level):
    r, s = rand(12 * MiB, 1), rand(20 * MiB, 2)
    data = r + s + r
    on = compress(level, data, ZSTD_ps_enable)
    off = compress(level, data)
    print(level, "ldm", len(on) / len(data), "off", len(off) / len(data))
    assert len(off) >= 0.99 * len(data)
    assert len(on) <= 0.74 * len(data)
    round_trip(on, data)


def test_gain_on_text_repeated_with_edits(gpu_lib):
    t = bytearray(datagen.gen("text", 8 * MiB, 3))
    gap = datagen.gen("text", 24 * MiB - len(t), 4)
    copy = bytearray(t)
    rng = random.Random(5)
    for _ in range(200):
        copy[rng.randrange(len(copy))] ^= 0x5A
    data = bytes(t) + gap + bytes(copy)
    on, off = compress(3, data, ZSTD_ps_enable), compress(3, data)
    print("text ldm", len(on) / len(data), "off", len(off) / len(data))
    assert len(on) < len(off)
    round_trip(on, data)


def test_parameters_are_honoured(gpu_lib):
    """8 MiB of random bytes, then 256-byte slices of it in shuffled order between fresh random bytes: the default minMatch (64)
    finds the slices, minMatch 1024 cannot, a split every 4096 bytes (hashRateLog 12) finds few of them"""
    srcb = rand(8 * MiB, 6)
    rng = random.Random(7)
    idx = list(range(0, 8 * MiB, 256))
    rng.shuffle(idx)
    fresh = rand(len(idx) * 64, 8)
    tail = b"".join(srcb[i:i + 256] + fresh[k * 64:(k + 1) * 64] for k, i in enumerate(idx[:16384]))
    data = srcb + tail
    base = compress(1, data, ZSTD_ps_enable)
    big_mm = compress(1, data, ZSTD_ps_enable, params={ZSTD_c_ldmMinMatch: 1024})
    sparse = compress(1, data, ZSTD_ps_enable, params={ZSTD_c_ldmHashRateLog: 12})
    print("defaults", len(base), "minMatch 1024", len(big_mm), "hashRateLog 12", len(sparse), "input", len(data))
    assert len(base) < len(srcb) + 0.5 * len(tail), "the slices are found with the defaults"
    assert len(big_mm) >= 0.99 * len(data), "no slice is 1024 bytes long"
    assert len(base) < len(sparse) and len(sparse) >= len(srcb) + 0.8 * len(tail), "a split every 4096 bytes misses most slices"
    for comp in (base, big_mm, sparse):
        round_trip(comp, data)


def test_window_is_honoured(gpu_lib):
    lib = gpu_lib
    a = rand(512 * 1024, 9)
    # a repeat 2 MiB back: out of a 1 MiB window
    far = a + rand(2 * MiB - len(a), 10) + a
    # a repeat 512 KiB back inside one 1 MiB-aligned span: only LDM reaches it (the fast finder's far candidates stop at ~188 KiB)
    near = a + a + rand(MiB, 11)
    for data, gain in ((far, False), (near, True)):
        on = compress(1, data, ZSTD_ps_enable, params={ZSTD_c_windowLog: 20})
        off = compress(1, data, params={ZSTD_c_windowLog: 20})
        assert (len(on) < 0.9 * len(off)) == gain, (len(on), len(off), gain)
        assert all(f <= 1 << 20 for f in frames(lib, on))
        assert stream_decode(lib, on, 20) == data
        round_trip(on, data)


def test_window_log_28_frame_needs_window_log_max_28(gpu_lib):
    lib = gpu_lib
    r = rand(16 * MiB, 12)
    data = r + rand(128 * MiB, 13) + r
    comp = compress(1, data, ZSTD_ps_enable, params={ZSTD_c_windowLog: 28})
    assert frames(lib, comp) == [len(data)]
    assert len(comp) < len(data) - 15 * MiB
    assert stream_decode(lib, comp) == -ZSTD_ErrorCode.ZSTD_error_frameParameter_windowTooLarge
    assert stream_decode(lib, comp, 28) == data
    round_trip(comp, data)


def _chunk(lib, cctx, idx):
    seqs = (_ffi.ZSTDMI_Seq * 16384)()
    lits = ctypes.create_string_buffer(65536)
    ns, ls = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.ZSTDMI_debugGetChunk(cctx, idx, seqs, 16384, ctypes.byref(ns), lits, 65536, ctypes.byref(ls)) == 0
    return [(seqs[i].offBase, seqs[i].litLength, seqs[i].mlBase) for i in range(ns.value)], lits.raw[:ls.value]


def test_offsets_above_2_to_the_28(gpu_lib):
    """windowLog 29, one 300 MiB frame, a repeat 280 MiB back: offset code 28 with 28 extra bits (no predefined OF table when a block
    needs more); exact under both decoders, and the debug hook shows such an offset"""
    lib = gpu_lib
    r = rand(4 * MiB, 14)
    data = r + rand(276 * MiB, 15) + r + rand(16 * MiB, 16)
    with z.Compressor(1) as c:
        c.SetParameter(LDM, ZSTD_ps_enable)
        c.SetParameter(ZSTD_c_windowLog, 29)
        comp = c.Wrap(data)
        blk = (len(r) + 276 * MiB) // 65536 + 1
        seqs, _ = _chunk(lib, c.cctx, blk)
    assert any(ob - 3 > (1 << 28) for ob, _, _ in seqs), seqs[:4]
    assert len(comp) < len(data) - 3 * MiB
    round_trip(comp, data)


def test_determinism_and_two_workers(gpu_lib):
    r = rand(6 * MiB, 17)
    data = r + datagen.gen("text", 20 * MiB, 18) + r
    outs = []
    for devs in (None, None, [0, 0]):
        with z.Compressor(3) as c:
            c.SetParameter(LDM, ZSTD_ps_enable)
            if devs:
                arr = (ctypes.c_int * len(devs))(*devs)
                assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, arr, len(devs)) == 0
            outs.append(c.Wrap(data))
    assert outs[0] == outs[1] == outs[2]
    round_trip(outs[0], data)


def test_checksum_no_content_size_and_small_passes(gpu_lib):
    lib = gpu_lib
    r = rand(3 * MiB, 19)
    data = r + rand(5 * MiB, 20) + r
    comp = compress(1, data, ZSTD_ps_enable, params={ZSTD_c_checksumFlag: 1, ZSTD_c_contentSizeFlag: 0})
    assert len(comp) < len(data) - 2 * MiB
    assert oracle_lib.decompress(comp, len(data)) == data
    assert stream_decode(lib, comp, 27) == data
    # passes of 64 blocks (4 MiB): frames are capped by the pass, a repeat 8 MiB back is out of reach, one inside a pass is not
    near = rand(MiB, 21) * 2 + rand(2 * MiB, 22)
    for inp, gain in ((data, False), (near, True)):
        with z.Compressor(1) as c:
            c.SetParameter(LDM, ZSTD_ps_enable)
            assert lib.ZSTDMI_CCtx_setPassChunks(c.cctx, 64) == 0
            comp = c.Wrap(inp)
        assert all(f <= 4 * MiB for f in frames(lib, comp))
        assert (len(comp) < 0.9 * len(inp)) == gain
        round_trip(comp, inp)


def test_streaming_finds_repeats_inside_a_batch(gpu_lib):
    r = rand(2 * MiB, 23)
    data = r + rand(4 * MiB, 24) + r
    from zstdsharp_amd.streams import CompressionStream
    import io
    buf = io.BytesIO()
    with CompressionStream(buf, 1) as cs:
        cs.SetParameter(LDM, ZSTD_ps_enable)
        cs.Write(data)
    comp = buf.getvalue()
    assert len(comp) < len(data) - MiB
    round_trip(comp, data)


def test_auto_disable_compressCCtx_and_small_inputs_keep_their_bytes(gpu_lib):
    lib = gpu_lib
    r = rand(2 * MiB, 25)
    data = r + datagen.gen("text", 3 * MiB, 26) + r
    for level in (1, 3, 19):
        plain = compress(level, data)
        assert compress(level, data, ZSTD_ps_auto) == plain
        assert compress(level, data, ZSTD_ps_disable) == plain
    small = datagen.gen("text", 65536, 27)
    assert compress(3, small, ZSTD_ps_enable) == compress(3, small)
    with z.Compressor(3) as c:
        ref = c.Wrap(data)
    with z.Compressor(3) as c:
        c.SetParameter(LDM, ZSTD_ps_enable)
        cap = lib.ZSTD_compressBound(len(data))
        out = ctypes.create_string_buffer(cap)
        n = lib.ZSTD_compressCCtx(c.cctx, out, cap, data, len(data), 3)
        assert not is_error(n)
        assert out.raw[:n] == ref, "ZSTD_compressCCtx takes the level alone"


def test_dictionary_with_ldm_is_unsupported(gpu_lib):
    data = datagen.gen("text", MiB, 28)
    with z.Compressor(1) as c:
        c.LoadDictionary(datagen.gen("text", 20000, 29))
        c.SetParameter(LDM, ZSTD_ps_enable)
        with pytest.raises(ZstdException) as e:
            c.Wrap(data)
        assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_parameter_unsupported


def _replay_block(seqs, lits, prior, n, rep):
    """execute a block's sequences as the decoder does (repcodes included: seq_encode leaves them resolved in the store)"""
    out = bytearray(prior)
    rep = list(rep)
    lp = 0
    for ob, ll, mlb in seqs:
        out += lits[lp:lp + ll]; lp += ll
        if ob > 3:
            off = ob - 3; rep = [off, rep[0], rep[1]]
        else:
            idx = ob - 1 + (1 if ll == 0 else 0)
            if idx == 0:
                off = rep[0]
            else:
                off = rep[0] - 1 if idx == 3 else rep[idx]
                rep = [off, rep[0], rep[1]] if idx != 1 else [off, rep[0], rep[2]]
        assert 1 <= off <= len(out)
        for _ in range(mlb + 3):
            out.append(out[-off])
    out += lits[lp:]
    assert len(out) == len(prior) + n
    return bytes(out[len(prior):])


def test_merged_sequences_rebuild_every_block(gpu_lib):
    lib = gpu_lib
    r = datagen.gen("text", 1 * MiB, 30)
    data = r + rand(MiB, 31) + r[:700000] + datagen.gen("text", 300000, 32)
    far = 0
    with z.Compressor(1) as c:
        c.SetParameter(LDM, ZSTD_ps_enable)
        comp = c.Wrap(data)
        nblocks = (len(data) + 65535) // 65536
        for b in range(nblocks):
            seqs, lits = _chunk(lib, c.cctx, b)
            end = min(len(data), (b + 1) * 65536)
            # (one frame: its first block starts from the repcodes 1, 4, 8, the later ones from unknown ones that must not be used)
            rep = (1, 4, 8) if b == 0 else (0, 0, 0)
            assert _replay_block(seqs, lits, data[:b * 65536], end - b * 65536, rep) == data[b * 65536:end], b
            far += sum(1 for ob, _, _ in seqs if ob - 3 > 65536)
    assert far > 0
    round_trip(comp, data)
