"""GPU tests of what a single call hands to the host through its context's pinned block instead of a copy to pageable memory
(DESIGN.md 5s): the decoder's status words (reset by a kernel, filed by walk_link, seq_scan and the mirror kernel) and the
compressor's per-pass total and mark offsets (filed by scan_sizes), and of seq_scan's dense plane of sequence counts.

The results must be what they were: every decode is compared byte for byte with the input and with the oracle's decoder, every
compressed stream with the same call under another pass size and with the oracle's decoder.  The pinned block lives as long as the
context and is never cleared between calls, so every property is checked on a context that has just answered something else: an
error behind a good call, a good call behind an error, a small call behind a large one.

Host waits per call (ZSTDMI_debugHostWaitsD / ZSTDMI_debugHostWaits) are held to what the parent of this change was found to make
on an MI355X with these very inputs: 3 for a ZSTDMI_decompressDevice call on the parallel walk (the counting walk, the pre-pass, the
end), ERROR_WAITS for the failing calls, COMPRESS_WAITS for ZSTDMI_compressDevice."""
import ctypes
import functools

import numpy as np
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

pytestmark = pytest.mark.gpu

DECODE_WAITS = 3            # (see the module docstring)
ERROR_WAITS = {"truncated-last-frame": 2, "corrupted-block-header": 2, "capacity-one-short": 1}
COMPRESS_WAITS = {1: (1, 1), 3: (1, 3), 17: (1, 17)}       # chunks -> (default pass size, ZSTDMI_CCtx_setPassChunks(4))
CHUNK = 65536


# ---------------------------------------------------------------- decoder ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decode_cases():
    """name -> (stream, content): the library's level-1 frames and the oracle's, with and without sequences, block counts on both sides of
    a multiple of four (a thread of seq_scan takes four blocks' counts as one load) and of 12 288 (the literal decoder's own stream)"""
    import oracle_lib
    zipf, text = datagen.gen("zipf", 12289 * 512, 3), datagen.gen("text", 900000, 4)
    out = {}
    with z.Compressor(1) as c:
        out["lib-zipf-3-chunks"] = (c.Wrap(zipf[:2 * CHUNK + 1000]), zipf[:2 * CHUNK + 1000])
        out["lib-text-14-chunks"] = (c.Wrap(text), text)
    out["oracle-zipf-12289-frames"] = (oracle_lib.compress(zipf, 1, 0, 512), zipf)
    for n in (1, 2, 3, 5, 4097):        # frames of one block with sequences each
        data = text[:n * 211]
        out[f"oracle-text-{n}-frames"] = (oracle_lib.compress(data, 1, 0, 211), data)
    out["oracle-text-one-frame-7-blocks"] = (oracle_lib.compress(text, 1, 1, 0), text)
    for name, (blob, data) in out.items():
        assert isinstance(blob, bytes), name
    return out


class Device:
    """a stream on the device and a canary-filled destination"""

    def __init__(self, blob, room):
        import torch
        self.torch = torch
        self.src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        self.dst = torch.full((room + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def decode(self, lib, d, cap, size=None):
        size = self.src.numel() if size is None else size
        r = lib.ZSTDMI_decompressDevice(d.dctx, self.dst.data_ptr(), cap, self.src.data_ptr(), size)
        return -get_error_code(r) if is_error(r) else r

    def content(self, n):
        host = self.dst.cpu().numpy()
        assert (host[n:] == 0xA5).all(), "bytes behind the content were written"
        return host[:n].tobytes()


def check_decode(lib, oracle, d, blob, data, what):
    dev = Device(blob, len(data))
    waits = lib.ZSTDMI_debugHostWaitsD(d.dctx)
    r = dev.decode(lib, d, len(data))
    assert r == len(data), (what, r)
    assert lib.ZSTDMI_debugLastWalkSerial(d.dctx) == 0, what
    assert lib.ZSTDMI_debugHostWaitsD(d.dctx) - waits == DECODE_WAITS, what
    assert dev.content(len(data)) == data, what
    assert oracle.decompress(blob, max(len(data), 1)) == data, what


@pytest.mark.parametrize("name", ["lib-zipf-3-chunks", "lib-text-14-chunks", "oracle-zipf-12289-frames", "oracle-text-1-frames", "oracle-text-2-frames",
                                  "oracle-text-3-frames", "oracle-text-5-frames", "oracle-text-4097-frames", "oracle-text-one-frame-7-blocks"])
def test_decode_on_a_fresh_context(gpu_lib, oracle, name):
    blob, data = decode_cases()[name]
    with z.Decompressor() as d:
        check_decode(gpu_lib, oracle, d, blob, data, name)
        allocs = gpu_lib.ZSTDMI_debugDeviceAllocsD(d.dctx)
        check_decode(gpu_lib, oracle, d, blob, data, (name, "again"))
        assert gpu_lib.ZSTDMI_debugDeviceAllocsD(d.dctx) == allocs, "the second call of a steady workload allocates nothing"


def test_decode_one_context_through_every_case(gpu_lib, oracle):
    """large behind small and small behind large: nothing of an earlier call's status words reaches a later call"""
    cases = decode_cases()
    order = sorted(cases, key=lambda k: len(cases[k][0]))
    with z.Decompressor() as d:
        for name in order + order[::-1]:
            check_decode(gpu_lib, oracle, d, *cases[name], name)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4099])
def test_frames_without_a_content_size(gpu_lib, oracle, n):
    """frame_rescan sums the frames' regenerated sizes from block_offsets' dense plane, a thread's four as two loads: frame counts on
    both sides of a multiple of four and beyond one round of the scan, sized frames among the unsized ones"""
    texts = [datagen.gen("text", 300 + 37 * k, 90 + k) for k in range(4)]
    with z.Compressor(1) as c:
        sized = [c.Wrap(t) for t in texts]
        c.SetParameter(200, 0)                              # ZSTD_c_contentSizeFlag
        unsized = [c.Wrap(t) for t in texts]
    pick = [(3 * i) % 4 for i in range(n)]
    blob = b"".join((sized if i % 3 == 2 else unsized)[k] for i, k in enumerate(pick))
    data = b"".join(texts[k] for k in pick)
    dev = Device(blob, len(data))
    with z.Decompressor() as d:
        for again in range(2):
            assert dev.decode(gpu_lib, d, len(data)) == len(data), (n, again)
            assert gpu_lib.ZSTDMI_debugLastWalkSerial(d.dctx) == 1, "frames without a content size take the serial walk"
            assert dev.content(len(data)) == data, (n, again)
        assert dev.decode(gpu_lib, d, len(data) - 1) == -int(ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall)
    assert oracle.decompress(blob, len(data)) == data


def error_cases():
    """name -> (stream, bytes of it to hand over, capacity, the error): as the reference decoder answers them"""
    E = ZSTD_ErrorCode
    def frame_header_size(blob):        # magic, descriptor, window byte, dictID, content size
        fhd = blob[4]
        single, fcs_id, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
        return 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0) if fcs_id == 0 else 1 << fcs_id)
    blob, data = decode_cases()["lib-text-14-chunks"]
    bad = bytearray(blob)
    bad[frame_header_size(blob)] |= 0x06        # the first frame's first block header: block type 3 (reserved)
    return {
        "truncated-last-frame": (blob, len(blob) - 5, len(data), E.ZSTD_error_srcSize_wrong),
        "corrupted-block-header": (bytes(bad), len(bad), len(data), E.ZSTD_error_corruption_detected),
        "capacity-one-short": (blob, len(blob), len(data) - 1, E.ZSTD_error_dstSize_tooSmall),
    }


@pytest.mark.parametrize("name", ["truncated-last-frame", "corrupted-block-header", "capacity-one-short"])
def test_errors_first_and_behind_good_calls(gpu_lib, oracle, name):
    blob, size, cap, want = error_cases()[name]
    good_blob, good = decode_cases()["lib-text-14-chunks"]
    ref = oracle.decompress(blob[:size], cap)
    assert ref == -int(want), (name, "the oracle's decoder answers the same error")
    dev = Device(blob, len(good))
    with z.Decompressor() as d:
        for when in ("first call of the context", "behind a good call"):
            waits = gpu_lib.ZSTDMI_debugHostWaitsD(d.dctx)
            assert dev.decode(gpu_lib, d, cap, size) == -int(want), (name, when)
            assert gpu_lib.ZSTDMI_debugHostWaitsD(d.dctx) - waits == ERROR_WAITS[name], (name, when)
            check_decode(gpu_lib, oracle, d, good_blob, good, (name, "good behind bad", when))


# ---------------------------------------------------------------- compressor ----------------------------------------------------------------
def compress_device(lib, c, src, n):
    import torch
    cap = lib.ZSTD_compressBound(n)
    dst = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    waits = lib.ZSTDMI_debugHostWaits(c.cctx)
    r = lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, src.data_ptr(), n)
    assert not is_error(r), lib.ZSTD_getErrorName(r)
    host = dst.cpu().numpy()
    assert (host[cap:] == 0xA5).all()
    return host[:r].tobytes(), lib.ZSTDMI_debugHostWaits(c.cctx) - waits


@pytest.mark.parametrize("chunks", [1, 3, 17])
def test_compress_passes(gpu_lib, oracle, chunks):
    """the last chunk is short; four chunks per pass: the total of every pass reaches the host, and the passes' outputs lie one behind the other"""
    import torch
    n = (chunks - 1) * CHUNK + 12345
    data = datagen.gen("text", n, 50 + chunks)
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    with z.Compressor(1) as whole, z.Compressor(1) as passes:
        assert gpu_lib.ZSTDMI_CCtx_setPassChunks(passes.cctx, 4) == 0
        want, w1 = compress_device(gpu_lib, whole, src, n)
        for again in range(2):
            got, w4 = compress_device(gpu_lib, passes, src, n)
            assert got == want, (chunks, again)
            assert (w1, w4) == COMPRESS_WAITS[chunks], "as at the parent"
    assert oracle.decompress(want, n) == data


def tiled(kind_sizes, seed):
    """a device buffer of stretches: text (a 1 MiB piece repeated) where the finder has work, random bytes where it has none"""
    import torch
    piece = torch.from_numpy(np.frombuffer(datagen.gen("text", 1 << 20, seed), dtype=np.uint8).copy()).cuda()
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    parts = [piece.repeat(mib) if kind == "text" else torch.randint(0, 256, (mib << 20,), dtype=torch.uint8, device="cuda", generator=gen) for kind, mib in kind_sizes]
    return torch.cat(parts)


# (a plan of ranges, compress_plan: the ranges of a kind are one pass sequence, and each range's place in its output is a mark.  Three
# ranges: the marks travel through the pinned block; eighteen of a kind in one pass: more than it holds, they are read back one by one)
@pytest.mark.parametrize("ranges", [3, 35])
def test_compress_plan_marks(gpu_lib, ranges):
    import torch
    src = tiled([("text", 4) if i % 2 == 0 else ("rand", 8) for i in range(ranges)], ranges)
    n = src.numel()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    with z.Compressor(3) as c, z.Decompressor() as d:
        blob, _ = compress_device(gpu_lib, c, src, n)
        again, _ = compress_device(gpu_lib, c, src, n)
        assert again == blob
        comp = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        r = gpu_lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), n, comp.data_ptr(), len(blob))
        assert r == n, r if not is_error(r) else gpu_lib.ZSTD_getErrorName(r)
    assert torch.equal(out, src)
    # the random stretches were stored and the text was not: both kinds of range ran
    text_mib, rand_mib = 4 * ((ranges + 1) // 2), 8 * (ranges // 2)
    assert (rand_mib << 20) < len(blob) < (rand_mib << 20) + (text_mib << 20) // 2
