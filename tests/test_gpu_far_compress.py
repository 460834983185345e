"""GPU tests of ZSTDMI_CCtx_setFarOffsets (run with -m gpu on an MI355X): delta frames whose matches lie 2^29 bytes and more back.

Everything large stays on the device: inputs are made there (seeded), compressed with ZSTDMI_compressDevice, decoded with
ZSTDMI_decompressDevice and compared there; the oracle decodes each frame once on the host.  The bounds are structural: random bytes
are stored raw (README, the repeated-random row: 0.5001), so a 32 MiB tail that is found in the prefix saves 32 MiB less a few headers,
and 64 MiB found 544 MiB back cost sequences only.
"""
import ctypes

import pytest
import torch

import oracle_lib
import prefix_cases
import zstdsharp_amd as z
from zstdsharp_amd.compressor import ZSTD_c_enableLongDistanceMatching as LDM, ZSTD_ps_enable
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

pytestmark = pytest.mark.gpu

MiB = 1 << 20
ZSTD_c_windowLog = 101
UNSUPPORTED = int(ZSTD_ErrorCode.ZSTD_error_parameter_unsupported)
PREFIX, FRESH, TAIL = 384 * MiB, 130 * MiB, 32 * MiB


def rand_dev(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


def compress_device(lib, c, src, prefix=None):
    """ZSTDMI_compressDevice (behind a referenced device prefix) -> the frame as a device tensor, or the error code as a negative number"""
    cap = lib.ZSTD_compressBound(src.numel())
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if prefix is not None:
        assert lib.ZSTD_CCtx_refPrefix(c.cctx, prefix.data_ptr(), prefix.numel()) == 0
    r = lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, src.data_ptr(), src.numel())
    if is_error(r):
        return -int(get_error_code(r))
    return dst[:r].clone()


def decode_device(lib, comp, n, prefix=None, long_frames=0):
    with z.Decompressor() as d:
        assert lib.ZSTDMI_DCtx_setLongFrames(d.dctx, long_frames) == 0
        out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if prefix is not None:
            assert lib.ZSTD_DCtx_refPrefix(d.dctx, prefix.data_ptr(), prefix.numel()) == 0
        r = lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), n, comp.data_ptr(), comp.numel())
        assert not is_error(r) and r == n, lib.ZSTD_getErrorName(r)
        assert lib.ZSTDMI_debugLastFarPlane(d.dctx) == 1
        assert bool((out[n:] == 0xA5).all())
        return out[:n]


def one_frame(lib, comp, n):
    host = comp.cpu().numpy().tobytes()
    fsz = lib.ZSTD_findFrameCompressedSize(host, len(host))
    return not is_error(fsz) and fsz == len(host) and lib.ZSTD_getFrameContentSize(host, len(host)) == n


def test_delta_of_384_plus_162_mib(gpu_lib):
    """a 384 MiB random prefix; the source is 130 MiB of fresh random bytes and then prefix[:32 MiB]: every match lies 514 MiB back"""
    lib = gpu_lib
    prefix = rand_dev(PREFIX, 1)
    src = torch.cat([rand_dev(FRESH, 2), prefix[:TAIL]])
    n = src.numel()
    assert PREFIX + FRESH >= 1 << 29
    with z.Compressor(1) as c:
        assert compress_device(lib, c, src, prefix) == -UNSUPPORTED            # the switch is off
        c.far_offsets = True
        comp = compress_device(lib, c, src, prefix)
        assert not isinstance(comp, int), comp
        assert one_frame(lib, comp, n)
        # the same call with a fresh random tail: nothing to find
        other = torch.cat([src[:FRESH], rand_dev(TAIL, 3)])
        plain = compress_device(lib, c, other, prefix)
        assert not isinstance(plain, int), plain
        saved = plain.numel() - comp.numel()
        print(f"delta frame {comp.numel()} B, with a fresh tail {plain.numel()} B, saved {saved / MiB:.3f} MiB")
        assert saved >= 31 * MiB
        del other, plain
    for mode in (1, 2):         # the ordered walk, the origin path
        out = decode_device(lib, comp, n, prefix, long_frames=mode)
        assert torch.equal(out, src), ("long frames", mode)
        del out
    got = oracle_lib.decompress(comp.cpu().numpy().tobytes(), n, dict_bytes=prefix.cpu().numpy().tobytes())
    assert not isinstance(got, int), got
    assert got == src.cpu().numpy().tobytes()


def sliding_cctx(lib, window_log, far, pass_chunks=0):
    c = z.Compressor(1)
    c.SetParameter(LDM, ZSTD_ps_enable)
    c.SetParameter(ZSTD_c_windowLog, window_log)
    c.single_frame = True
    c.sliding_ldm = True
    c.far_offsets = far
    if pass_chunks:
        assert lib.ZSTDMI_CCtx_setPassChunks(c.cctx, pass_chunks) == 0
    return c


@pytest.mark.parametrize("pass_chunks", [0, 8192], ids=["one-pass", "window-in-front-of-the-second-pass"])
def test_sliding_window_of_2_30(gpu_lib, pass_chunks):
    """64 MiB random R + 480 MiB zeros + R in ONE frame: at windowLog 30 with the switch on, the second R (544 MiB behind the first) costs
    under 1 MiB.  With 8192 blocks a pass the second R lies in the second pass and its matches in the window in front of it."""
    lib = gpu_lib
    r = rand_dev(64 * MiB, 4)
    src = torch.cat([r, torch.zeros(480 * MiB, dtype=torch.uint8, device="cuda"), r])
    n = src.numel()
    with sliding_cctx(lib, 30, False) as c:
        assert compress_device(lib, c, src) == -UNSUPPORTED                    # windowLog 29 .. 31 without the switch: refused
    with sliding_cctx(lib, 31, True) as c:
        assert compress_device(lib, c, src) == -UNSUPPORTED                    # 31 stays refused
    with sliding_cctx(lib, 30, True, pass_chunks) as c:
        comp = compress_device(lib, c, src)
        assert not isinstance(comp, int), comp
        front = compress_device(lib, c, src[:n - r.numel()])                   # the same frame without the second R
        assert not isinstance(front, int), front
    cost = comp.numel() - front.numel()
    print(f"R + zeros + R: {comp.numel()} B, R + zeros: {front.numel()} B, the second R costs {cost} B")
    assert one_frame(lib, comp, n) and front.numel() > r.numel() and cost < MiB
    out = decode_device(lib, comp, n, long_frames=1)
    assert torch.equal(out, src)
    del out
    if not pass_chunks:
        got = oracle_lib.decompress(comp.cpu().numpy().tobytes(), n)
        assert not isinstance(got, int), got
        assert got == src.cpu().numpy().tobytes()


def test_window_log_29_without_the_switch_stores_the_second_r_raw(gpu_lib):
    """the same input through what windowLog 29 gives without the switch — aligned long-distance frames of 512 MiB (the sliding window
    is refused there, tests/test_gpu_sliding_ldm.py): the second R begins 544 MiB behind the first, in another frame, and is stored raw"""
    lib = gpu_lib
    r = rand_dev(64 * MiB, 4)
    src = torch.cat([r, torch.zeros(480 * MiB, dtype=torch.uint8, device="cuda"), r])
    with z.Compressor(1) as c:
        c.SetParameter(LDM, ZSTD_ps_enable)
        c.SetParameter(ZSTD_c_windowLog, 29)
        comp = compress_device(lib, c, src)
        assert not isinstance(comp, int), comp
    assert comp.numel() >= 2 * r.numel()


def test_switch_on_changes_nothing_where_it_does_not_apply(gpu_lib):
    prefix, data = prefix_cases.build("small_change")
    outs = []
    for far in (False, True):
        with z.Compressor(1) as c:
            c.far_offsets = far
            c.RefPrefix(prefix)
            outs.append(c.Wrap(data))
    assert outs[0] == outs[1]
    with z.Decompressor() as d:
        d.RefPrefix(prefix)
        assert d.Unwrap(outs[1]) == data
        assert gpu_lib.ZSTDMI_debugLastFarPlane(d.dctx) == 0
