"""GPU tests (run with -m gpu on an MI355X): offsets of 2^29 and more in the decoder (tests/far_cases.py; tests/test_far_cases_cpu.py
holds the same frames to the oracle and to the forge's executor).

A case regenerates 512 MiB (one: 1 GiB), so output is compared ON THE DEVICE: the destination is filled with 0xA5, decoded into, and
must hold the seed, zeros, and the tail behind them.  A frame is forged once per session and decoded under every setting.  The
device holds at most about 3 GiB at a time (destination, literal scratch and — on the origin path — four bytes of origin per byte).
"""
import ctypes
import struct

import numpy as np
import pytest

import far_cases
import zstdsharp_amd as z
from zstdsharp_amd.decompressor import ZSTD_d_windowLogMax
from zstdsharp_amd.dictionaries import DDict
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer

pytestmark = pytest.mark.gpu

WINDOW_TOO_LARGE = int(ZSTD_ErrorCode.ZSTD_error_frameParameter_windowTooLarge)
CORRUPTION = int(ZSTD_ErrorCode.ZSTD_error_corruption_detected)
_built = {}


def case(name):
    """forged once per session; on the device: the frame, and the seed and tail the content must hold"""
    import torch
    if name not in _built:
        c = far_cases.build(name)
        dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
        c["d_blob"] = dev(c["blob"])
        if c["valid"]:
            c["d_head"], c["d_tail"] = dev(c["head"]), dev(c["tail"])
        _built[name] = c
    return _built[name]


def decode_device(lib, d, c):
    """ZSTDMI_decompressDevice into a destination of the case's capacity -> (result, destination)"""
    import torch
    out = torch.full((c["cap"] + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), c["cap"], c["d_blob"].data_ptr(), c["d_blob"].numel())
    return r, out


def check_content(c, out):
    """the comparison, on the device: seed | zeros | tail, and nothing behind the content"""
    import torch
    n, t = c["size"], c["tail_off"]
    assert torch.equal(out[:far_cases.SEED_BYTES], c["d_head"]), (c["name"], "seed")
    assert not bool(out[far_cases.SEED_BYTES:t].any()), (c["name"], "fill")
    if not torch.equal(out[t:n], c["d_tail"]):
        got, want = out[t:n].cpu().numpy(), c["d_tail"].cpu().numpy()
        first = int(np.nonzero(got != want)[0][0])
        raise AssertionError((c["name"], "tail differs first at", first, bytes(got[first:first + 16]), bytes(want[first:first + 16])))
    assert bool((out[n:] == 0xA5).all()), (c["name"], "wrote behind the content")


def with_dictionary(d, c, how="load"):
    if c["dict"] is None:
        return None
    if how == "load":
        d.LoadDictionary(c["dict"])
    elif how == "ddict":
        dd = DDict(c["dict"])
        d.RefDDict(dd)
        return dd
    else:
        d.RefPrefix(c["dict"])
    return None


@pytest.mark.parametrize("waves", [1, 16])
@pytest.mark.parametrize("mode", [1, 2], ids=["walk", "origin"])
@pytest.mark.parametrize("name", far_cases.VALID)
def test_far_frames_decode_bit_exact(gpu_lib, name, mode, waves):
    c = case(name)             # (a frame of 1 GiB and more keeps the ordered walk under either setting of setLongFrames)
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setLongFrames(d.dctx, mode) == 0 and gpu_lib.ZSTDMI_DCtx_setExecWaves(d.dctx, waves) == 0
        keep = with_dictionary(d, c)
        r, out = decode_device(gpu_lib, d, c)
        assert not is_error(r), (name, gpu_lib.ZSTD_getErrorName(r))
        assert r == c["size"]
        assert gpu_lib.ZSTDMI_debugLastFarPlane(d.dctx) == 1
        check_content(c, out)
        del keep


@pytest.mark.parametrize("how", ["ddict", "prefix", "using_ddict"])
def test_far_offset_into_a_dictionary_however_it_is_given(gpu_lib, how):
    """refDDict, refPrefix and ZSTD_decompress_usingDDict (a host call: 512 MiB come back and are compared on the host)"""
    import torch
    c = case("raw_dict_1000")
    with z.Decompressor() as d:
        if how == "using_ddict":
            dd = DDict(c["dict"])
            out = np.full(c["cap"], 0xA5, dtype=np.uint8)
            r = gpu_lib.ZSTD_decompress_usingDDict(d.dctx, out.ctypes.data, c["cap"], c["blob"], len(c["blob"]), dd.handle)
            assert not is_error(r) and r == c["size"], gpu_lib.ZSTD_getErrorName(r)
            t = c["tail_off"]
            assert out[:4096].tobytes() == c["head"] and not out[4096:t].any() and out[t:].tobytes() == c["tail"]
            return
        keep = with_dictionary(d, c, how)
        torch.cuda.synchronize()
        r, out = decode_device(gpu_lib, d, c)
        assert not is_error(r) and r == c["size"], gpu_lib.ZSTD_getErrorName(r)
        check_content(c, out)
        del keep


def stream_decode(lib, d, blob, cap):
    """the whole frame through ZSTD_decompressStream into one host buffer -> (bytes written or an error code as a negative number, buffer)"""
    out = np.full(cap + 64, 0xA5, dtype=np.uint8)
    src = ctypes.create_string_buffer(blob, len(blob))
    o, i = ZSTD_outBuffer(out.ctypes.data, cap, 0), ZSTD_inBuffer(ctypes.addressof(src), len(blob), 0)
    for _ in range(1 << 16):
        r = lib.ZSTD_decompressStream(d.dctx, ctypes.byref(o), ctypes.byref(i))
        if is_error(r):
            return -int(get_error_code(r)), out
        if r == 0 and i.pos == i.size:
            return o.pos, out
    raise AssertionError("the stream does not end")


@pytest.mark.parametrize("name", far_cases.VALID)
def test_far_frames_through_decompress_stream(gpu_lib, name):
    """unsegmented ZSTD_decompressStream: ZSTD_d_windowLogMax still decides what a frame may ask for — 30 admits every case below
    1 GiB and refuses the 1 GiB frame, which 31 admits"""
    c = case(name)
    with z.Decompressor() as d:
        d.SetParameter(ZSTD_d_windowLogMax, 30)
        with_dictionary(d, c)
        if not c["below_1g"]:
            n, _ = stream_decode(gpu_lib, d, c["blob"], c["cap"])
            assert n == -WINDOW_TOO_LARGE
            d.SetParameter(ZSTD_d_windowLogMax, 31)
        n, out = stream_decode(gpu_lib, d, c["blob"], c["cap"])
        assert n == c["size"], n
        t = c["tail_off"]
        assert out[:far_cases.SEED_BYTES].tobytes() == c["head"] and not out[far_cases.SEED_BYTES:t].any()
        assert out[t:n].tobytes() == c["tail"] and (out[n:] == 0xA5).all()


def test_stream_window_log_max_29_refuses_the_far_frames(gpu_lib):
    c = case("code29")
    with z.Decompressor() as d:
        d.SetParameter(ZSTD_d_windowLogMax, 29)
        n, _ = stream_decode(gpu_lib, d, c["blob"], c["cap"])
        assert n == -WINDOW_TOO_LARGE


@pytest.mark.parametrize("waves", [1, 16])
@pytest.mark.parametrize("mode", [1, 2], ids=["walk", "origin"])
def test_far_offset_in_front_of_the_frame_is_corruption(gpu_lib, mode, waves):
    c = case("before_frame")
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setLongFrames(d.dctx, mode) == 0 and gpu_lib.ZSTDMI_DCtx_setExecWaves(d.dctx, waves) == 0
        r, _ = decode_device(gpu_lib, d, c)
        assert is_error(r) and int(get_error_code(r)) == CORRUPTION, gpu_lib.ZSTD_getErrorName(r)


def test_a_frame_that_cannot_reach_that_far_keeps_its_answer(gpu_lib):
    """the code-29 block behind 64 KiB instead of 512 MiB: no far plane, and the answer such a frame always got — also as the small
    neighbour of a far-capable frame in the same call, where the kernels are the far instances"""
    import torch
    import zstd_forge as F
    blocks = [far_cases.raw(far_cases.seed_block()), far_cases.rle(0, 60 << 10), far_cases.far_block(far_cases.three(536874913), 2)]
    small, _ = F.frame(blocks, valid=False, fcs_value=(64 << 10) + 300)
    with z.Decompressor() as d:
        with pytest.raises(ZstdException) as e:
            d.Unwrap(small, bytearray(1 << 17))
        assert int(e.value.Code) == WINDOW_TOO_LARGE and gpu_lib.ZSTDMI_debugLastFarPlane(d.dctx) == 0
        c = case("code29")
        both = torch.frombuffer(bytearray(c["blob"] + small), dtype=torch.uint8).cuda()
        out = torch.empty(c["size"] + (1 << 17), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r = gpu_lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), out.numel(), both.data_ptr(), both.numel())
        assert is_error(r) and int(get_error_code(r)) == WINDOW_TOO_LARGE and gpu_lib.ZSTDMI_debugLastFarPlane(d.dctx) == 1


def test_ordinary_calls_have_no_far_plane(gpu_lib):
    import datagen
    data = datagen.gen("text", 300000, 3)
    with z.Compressor(3) as cc, z.Decompressor() as d:
        assert d.Unwrap(cc.Wrap(data)) == data
        assert gpu_lib.ZSTDMI_debugLastFarPlane(d.dctx) == 0


def with_seek_table(blob, size):
    """the frame as a seekable stream of one entry (the zstd seekable format)"""
    return blob + struct.pack("<IIIIIBI", 0x184D2A5E, 8 + 9, len(blob), size, 1, 0, 0x8F92EAB1)


def test_batch_ranges_and_segments_keep_their_refusal(gpu_lib):
    import torch
    c = case("code29")
    with z.Decompressor() as d:
        # ZSTDMI_decompressBatch: the entry's own answer
        out = torch.empty(c["cap"], dtype=torch.uint8, device="cuda")
        got = (ctypes.c_size_t * 1)()
        torch.cuda.synchronize()
        r = gpu_lib.ZSTDMI_decompressBatch(d.dctx, (ctypes.c_void_p * 1)(c["d_blob"].data_ptr()), (ctypes.c_size_t * 1)(len(c["blob"])), 1,
                                           (ctypes.c_void_p * 1)(out.data_ptr()), (ctypes.c_size_t * 1)(c["cap"]), got)
        assert not is_error(r) and is_error(got[0]) and int(get_error_code(got[0])) == WINDOW_TOO_LARGE
        del out
        # ZSTDMI_decompressRange / ZSTDMI_decompressRanges over the frame with a seek table
        seekable = torch.frombuffer(bytearray(with_seek_table(c["blob"], c["size"])), dtype=torch.uint8).cuda()
        with pytest.raises(ZstdException) as e:
            d.unwrap_range(seekable, c["tail_off"], 100)
        assert int(e.value.Code) == WINDOW_TOO_LARGE
        with pytest.raises(ZstdException) as e:
            d.unwrap_ranges(seekable, [(c["tail_off"], 100)])
        assert int(e.value.Code) == WINDOW_TOO_LARGE
    with z.Decompressor() as d:
        # a segmented stream (ZSTDMI_DCtx_setStreamSegment): the frame is decoded in pieces, and the piece with the far offset is refused
        d.stream_segment = 4096
        d.SetParameter(ZSTD_d_windowLogMax, 30)         # (the header's window passes: what refuses is the sequence)
        n, _ = stream_decode(gpu_lib, d, c["blob"], c["cap"])
        assert n == -WINDOW_TOO_LARGE and gpu_lib.ZSTDMI_debugStreamSegments(d.dctx) >= 2
