"""GPU tests of delta compression (ZSTD_CCtx_refPrefix / ZSTD_DCtx_refPrefix): libzstd-made delta frames decode behind their prefix on
every match-execution path, the GPU compressor's delta frames decode under the oracle and on the GPU, are ONE frame, deterministic
and independent of where the prefix lies, really take their matches from the prefix, and the contract points of the header hold."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

import datagen
import oracle_lib
import prefix_cases
import zstdsharp_amd as z
from prefix_cases import MiB
from zstdsharp_amd.batch import compress_batch, decompress_batch
from zstdsharp_amd.compressor import ZSTD_c_enableLongDistanceMatching as LDM, ZSTD_ps_disable, ZSTD_ps_enable
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer

pytestmark = pytest.mark.gpu

ZSTD_c_windowLog, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 101, 200, 201
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_prefix.json")))["cases"]
CORRUPTION, CHECKSUM_WRONG = ZSTD_ErrorCode.ZSTD_error_corruption_detected, ZSTD_ErrorCode.ZSTD_error_checksum_wrong
UNSUPPORTED = ZSTD_ErrorCode.ZSTD_error_parameter_unsupported


def rand(n, seed):
    return datagen.gen("rand", n, seed)


def on_device(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def wrap(level, data, prefix=None, params=None):
    with z.Compressor(level) as c:
        for k, v in (params or {}).items():
            c.SetParameter(k, v)
        if prefix is not None:
            c.RefPrefix(prefix)
        return c.Wrap(data)


def wrap_code(level, data, prefix, params=None):
    with pytest.raises(ZstdException) as e:
        wrap(level, data, prefix, params)
    return e.value.Code


def unwrap(comp, n, prefix=None, long_frames=0, exec_waves=0):
    with z.Decompressor() as d:
        assert d._lib.ZSTDMI_DCtx_setLongFrames(d.dctx, long_frames) == 0 and d._lib.ZSTDMI_DCtx_setExecWaves(d.dctx, exec_waves) == 0
        if prefix is not None:
            d.RefPrefix(prefix)
        return d.Unwrap(comp, maxDecompressedSize=n)


def unwrap_code(comp, n, prefix=None, **kw):
    with pytest.raises(ZstdException) as e:
        unwrap(comp, n, prefix, **kw)
    return e.value.Code


def frames(lib, comp):
    """content size of every frame of a concatenation"""
    out, pos = [], 0
    while pos < len(comp):
        fsz = lib.ZSTD_findFrameCompressedSize(comp[pos:], len(comp) - pos)
        assert not is_error(fsz)
        out.append(lib.ZSTD_getFrameContentSize(comp[pos:pos + fsz], fsz))
        pos += fsz
    return out


def round_trip(lib, comp, prefix, data):
    assert frames(lib, comp) == [len(data)], "one frame that names its content size"
    assert oracle_lib.decompress(comp, len(data), dict_bytes=prefix) == data, "the oracle's decoder must restore the input behind the prefix"
    assert unwrap(comp, len(data), prefix) == data, "the GPU decoder must restore the input behind the prefix"


# ---------------------------------------------------------------- decoder: libzstd's delta frames

@pytest.mark.parametrize("case", MANIFEST, ids=lambda c: c["case"])
def test_fixture_decodes_behind_its_prefix_on_every_path(gpu_lib, case):
    prefix, content = prefix_cases.build(case["case"])
    blob = open(os.path.join(GOLDEN, case["file"]), "rb").read()
    sha = case["sha256"]
    dev = on_device(prefix)
    for p in (prefix, dev):
        for long_frames, exec_waves in ((0, 0), (1, 0), (2, 0), (1, 1), (1, 4), (1, 16), (2, 4)):
            out = unwrap(blob, case["n"], p, long_frames, exec_waves)
            assert len(out) == case["n"] and hashlib.sha256(out).hexdigest() == sha, (long_frames, exec_waves, p is dev)
    # no prefix: the matches reach in front of the frame; a wrong prefix of the same length: only the checksum can tell.  Neither faults.
    for long_frames in (0, 1, 2):
        assert unwrap_code(blob, case["n"], None, long_frames=long_frames) == CORRUPTION
        assert unwrap_code(blob, case["n"], rand(len(prefix), 999), long_frames=long_frames) == CHECKSUM_WRONG


def test_decoder_prefix_is_single_use(gpu_lib):
    case = next(c for c in MANIFEST if c["case"] == "small_change")
    prefix, content = prefix_cases.build("small_change")
    blob = open(os.path.join(GOLDEN, case["file"]), "rb").read()
    plain = wrap(1, content)
    with z.Decompressor() as d:
        d.RefPrefix(prefix)
        assert d.Unwrap(blob) == content
        with pytest.raises(ZstdException) as e:
            d.Unwrap(blob)
        assert e.value.Code == CORRUPTION
        assert d.Unwrap(plain) == content
        # refused while pending, and still pending afterwards
        d.RefPrefix(on_device(prefix))
        with pytest.raises(ZstdException) as e:
            decompress_batch(d, [blob], [len(content)])
        assert e.value.Code == UNSUPPORTED
        out = ctypes.create_string_buffer(64)
        assert get_error_code(gpu_lib.ZSTDMI_decompressRange(d.dctx, out, 64, blob, len(blob), 0, 1)) == UNSUPPORTED
        assert get_error_code(gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, (ctypes.c_int * 2)(0, 0), 2)) == 0
        keep = d._prefix_keep
        with pytest.raises(ZstdException) as e:
            d.Unwrap(blob)
        assert e.value.Code == UNSUPPORTED                  # several device workers: refused, and the prefix is consumed
        assert gpu_lib.ZSTDMI_DCtx_setDevices(d.dctx, None, 0) == 0
        d.RefPrefix(keep)
        assert d.Unwrap(blob) == content
        # ZSTD_DCtx_loadDictionary cancels a pending prefix; a prefix cancels a loaded dictionary
        d.RefPrefix(prefix); d.LoadDictionary(rand(len(prefix), 999))
        with pytest.raises(ZstdException) as e:
            d.Unwrap(blob)
        assert e.value.Code == CHECKSUM_WRONG
        d.RefPrefix(prefix)
        assert d.Unwrap(blob) == content
        assert d.Unwrap(plain) == content


# ---------------------------------------------------------------- compressor: round trips

@pytest.mark.parametrize("checksum", [0, 1])
@pytest.mark.parametrize("level", [1, 3, 5])
@pytest.mark.parametrize("name", list(prefix_cases.CASES))
def test_round_trip_one_frame_deterministic_host_or_device_prefix(gpu_lib, name, level, checksum):
    prefix, data = prefix_cases.build(name)
    params = {ZSTD_c_checksumFlag: checksum}
    comp = wrap(level, data, prefix, params)
    print(name, level, len(comp), len(comp) / len(data))
    round_trip(gpu_lib, comp, prefix, data)
    assert wrap(level, data, prefix, params) == comp, "a second call writes the same bytes"
    assert wrap(level, data, on_device(prefix), params) == comp, "a device prefix writes the same bytes as a host prefix"
    assert unwrap(comp, len(data), on_device(prefix), long_frames=2, exec_waves=4) == data
    assert unwrap(comp, len(data), prefix, long_frames=1, exec_waves=1) == data
    if prefix_cases.CASES[name][1] == "rand" and name != "edited_rand":
        # random bytes: an unmatched byte costs a byte.  What stays unmatched is a split distance (128 B) plus minMatch (64 B) per
        # 32 - 64 KiB block at the most, so below 1 %; libzstd needs 0.02 - 0.05 % on these inputs
        assert len(comp) <= 0.03 * len(data)


@pytest.mark.parametrize("level", [1, 3])
def test_seam_matches_really_come_from_the_prefix(gpu_lib, level):
    prefix, data = prefix_cases.build("seam")
    cut = wrap(level, data, prefix[:100000])            # nothing of the content is in the first half: only the self-repeat remains
    round_trip(gpu_lib, cut, prefix[:100000], data)
    assert len(cut) >= 0.45 * len(data)
    assert len(wrap(level, data, prefix)) <= 0.03 * len(data)


def test_prefix_much_larger_than_source_and_the_reverse(gpu_lib):
    prefix, data = prefix_cases.build("cut")            # 3 MiB : 70 003 B
    comp = wrap(3, data, prefix)
    round_trip(gpu_lib, comp, prefix, data)
    assert len(comp) <= 0.03 * len(data)
    s = rand(70001, 21)
    body = bytearray(rand(3 * MiB, 22))
    body[MiB:MiB + len(s)] = s
    body[2 * MiB:2 * MiB + len(s) - 1000] = s[1000:]
    body = bytes(body)
    with_prefix = wrap(3, body, s)
    round_trip(gpu_lib, with_prefix, s, body)
    ldm_only = wrap(3, body, None, {LDM: ZSTD_ps_enable})
    print("prefix", len(with_prefix), "ldm only", len(ldm_only))
    assert len(ldm_only) - len(with_prefix) >= 60000        # (libzstd gains 69 990)


# ---------------------------------------------------------------- short form

@pytest.mark.parametrize("n", [900, 30000])
@pytest.mark.parametrize("level", [1, 5])
def test_short_form_writes_the_bytes_of_load_dictionary(gpu_lib, n, level):
    whole = datagen.gen("text", 6000 + n, 31)          # one stream: prefix and content share its vocabulary (a seed has its own)
    prefix, data = whole[:6000], whole[6000:]
    with z.Compressor(level) as c:
        c.LoadDictionary(prefix)
        want = c.Wrap(data)
    for p in (prefix, on_device(prefix)):
        got = wrap(level, data, p)
        assert got == want
    round_trip(gpu_lib, want, prefix, data)
    assert len(want) < len(wrap(level, data))


@pytest.mark.parametrize("prefix_n,n", [(20000, 900), (120000, 200000)])       # the short form and the long form
def test_a_prefix_that_starts_with_the_dictionary_magic_is_raw_content(gpu_lib, prefix_n, n):
    prefix = bytes([0x37, 0xA4, 0x30, 0xEC]) + rand(prefix_n, 33)
    data = prefix[5000:5000 + n // 2] + rand(n - n // 2, 34)
    with z.Compressor(1) as c:
        with pytest.raises(ZstdException) as e:
            c.LoadDictionary(prefix)
            c.Wrap(data)
        assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_dictionary_corrupted
    comp = wrap(1, data, prefix)
    # (the oracle only has decompress_usingDict, which parses such bytes as a formatted dictionary: the GPU decoder alone checks this one)
    assert frames(gpu_lib, comp) == [len(data)]
    assert unwrap(comp, len(data), prefix) == data and unwrap(comp, len(data), on_device(prefix), long_frames=1, exec_waves=1) == data
    assert len(comp) <= 0.56 * len(data)


# ---------------------------------------------------------------- other contract points

def test_short_prefix_single_use_and_cancelling(gpu_lib):
    prefix, data = prefix_cases.build("small_change")
    plain = wrap(3, data)
    assert wrap(3, data, prefix[:7]) == plain               # under 8 bytes: ignored
    with z.Compressor(3) as c:
        c.RefPrefix(prefix)
        first = c.Wrap(data)
        assert len(first) < len(plain) // 10
        assert c.Wrap(data) == plain                        # single use
        c.RefPrefix(prefix)
        ok, _ = c.TryWrap(data, bytearray(10))              # dstSize_tooSmall consumes it too
        assert not ok
        assert c.Wrap(data) == plain
        c.RefPrefix(prefix)
        cap = z.Compressor.GetCompressBound(len(data)); out = ctypes.create_string_buffer(cap)
        r = gpu_lib.ZSTD_compressCCtx(c.cctx, out, cap, data, len(data), 3)       # level-only parameters: ignores it, leaves it pending
        assert out.raw[:r] == plain
        assert c.Wrap(data) == first
        # ZSTD_CCtx_loadDictionary cancels a pending prefix, a prefix (NULL included) a loaded dictionary
        c.RefPrefix(prefix); c.LoadDictionary(None)
        assert c.Wrap(data) == plain
        c.LoadDictionary(prefix[:6000]); c.RefPrefix(None)
        assert c.Wrap(data) == plain
        c.LoadDictionary(prefix[:6000]); c.RefPrefix(prefix)
        assert c.Wrap(data) == first
        assert c.Wrap(data) == plain


def test_device_call_consumes_the_prefix(gpu_lib):
    prefix, data = prefix_cases.build("seam")
    want = wrap(1, data, prefix)
    src, pre = on_device(data), on_device(prefix)
    cap = z.Compressor.GetCompressBound(len(data))
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with z.Compressor(1) as c:
        c.RefPrefix(pre)
        r = gpu_lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, src.data_ptr(), len(data))
        assert not is_error(r) and dst[:r].cpu().numpy().tobytes() == want
        r2 = gpu_lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, src.data_ptr(), len(data))
        assert not is_error(r2) and dst[:r2].cpu().numpy().tobytes() == wrap(1, data)
    out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    comp = on_device(want)
    torch.cuda.synchronize()
    with z.Decompressor() as d:
        d.RefPrefix(pre)
        r = gpu_lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), len(data), comp.data_ptr(), len(want))
        assert r == len(data) and out.cpu().numpy().tobytes() == data
        assert get_error_code(gpu_lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), len(data), comp.data_ptr(), len(want))) == CORRUPTION


def test_what_the_long_form_refuses(gpu_lib):
    prefix, data = prefix_cases.build("small_change")
    assert wrap_code(1, data, prefix, {LDM: ZSTD_ps_disable}) == UNSUPPORTED
    assert wrap_code(1, data, prefix, {ZSTD_c_contentSizeFlag: 0}) == UNSUPPORTED
    assert wrap_code(1, data, prefix, {ZSTD_c_windowLog: 17}) == UNSUPPORTED          # 140 004 bytes need 18
    comp = wrap(1, data, prefix, {ZSTD_c_windowLog: 18})
    round_trip(gpu_lib, comp, prefix, data)
    assert comp == wrap(1, data, prefix) == wrap(1, data, prefix, {LDM: ZSTD_ps_enable})
    with z.Compressor(1) as c:
        assert gpu_lib.ZSTDMI_CCtx_setPassChunks(c.cctx, 1) == 0                      # a source of more than one pass
        c.RefPrefix(prefix)
        with pytest.raises(ZstdException) as e:
            c.Wrap(data)
        assert e.value.Code == UNSUPPORTED
    # 512 MiB of uninitialised device memory + 70 KB: over the decoder's offset record, refused without reading a byte
    big = torch.empty(512 * MiB, dtype=torch.uint8, device="cuda")
    assert wrap_code(1, data, big) == UNSUPPORTED
    del big


def test_calls_that_refuse_a_pending_prefix(gpu_lib):
    prefix, data = prefix_cases.build("small_change")
    want = wrap(1, data, prefix)
    with z.Compressor(1) as c:
        c.RefPrefix(prefix)
        with pytest.raises(ZstdException) as e:
            compress_batch(c, [data[:1000], data[:2000]])
        assert e.value.Code == UNSUPPORTED
        out = ctypes.create_string_buffer(1 << 17); src = ctypes.create_string_buffer(data, len(data))
        ob = ZSTD_outBuffer(ctypes.cast(out, ctypes.c_void_p), 1 << 17, 0)
        ib = ZSTD_inBuffer(ctypes.cast(src, ctypes.c_void_p), len(data), 0)
        assert get_error_code(gpu_lib.ZSTD_compressStream2(c.cctx, ctypes.byref(ob), ctypes.byref(ib), 2)) == UNSUPPORTED
        assert ib.pos == 0 and ob.pos == 0
        assert c.Wrap(data) == want                         # none of them consumed it
        c.seek_table = True
        c.RefPrefix(prefix)
        with pytest.raises(ZstdException) as e:
            c.Wrap(data)
        assert e.value.Code == UNSUPPORTED
        c.seek_table = False
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        c.RefPrefix(prefix)
        with pytest.raises(ZstdException) as e:
            c.Wrap(data)
        assert e.value.Code == UNSUPPORTED
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c.cctx, None, 0) == 0
        c.RefPrefix(prefix)
        assert c.Wrap(data) == want


# ---------------------------------------------------------------- size against the reference

# GPU size against libzstd's (manifest csize) for the (d) cases.  The measured ratio on the MI355X + 10 % was to be the bound; no
# MI355X could be reached when this was written, so MEASURED_VS_LIBZSTD is "not measured" and the bound is structural instead:
# both compressors pay for the edits' random bytes (they are in csize); on top of that this compressor may leave a split distance
# (128 B) plus minMatch (64 B) unmatched per block and writes a block header, a literals header and a sequences section per block
# (33 B allowed), in at most ceil(n / 32 KiB) blocks (the smallest block of any level's framing), and a 13-byte frame header.  An
# edit costs nothing more: the match in front of it runs up to it, the next split behind it is extended back to it.  The test
# prints the ratio; put the measured one here and tighten the bound to it + 10 % once it is known.
MEASURED_VS_LIBZSTD = {"edited_rand": "not measured", "edited_text": "not measured"}


@pytest.mark.parametrize("name", ["edited_rand", "edited_text"])
def test_size_against_libzstd(gpu_lib, name):
    case = next(c for c in MANIFEST if c["case"] == name)
    prefix, data = prefix_cases.build(name)
    comp = wrap(case["level"], data, prefix, {ZSTD_c_checksumFlag: 1})
    blocks = (len(data) + 32767) // 32768
    bound = case["csize"] + blocks * (128 + 64 + 33) + 13
    print(name, "gpu", len(comp), "libzstd", case["csize"], "ratio", len(comp) / case["csize"], "bound", bound / case["csize"],
          "measured", MEASURED_VS_LIBZSTD[name])
    assert len(comp) <= bound
    if name == "edited_rand":
        assert len(comp) <= 0.25 * len(wrap(case["level"], data))       # (the no-prefix size is about n)
