"""GPU tests (run with -m gpu on an MI355X): the decoder on FORGED frames — corners of the format that none of the encoders here
writes (tests/forge_cases.py lists them; tests/zstd_forge.py writes them; DESIGN.md "Parity").

What a case must give is in the manifest (forge_cases.load_manifest): for an agreed case the forge's own content, or a refusal;
for a contested one what the oracle does.  Only the committed fixtures, the manifest and the oracle library are read here.
"""
import ctypes
import hashlib
import io
import random

import pytest

import forge_cases
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error
from zstdsharp_amd.streams import DecompressionStream

pytestmark = pytest.mark.gpu

MANIFEST = forge_cases.load_manifest()
CASES = MANIFEST["cases"]
# seq_max_bits_of24 regenerates 17 MiB behind 16 MiB of RLE blocks: it runs under every setting too, but in tests of its own
# (`*_of24`), so that no single test regenerates more than about 20 MiB
OF24 = next(c for c in CASES if c["name"] == "seq_max_bits_of24")
CASES = [c for c in CASES if c is not OF24]
POSITIVES = [c for c in CASES if c["valid"] and c["expect"][0] == "bytes"]
NEGATIVES = [c for c in CASES if c["agreed"] and not c["valid"]]
# THE ONE NAMED EXCEPTION to "a contested case decodes as the oracle decodes it".  A frame without a content size is decoded into a
# slot of its own bound (blocks x block size limit, what ZSTD_decompressBound answers), and one that regenerates more than that is
# refused (block_offsets_kernel, corruption_detected).  Such frames are invalid by the format; the oracle, like the reference's
# one-shot decoder, decodes them when the caller's destination is larger than the bound.  test_unsized_frame_above_its_bound_is_refused
UNSIZED_ABOVE_BOUND = {"neg_unsized_block_above_window", "neg_unsized_rle_block_above_window",
                       "neg_unsized_compressed_block_regenerates_above_window", "neg_unsized_block_regenerates_128k_plus_2"}


def want(c):
    return ("reject",) if c["name"] in UNSIZED_ABOVE_BOUND else c["expect"]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def result(d, c):
    """what the decoder makes of a case, in the manifest's terms"""
    dest = bytearray(max(c["cap"], 1))
    try:
        n = d.Unwrap(c["blob"], dest)
    except ZstdException:
        return ("reject",)
    return ("bytes", n, sha(bytes(dest[:n])))


def check_all(d, cases, what):
    wrong = [(c["name"], want(c)[:2], r[:2]) for c in cases for r in [result(d, c)] if r != want(c)]
    assert not wrong, (what, wrong)


@pytest.fixture(scope="module")
def dctx(gpu_lib):
    d = z.Decompressor()
    yield d
    d.Dispose()


@pytest.fixture(scope="module", params=[1, 2, 3], ids=["serial-literals", "selfsync-literals", "compact-literals"])
def forced_decoder(gpu_lib, request):
    d = z.Decompressor()
    assert gpu_lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, request.param) == 0
    yield d
    d.Dispose()


def test_host_call(dctx):
    check_all(dctx, CASES, "default settings")


def test_host_call_of24(dctx):
    check_all(dctx, [OF24], "default settings")


def test_unsized_frame_above_its_bound_is_refused(dctx, oracle):
    """the named exception above, pinned: the oracle decodes these four, this decoder answers corruption_detected"""
    named = [c for c in MANIFEST["cases"] if c["name"] in UNSIZED_ABOVE_BOUND]
    assert len(named) == len(UNSIZED_ABOVE_BOUND)
    for c in named:
        assert not c["agreed"] and c["oracle"].startswith("different") and not forge_cases.all_sized(c["blob"]), c["name"]
        assert not isinstance(oracle.decompress(c["blob"], c["cap"]), int), c["name"]
        with pytest.raises(ZstdException) as e:
            dctx.Unwrap(c["blob"], bytearray(c["cap"]))
        assert e.value.Code == ZSTD_ErrorCode.ZSTD_error_corruption_detected, c["name"]


def test_every_literal_decoder(forced_decoder):
    check_all(forced_decoder, CASES, "literal decoder")


def test_every_literal_decoder_of24(forced_decoder):
    check_all(forced_decoder, [OF24], "literal decoder")


EXEC_MODES = [("ZSTDMI_DCtx_setExecWaves", 1), ("ZSTDMI_DCtx_setExecWaves", 16), ("ZSTDMI_DCtx_setOverlap", 1), ("ZSTDMI_DCtx_setOverlap", 2)]


@pytest.mark.parametrize("setter,value", EXEC_MODES)
def test_match_execution_modes(gpu_lib, setter, value):
    with z.Decompressor() as d:
        assert getattr(gpu_lib, setter)(d.dctx, value) == 0
        check_all(d, CASES, (setter, value))


@pytest.mark.parametrize("setter,value", EXEC_MODES)
def test_match_execution_modes_of24(gpu_lib, setter, value):
    with z.Decompressor() as d:
        assert getattr(gpu_lib, setter)(d.dctx, value) == 0
        check_all(d, [OF24], (setter, value))


@pytest.mark.parametrize("name", [c["name"] for c in CASES + [OF24] if {"long-frame", "seq-max-bits"} & set(c["tags"])])
@pytest.mark.parametrize("mode", [1, 2], ids=["walk", "origin-pointers"])
def test_long_frames(gpu_lib, mode, name):
    c = next(c for c in CASES + [OF24] if c["name"] == name)
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setLongFrames(d.dctx, mode) == 0
        assert result(d, c) == c["expect"]


def _concat_orders(cases):
    for seed in (1, 2, 3):
        order = list(cases)
        random.Random(seed).shuffle(order)
        yield order


def test_many_sized_frames_in_one_call(gpu_lib, dctx):
    """frames of every header form, block mix, mode and table log side by side in one call: one parallel walk, and blocks of
    different kinds in one sequence-decoder workgroup"""
    cases = [c for c in POSITIVES if c["agreed"] and forge_cases.all_sized(c["blob"]) and c["size"] <= (1 << 20)]      # (three orders: 8 MiB)
    assert len(cases) > 100 and any("skippable" in c["tags"] for c in cases)
    for order in _concat_orders(cases):
        blob = b"".join(c["blob"] for c in order)
        total = sum(c["size"] for c in order)
        dest = bytearray(total)
        assert dctx.Unwrap(blob, dest) == total
        assert gpu_lib.ZSTDMI_debugLastWalkSerial(dctx.dctx) == 0
        at = 0
        for c in order:
            assert sha(bytes(dest[at:at + c["size"]])) == c["sha256"], c["name"]
            at += c["size"]


def test_many_unsized_frames_in_one_call(gpu_lib, dctx):
    cases = [c for c in POSITIVES if c["agreed"] and not forge_cases.all_sized(c["blob"])]
    assert len(cases) > 10
    for order in _concat_orders(cases):
        blob = b"".join(c["blob"] for c in order)
        total = sum(c["size"] for c in order)
        dest = bytearray(total)
        assert dctx.Unwrap(blob, dest) == total
        assert gpu_lib.ZSTDMI_debugLastWalkSerial(dctx.dctx) == 1
        at = 0
        for c in order:
            assert sha(bytes(dest[at:at + c["size"]])) == c["sha256"], c["name"]
            at += c["size"]


def batch(lib, d, blobs, caps):
    """ZSTDMI_decompressBatch over host blobs -> per entry its bytes, or its error code as a negative number"""
    import torch
    n = len(blobs)
    flat = torch.frombuffer(bytearray(b"".join(blobs)) or bytearray(1), dtype=torch.uint8).cuda()
    srcs, at = [], 0
    for b in blobs:
        srcs.append(flat.data_ptr() + at if b else None)
        at += len(b)
    starts, at = [], 0
    for cap in caps:
        starts.append(at)
        at += cap + 32
    out = torch.full((max(at, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    got = (ctypes.c_size_t * n)()
    torch.cuda.synchronize()
    r = lib.ZSTDMI_decompressBatch(d.dctx, (ctypes.c_void_p * n)(*srcs), (ctypes.c_size_t * n)(*[len(b) for b in blobs]), n,
                                   (ctypes.c_void_p * n)(*[out.data_ptr() + s for s in starts]), (ctypes.c_size_t * n)(*caps), got)
    assert not is_error(r), lib.ZSTD_getErrorName(r)
    host = out.cpu().numpy()
    res = []
    for i in range(n):
        if is_error(got[i]):
            res.append(-int(get_error_code(got[i])))
        else:
            res.append(host[starts[i]:starts[i] + got[i]].tobytes())
            assert (host[starts[i] + got[i]:starts[i] + caps[i] + 32] == 0xA5).all(), ("entry wrote past its result", i)
    return res


def test_batch_of_all_positives(gpu_lib, dctx):
    cases = POSITIVES
    res = batch(gpu_lib, dctx, [c["blob"] for c in cases], [c["cap"] for c in cases])
    # README "Batch": entries that hold a frame without a content size, and entries above 4 MiB compressed, go alone
    alone = sum(1 for c in cases if not forge_cases.all_sized(c["blob"]) or c["csize"] > (4 << 20))
    assert 0 < alone < len(cases) and gpu_lib.ZSTDMI_debugLastBatchAloneD(dctx.dctx) == alone
    wrong = [c["name"] for c, r in zip(cases, res) if isinstance(r, int) or (len(r), sha(r)) != c["expect"][1:]]
    assert not wrong, wrong


def test_batch_of24(gpu_lib, dctx):
    mates = [c for c in POSITIVES if c["agreed"] and c["size"] <= 8192][:6]
    cases = mates[:3] + [OF24] + mates[3:]
    res = batch(gpu_lib, dctx, [c["blob"] for c in cases], [c["cap"] for c in cases])
    wrong = [c["name"] for c, r in zip(cases, res) if isinstance(r, int) or (len(r), sha(r)) != c["expect"][1:]]
    assert not wrong, wrong


def test_batch_with_one_negative_entry(gpu_lib, dctx):
    """a refused entry fails alone, with the code the single call gives it, and its neighbours' bytes are intact"""
    around = [c for c in POSITIVES if c["agreed"] and c["size"] <= 8192]
    rng = random.Random(5)
    for neg in NEGATIVES:
        with pytest.raises(ZstdException) as e:
            dctx.Unwrap(neg["blob"], bytearray(neg["cap"]))
        code = int(e.value.Code)
        mates = rng.sample(around, 4)
        cases = mates[:2] + [neg] + mates[2:]
        res = batch(gpu_lib, dctx, [c["blob"] for c in cases], [c["cap"] for c in cases])
        assert res[2] == -code, (neg["name"], res[2], code)
        for c, r in zip(cases, res):
            if c is not neg:
                assert not isinstance(r, int) and (len(r), sha(r)) == c["expect"][1:], (neg["name"], c["name"])


FEEDS = dict(argvalues=[1, 7, 1 << 20], ids=["1-byte", "7-bytes", "all-at-once"])


def stream_all(cases, feed):
    with z.Decompressor() as d:
        for c in cases:
            with DecompressionStream(io.BytesIO(c["blob"]), feed, decompressor=d) as ds:
                out = ds.ReadToEnd(1 << 20)
            assert (len(out), sha(out)) == c["expect"][1:], (c["name"], feed)


@pytest.mark.parametrize("feed", **FEEDS)
def test_streaming(gpu_lib, feed):
    stream_all(POSITIVES, feed)


@pytest.mark.parametrize("feed", **FEEDS)
def test_streaming_of24(gpu_lib, feed):
    stream_all([OF24], feed)


@pytest.mark.parametrize("name", [c["name"] for c in CASES if "long-frame" in c["tags"]])
def test_streaming_long_frames_in_segments(gpu_lib, name):
    """ZSTDMI_DCtx_setStreamSegment at its smallest value: every whole block that has arrived is a segment of its own"""
    c = next(c for c in CASES if c["name"] == name)
    with z.Decompressor() as d:
        d.stream_segment = 1
        with DecompressionStream(io.BytesIO(c["blob"]), 256, decompressor=d) as ds:
            out = ds.ReadToEnd(1 << 20)
        assert (len(out), sha(out)) == c["expect"][1:]
        # fed 256 bytes at a time, no call sees the whole frame (8 KiB and more): it was decoded in pieces, not as one frame
        assert c["csize"] > 8 * 256 and gpu_lib.ZSTDMI_debugStreamSegments(d.dctx) >= 2


def test_random_frames(gpu_lib, dctx):
    """the 200 seeded frames of tests/test_forge_cpu.py, forged here: one batch call, and one call over all of them in a row"""
    frames = [forge_cases.random_frame(1000 + seed) for seed in range(200)]
    res = batch(gpu_lib, dctx, [f for f, _ in frames], [len(c) for _, c in frames])
    wrong = [seed for seed, ((_, c), r) in enumerate(zip(frames, res)) if r != c]
    assert not wrong, wrong
    want = b"".join(c for _, c in frames)
    dest = bytearray(len(want))
    assert dctx.Unwrap(b"".join(f for f, _ in frames), dest) == len(want)
    assert bytes(dest) == want


def test_no_negative_is_accepted(forced_decoder):
    """frames that both libzstd versions and the oracle refuse: none may be accepted (the `lenient == 0` condition of
    test_gpu_parity.test_corrupted_frames_fail_cleanly)"""
    assert len(NEGATIVES) >= 20
    lenient = [c["name"] for c in NEGATIVES if result(forced_decoder, c) != ("reject",)]
    assert len(lenient) == 0, lenient
