"""GPU tests (run with -m gpu on an MI355X): the serial literal decoders (modes 1 and 3, and whatever mode 0 picks) with the
touch that warms a Huffman stream ZMI_LIT_AHEAD bytes ahead of the exact look-ahead loads (decode_lit.hip, huf_decode_stream_fs;
zmi_lit_ahead.h).  The touch reads the stream further down than anything else does, so what is checked is that it
changes no byte and no verdict where its address is clamped: streams shorter than, about as long as and longer than every distance
of DESIGN 11's table, an input that begins at the first byte of its allocation, sections that are damaged.

Every input is built once per module (CPU, the oracle) and only read by the tests."""
import numpy as np
import pytest

import datagen
import zstd_blocks
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

pytestmark = pytest.mark.gpu

SIZES = list(range(300, 4401, 100)) + [65536]
DISTANCES = (128, 256, 384, 512, 768)


def literal_streams(frame):
    """a one-block frame whose block is compressed with a four-stream Huffman literals section and a tree description of its own
    -> (offset of the section's header in the frame, header bytes, bytes of the tree description, the four stream sizes)"""
    blocks = zstd_blocks.blocks_of(frame)
    assert len(blocks) == 1 and blocks[0][0] == 2, [(t, len(b)) for t, b in blocks]
    body = blocks[0][1]
    lit_type, fmt = body[0] & 3, (body[0] >> 2) & 3
    assert lit_type == 2 and fmt != 0, (lit_type, fmt)              # Huffman with its own tree; size formats 1-3 = four streams
    lh = (3, 3, 4, 5)[fmt]
    _, regen, section = zstd_blocks.literals_of(body)
    hb = body[lh]
    tree = 1 + (hb if hb < 128 else (hb - 127 + 1) // 2)
    at = lh + tree
    l1, l2, l3 = (int.from_bytes(body[at + 2 * k:at + 2 * k + 2], "little") for k in range(3))
    l4 = section - lh - tree - 6 - l1 - l2 - l3
    assert l4 > 0, (section, lh, tree, l1, l2, l3)
    return len(frame) - len(body), lh, tree, (l1, l2, l3, l4)


@pytest.fixture(scope="module")
def sweep(oracle):
    src = datagen.zipf_bytes(1 << 20, 5)
    pieces = [src[:n].tobytes() for n in SIZES]
    frames = [oracle.compress(p, 1, 0, 0) for p in pieces]
    sizes = [s for f in frames for s in literal_streams(f)[3]]
    return b"".join(pieces), b"".join(frames), sizes


def test_sweep_is_four_stream_huffman_around_every_distance(sweep):
    """CPU side of the sweep: every frame is one block with four Huffman streams, and the streams lie below, at and above every
    distance (a stream shorter than 16 bytes would go to the plain bit reader and never touch)"""
    _, _, sizes = sweep
    assert len(sizes) == 4 * len(SIZES) and min(sizes) >= 16
    assert min(sizes) < DISTANCES[0] and max(sizes) > 8 * DISTANCES[-1]
    for a, b in zip((0,) + DISTANCES, DISTANCES + (1 << 20,)):
        assert any(a < s <= b for s in sizes), (a, b, sorted(sizes))


@pytest.mark.parametrize("mode", [0, 1, 3], ids=["default", "serial", "compact"])
def test_stream_size_sweep(gpu_lib, sweep, mode):
    """43 frames in one call; the input is a device allocation of its own, so the first frame's streams begin within a few bytes
    of it and the touch of every short stream is clamped to the stream"""
    import torch
    want, blob, _ = sweep
    src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    out = torch.zeros(len(want) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, mode) == 0
        r = gpu_lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), len(want), src.data_ptr(), len(blob))
        assert not is_error(r) and r == len(want), (r, get_error_code(r))
    got = out.cpu().numpy()
    assert got[:r].tobytes() == want and not got[r:].any()


@pytest.fixture(scope="module")
def gpu_frames(gpu_lib):
    zipf = datagen.zipf_bytes(1 << 20, 11).tobytes()
    text = datagen.text_like(1 << 20, 3).tobytes()[:1 << 20]
    with z.Compressor(1) as c:
        return [(zipf, bytes(c.Wrap(zipf))), (text, bytes(c.Wrap(text)))]


@pytest.mark.parametrize("mode", [1, 3], ids=["serial", "compact"])
def test_headline_shaped_and_text_frames(gpu_lib, gpu_frames, mode):
    """16 frames of 64 KiB each: Zipf bytes (no sequences: the literals are decoded in place) and text (sequences: they go to the
    literal scratch, and a block's streams are consumed at another rate)"""
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, mode) == 0
        for data, comp in gpu_frames:
            assert len(zstd_blocks.frames_of(comp)) == 16
            assert bytes(d.Unwrap(comp)) == data


def reframe(frame, cut=0, patch=None):
    """the frame with `cut` bytes taken off the end of its literals section (headers resized) and/or bytes of the section replaced:
    patch = (offset in the block's body, bytes)"""
    at, lh, tree, sizes = literal_streams(frame)
    body = bytearray(frame[at:])
    _, regen, section = zstd_blocks.literals_of(body)
    assert section == lh + tree + 6 + sum(sizes)
    if patch:
        off, b = patch
        assert lh <= off and off + len(b) <= section
        body[off:off + len(b)] = b
    if cut:
        del body[section - cut:section]
        fmt = (body[0] >> 2) & 3
        bits = (10, 10, 14, 18)[fmt]
        v = int.from_bytes(body[:lh], "little")
        comp = (v >> (4 + bits)) - cut
        v = (v & ((1 << (4 + bits)) - 1)) | (comp << (4 + bits))
        body[:lh] = v.to_bytes(lh, "little")
    head = bytearray(frame[:at])
    h = int.from_bytes(head[-3:], "little")
    head[-3:] = ((h & 7) | (len(body) << 3)).to_bytes(3, "little")
    return bytes(head + body)


@pytest.fixture(scope="module")
def damaged(oracle):
    src = datagen.zipf_bytes(1 << 20, 5)
    out = {}
    for n in (2000, 65536):
        data = src[:n].tobytes()
        frame = oracle.compress(data, 1, 0, 0)
        assert reframe(frame) == frame and oracle.decompress(frame, n) == data
        at, lh, tree, sizes = literal_streams(frame)
        section = lh + tree + 6 + sum(sizes)
        out[n] = {"jump_table_exceeds_section": reframe(frame, patch=(lh + tree, b"\xff\xff")),      # the first stream's size: 65535
                  "stream_cut_by_one_byte": reframe(frame, cut=1),                                  # the fourth stream loses its last byte
                  "last_byte_zero": reframe(frame, patch=(section - 1, b"\0"))}                     # the fourth stream's end mark
        for name, f in out[n].items():
            assert f != frame and isinstance(oracle.decompress(f, n), int), (n, name)
    return out


# the codes the build before the touch returned for these inputs, at both modes (run once on it, MI355X): all three are refused by
# the literal stage as corruption_detected
DAMAGED_CODE = {"jump_table_exceeds_section": 20, "stream_cut_by_one_byte": 20, "last_byte_zero": 20}


@pytest.mark.parametrize("mode", [1, 3], ids=["serial", "compact"])
@pytest.mark.parametrize("case", sorted(DAMAGED_CODE))
def test_damaged_sections(gpu_lib, damaged, case, mode):
    assert ZSTD_ErrorCode.ZSTD_error_corruption_detected == 20
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, mode) == 0
        for n in (2000, 65536):
            with pytest.raises(ZstdException) as e:
                d.Unwrap(damaged[n][case], bytearray(n))
            print(f"damaged {case} n={n} mode={mode}: code {int(e.value.Code)}")
            assert int(e.value.Code) == DAMAGED_CODE[case], (case, n, mode)
