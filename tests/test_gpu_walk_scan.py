"""GPU tests of the decoder's front end: the parallel frame walk's scan for a segment's first frame start (walk_segments reads
its 128 KiB segment in windows of several KiB, sixteen positions per lane) and the single-workgroup scans behind it (walk_link,
seq_scan, frame_rescan).  Every case checks the decoded bytes, the return value and that the call took the parallel walk: a scan
that misses or misplaces a frame start cannot close the segment links, and the call lands on the serial walk.

Streams are hand-made: a first frame of about 70 KB of random bytes stored raw, then a skippable frame of zeros whose length puts
the next real frame's magic exactly where the case wants it in segment 1 (that segment's first candidate), then a few small frames.

False candidates: a fake is the zstd magic followed by an invalid frame header, g bytes in front of the real frame.  From g = 4 on
that is literal (at g = 4 the real frame's first byte, 0x28, is the fake's header byte: its reserved bit is set).  No frame magic
is a shifted copy of another one's tail, so two magics can never start fewer than four bytes apart; for g = 1, 2, 3 the case is the
nearest thing that exists: the first g bytes of the magic, cut short by the real frame (a near miss that must not become a hit)."""
import numpy as np
import pytest

import datagen
import zstdsharp_amd as z

pytestmark = pytest.mark.gpu

SEG = 1 << 17
ZSTD_MAGIC = bytes([0x28, 0xB5, 0x2F, 0xFD])
FRONT = 64                                  # bytes of the tensor in front of the source (keeps the shift as the pointer's alignment)


def raw_frame(payload: bytes) -> bytes:
    """a single-segment frame with a content size whose blocks are stored raw"""
    n = len(payload)
    if n < 256: hdr = bytes([0x20, n])
    elif n < 65536 + 256: hdr = bytes([0x60]) + (n - 256).to_bytes(2, "little")
    else: hdr = bytes([0xA0]) + n.to_bytes(4, "little")
    out = bytearray(ZSTD_MAGIC + hdr)
    if n == 0: return bytes(out + bytes([1, 0, 0]))
    for off in range(0, n, SEG):
        piece = payload[off:off + SEG]
        out += ((len(piece) << 3) | (1 if off + SEG >= n else 0)).to_bytes(3, "little") + piece
    return bytes(out)


def skippable(total: int, tail: bytes = b"", magic: int = 0x184D2A50) -> bytes:
    """a skippable frame of `total` bytes in all: zeros, ending with `tail`"""
    assert total >= 8 + len(tail), total
    return magic.to_bytes(4, "little") + (total - 8).to_bytes(4, "little") + bytes(total - 8 - len(tail)) + tail


@pytest.fixture(scope="module")
def parts(oracle):
    """the pieces every hand-made stream is built from (made once, never changed)"""
    rng = np.random.default_rng(2024)
    first = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    texts = [datagen.gen("text", 3000 + 17 * k, 40 + k) for k in range(3)]
    small = [oracle.compress(texts[0], 1, 0, 0), raw_frame(texts[1][:100]), oracle.compress(texts[2], 1, 1, 0)]
    assert all(isinstance(f, bytes) for f in small)
    return {"first": first, "first_frame": raw_frame(first), "small": small, "small_data": [texts[0], texts[1][:100], texts[2]]}


@pytest.fixture(scope="module")
def dctx(gpu_lib):
    with z.Decompressor() as d:
        yield d


def stream_with_magic_at(parts, pos: int, fake_tail: bytes = b""):
    """first frame, zeros up to `pos` (ending with fake_tail), then the small frames: the first of them starts at pos -> (stream, content)"""
    f0 = parts["first_frame"]
    blob = f0 + skippable(pos - len(f0), fake_tail) + b"".join(parts["small"])
    return blob, parts["first"] + b"".join(parts["small_data"])


def check(gpu_lib, oracle, d, blob: bytes, want: bytes, what, shift: int = 0, before: bytes = b"", after: bytes = b"", serial: int = 0, use_oracle: bool = True):
    """decode blob from a device pointer `shift` bytes off 16-byte alignment, `before` and `after` lying right around it in the same tensor"""
    import torch
    front = FRONT + shift
    assert len(before) <= front
    raw = bytes(front - len(before)) + before + blob + after
    buf = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
    out = torch.zeros(len(want) + 64, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + front) % 16 == shift
    r = gpu_lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), len(want), buf.data_ptr() + front, len(blob))
    assert r == len(want), (what, r if r < (1 << 63) else gpu_lib.ZSTD_getErrorName(r))
    assert out[:len(want)].cpu().numpy().tobytes() == want, what
    assert gpu_lib.ZSTDMI_debugLastWalkSerial(d.dctx) == serial, (what, "parallel walk expected" if not serial else "serial walk expected")
    if use_oracle:
        ref = oracle.decompress(blob, max(len(want), 1))
        if not isinstance(ref, int):            # (where the oracle's decoder takes the stream at all)
            assert ref == want, what


# ------------------------------------------------------------------------------------------------------------------
# scan phase: the lane, group and window seams of every window size
# ------------------------------------------------------------------------------------------------------------------
PHASES = [range(-3, 4), range(12, 20), range(252, 260), range(1020, 1028), range(2044, 2052), range(4092, 4100), range(8188, 8196)]


@pytest.mark.parametrize("deltas", PHASES, ids=lambda r: f"delta{r[0]}to{r[-1]}")
def test_first_candidate_at_every_seam(gpu_lib, oracle, parts, dctx, deltas):
    for delta in deltas:
        blob, want = stream_with_magic_at(parts, SEG + delta)
        assert blob[SEG + delta:SEG + delta + 4] == ZSTD_MAGIC
        check(gpu_lib, oracle, dctx, blob, want, ("delta", delta))


# ------------------------------------------------------------------------------------------------------------------
# false candidates in front of the real frame
# ------------------------------------------------------------------------------------------------------------------
def fake_tail(g: int) -> bytes:
    if g < 4: return ZSTD_MAGIC[:g]                         # (see the module docstring)
    return ZSTD_MAGIC + (bytes([0x08]) + bytes(g - 5) if g > 4 else b"")     # FHD with the reserved bit set: no frame


@pytest.mark.parametrize("delta", [21, 1029, 4107])
@pytest.mark.parametrize("g", [1, 2, 3, 4, 5, 8, 15, 16, 17, "two"])
def test_false_candidates_before_the_frame(gpu_lib, oracle, parts, dctx, delta, g):
    tail = fake_tail(8) + fake_tail(8) if g == "two" else fake_tail(g)       # "two": fakes 16 and 8 bytes in front, one 16-byte piece
    blob, want = stream_with_magic_at(parts, SEG + delta, tail)
    p = SEG + delta
    assert blob[p:p + 4] == ZSTD_MAGIC and blob[p - len(tail):p] == tail and p - len(tail) >= SEG
    check(gpu_lib, oracle, dctx, blob, want, ("fake", g, delta))


# ------------------------------------------------------------------------------------------------------------------
# the ends of the input
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 7, 15])
@pytest.mark.parametrize("mod16", [1, 5, 9, 15])
def test_last_frame_in_the_last_16_bytes(gpu_lib, oracle, parts, dctx, shift, mod16):
    """The last segment's only frame start is an empty frame at the very end of an input of any size and alignment.  Complete valid
    frames lie right in front of the input and right behind it in the same tensor: the walk cannot fault there, so a read outside
    [src, src + srcSize) shows as a different frame count, result or walk."""
    total = SEG + 4096 + mod16
    assert total % 16 == mod16
    empty = raw_frame(b"")
    f0 = parts["first_frame"]
    blob = f0 + skippable(total - len(f0) - len(empty)) + empty
    assert len(blob) == total and len(empty) <= 16
    outside = raw_frame(b"outside the input: never to be decoded")
    check(gpu_lib, oracle, dctx, blob, parts["first"], ("end", mod16, shift), shift=shift, before=outside, after=outside + outside)


# ------------------------------------------------------------------------------------------------------------------
# scan rounds: many frames, many blocks, many segments
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_frames(oracle):
    texts = [datagen.gen("text", 400 + 31 * k, 70 + k) for k in range(8)]
    frames = [oracle.compress(t, 1, 0, 0) for t in texts]
    for t, f in zip(texts, frames):
        assert isinstance(f, bytes) and len(oracle.block_sequences(t, 1)[0]) > 0, "the frames must have sequences"
    return texts, frames


# (1024: a round of the scans as they were; 4096: a round of seq_scan and frame_rescan as they are)
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193])
def test_many_small_frames_with_sequences(gpu_lib, oracle, dctx, text_frames, n):
    texts, frames = text_frames
    order = [(7 * i + i // 8) % 8 for i in range(n)]
    blob = b"".join(frames[k] for k in order)
    want = b"".join(texts[k] for k in order)
    check(gpu_lib, oracle, dctx, blob, want, ("frames", n))


def test_frames_without_content_size_take_the_serial_walk_and_the_rescan(gpu_lib, oracle, dctx, text_frames):
    texts, frames = text_frames
    with z.Compressor(1) as c:
        c.SetParameter(200, 0)                              # ZSTD_c_contentSizeFlag
        unsized = [c.Wrap(t) for t in texts[:2]]
    n = 4200                                                # more frames than one round of frame_rescan
    blob, want = [], []
    for i in range(n):
        k = (5 * i) % 8
        if i % 3 == 1: blob.append(unsized[k % 2]); want.append(texts[k % 2])
        else: blob.append(frames[k]); want.append(texts[k])
    check(gpu_lib, oracle, dctx, b"".join(blob), b"".join(want), "unsized mixed in", serial=1)


# (1024 segments: a round of walk_link as it was; 2048: a round as it is)
@pytest.mark.parametrize("mib", [128, 256])
def test_more_segments_than_one_link_round(gpu_lib, dctx, mib):
    """GPU-built frames of random bytes (stored raw: about 64 KiB each), one frame more than `mib` MiB: just over mib x 8 segments"""
    import torch
    n = (mib << 20) + 65536
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    cap = gpu_lib.ZSTD_compressBound(n)
    comp = torch.empty(cap, dtype=torch.uint8, device="cuda"); out = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with z.Compressor(1) as c:
        cs = gpu_lib.ZSTDMI_compressDevice(c.cctx, comp.data_ptr(), cap, src.data_ptr(), n)
    assert n < cs < (1 << 63), cs
    assert (cs + SEG - 1) // SEG > mib * 8
    r = gpu_lib.ZSTDMI_decompressDevice(dctx.dctx, out.data_ptr(), n, comp.data_ptr(), cs)
    assert r == n, r if r < (1 << 63) else gpu_lib.ZSTD_getErrorName(r)
    assert torch.equal(out, src)
    assert gpu_lib.ZSTDMI_debugLastWalkSerial(dctx.dctx) == 0, "the parallel walk"
