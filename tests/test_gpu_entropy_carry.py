"""GPU tests of ZSTDMI_CCtx_setEntropyCarry: with the switch on, the blocks of a multi-block frame are coded in order inside carry
groups of 8 and may reuse the Huffman table (treeless literals), the FSE tables (repeat mode) and the repcodes the blocks before them
left in the decoder.  Every frame written here goes through the state checker of tests/zstd_blocks.py (nothing is used before it was
defined, a group's first block uses nothing carried) and is decoded, bit-exact, by the oracle's decoder and by this library in both
match-execution modes; every door writes the same bytes; and a context that leaves the switch off, or a call the switch does not
apply to, writes what it wrote before.  Everything goes through the C ABI or its Python mirrors."""
import ctypes
import functools
import lzma
import os

import pytest

import datagen
import oracle_lib
import zstd_blocks as zb
import zstdsharp_amd as z
from zstdsharp_amd.compressor import ZSTD_c_enableLongDistanceMatching as ZSTD_c_ldm
from zstdsharp_amd.errors import get_error_code, is_error
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer, ZSTD_e_end, ZSTD_e_flush

pytestmark = pytest.mark.gpu

ZSTD_c_windowLog, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 101, 200, 201
KiB, MiB = 1 << 10, 1 << 20
GROUP = 8                           # kCarryGroup (zmi_carry.h)
W17 = {ZSTD_c_windowLog: 17}        # level 1 with history: frames of two 64 KiB blocks
B3 = 48 * KiB                       # level 3's block
# "pysrc" is the whole fixture, one byte under the sparse-input probe's 4 MiB threshold (the framing stays the level's own).  Source
# code brings new byte values with nearly every block, and a Huffman table without a code for one of a block's literals cannot be
# reused: of the 31 blocks behind a group's first in the fixture's first MiB at level 5, one has its alphabet covered by the block
# before it (text: 28 of 28), and that one pays less for a tree of its own — a prefix that short has no treeless block to show.
PYSRC = 4 * MiB - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------- inputs ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gen(kind, n, seed=5):
    if kind == "pysrc":             # CPython's standard library sources (tests/golden/make_pysrc.py)
        return lzma.decompress(open(os.path.join(GOLDEN, "pysrc_4m.xz"), "rb").read())[:n]
    return datagen.gen(kind, n, seed)


@functools.lru_cache(maxsize=None)
def no_match_piece(n):
    """n bytes without a repeated 3-gram (a de Bruijn sequence over 40 byte values no text holds): no finder has a match in it, and
    its literals are worth a Huffman table"""
    k, order = 40, 3
    a, seq = [0] * (k * order), []

    def db(t, p):
        if t > order:
            if order % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    assert len(seq) == k ** order >= n
    return bytes(128 + v for v in seq[:n])


@functools.lru_cache(maxsize=None)
def records(n):
    """100-byte records, each the one before with one byte changed: every match lies exactly 100 bytes back"""
    import random
    rnd = random.Random(3)
    rec = bytearray(rnd.randrange(256) for _ in range(100))
    out = bytearray()
    i = 0
    while len(out) < n:
        rec[(7 * i) % 100] = rnd.randrange(256)
        out += rec
        i += 1
    return bytes(out[:n])


# ---------------------------------------------------------------- helpers ----------------------------------------------------------------
def compressor(level, carry, params=None, single=False, pass_chunks=None):
    c = z.Compressor(level)
    for k, v in (params or {}).items():
        c.SetParameter(k, v)
    if single:
        c.single_frame = True
    if pass_chunks:
        assert c._lib.ZSTDMI_CCtx_setPassChunks(c.cctx, pass_chunks) == 0
    if carry is not None:           # (None: a context that never heard of the switch)
        c.entropy_carry = carry
    return c


def wrap(level, data, carry, **kw):
    """-> (bytes, carry groups the call walked)"""
    with compressor(level, carry, **kw) as c:
        blob = c.Wrap(data)
        return blob, c._lib.ZSTDMI_debugLastCarryGroups(c.cctx)


def decodes_everywhere(lib, blob, data, prefix=None):
    assert oracle_lib.decompress(blob, len(data), dict_bytes=prefix) == data, "the oracle's decoder must restore the input"
    for mode in (1, 2):             # walk and origin modes of the match execution
        with z.Decompressor() as d:
            assert lib.ZSTDMI_DCtx_setLongFrames(d.dctx, mode) == 0
            if prefix is not None:
                d.RefPrefix(prefix)
            assert d.Unwrap(blob, maxDecompressedSize=1 << 30) == data, f"the GPU decoder (long frames {mode}) must restore the input"


def structure(blob, group=GROUP):
    """the state checker over every frame -> (frames' block lists, carry groups counted from them)"""
    frames = zb.check_stream_state(blob, group)
    return frames, sum(zb.carry_groups(f, group) for f in frames)


def shares(frames):
    blocks = [b for f in frames for b in f]
    return sum(b.treeless for b in blocks), sum(b.repeats for b in blocks)


# ---------------------------------------------------------------- 1. round trip and structure ----------------------------------------------------------------
INPUTS = [("text", 300001), ("mixed", MiB), ("pysrc", PYSRC), ("runs", 300000), ("zipf", 262149), ("period", 262144), ("rand", 200000)]
LEVELS = [(1, W17), (3, None), (5, None), (9, None)]


@pytest.mark.parametrize("level, params", LEVELS, ids=["L1w17", "L3", "L5", "L9"])
@pytest.mark.parametrize("kind, n", INPUTS, ids=[k for k, _ in INPUTS])
def test_round_trip_and_structure(gpu_lib, kind, n, level, params):
    data = gen(kind, n)
    on, groups = wrap(level, data, True, params=params)
    off, none = wrap(level, data, False, params=params)
    frames, counted = structure(on)
    assert groups == counted > 0, "the counter equals the groups the parser counts"
    assert none == 0
    treeless, repeats = shares(frames)
    print(f"{kind} {n} L{level}: off {len(off)} on {len(on)} blocks {sum(map(len, frames))} treeless {treeless} repeated tables {repeats}")
    assert shares(zb.check_stream_state(off)) == (0, 0), "with the switch off: neither treeless literals nor repeat mode anywhere"
    if kind in ("text", "pysrc") and level in (3, 5):
        assert treeless >= 1 and repeats >= 1
    decodes_everywhere(gpu_lib, on, data)


# ---------------------------------------------------------------- 2. smallest frames ----------------------------------------------------------------
@pytest.mark.parametrize("n", [B3 + 1, 2 * B3, B3 + 64, 64 * KiB + 1, 2 * B3 + 1])
def test_smallest_frames_level_3(gpu_lib, n):
    """Up to 64 KiB a call is ONE block whatever the level (48 KiB + 1 and 48 KiB + 64 bytes: the switch changes nothing); above it
    level 3 cuts 48 KiB blocks: two whole ones, 48 + 16 KiB, and two with a block of one byte — under 7 bytes, stored raw — behind them."""
    data = gen("text", n)
    on, groups = wrap(3, data, True)
    frames, counted = structure(on)
    assert len(frames) == 1
    if n <= 64 * KiB:
        assert len(frames[0]) == 1 and groups == 0 and on == wrap(3, data, None)[0]
    else:
        assert len(frames[0]) == (n + B3 - 1) // B3 and groups == counted == 1
    if n == 2 * B3 + 1:
        assert frames[0][2].type == 0 and frames[0][2].size == 1, "a block under 7 bytes is stored raw"
    decodes_everywhere(gpu_lib, on, data)


# ---------------------------------------------------------------- 3. group boundaries ----------------------------------------------------------------
def test_single_frame_block_8_leads_a_group(gpu_lib):
    data = gen("text", 9 * B3 + 5)
    on, groups = wrap(3, data, True, single=True)
    frames, counted = structure(on)                 # (the checker refuses anything carried into the block with index 8)
    assert len(frames) == 1 and len(frames[0]) == 10 and groups == counted == 2
    assert any(b.carried for b in frames[0][1:8]) and not frames[0][8].carried
    decodes_everywhere(gpu_lib, on, data)


def test_long_distance_frame_is_cut_into_groups(gpu_lib):
    data = gen("text", 600 * KiB)
    on, groups = wrap(3, data, True, params={ZSTD_c_ldm: 1, ZSTD_c_windowLog: 20})
    frames, counted = structure(on)
    assert len(frames) == 1 and len(frames[0]) == 13 and groups == counted == 2
    assert any(b.carried for b in frames[0])
    decodes_everywhere(gpu_lib, on, data)


def test_prefix_long_form(gpu_lib):
    prefix, data = gen("text", 200 * KiB, 8), gen("text", 200 * KiB, 9)
    with compressor(3, True) as c:
        c.RefPrefix(prefix)
        on = c.Wrap(data)
        groups = c._lib.ZSTDMI_debugLastCarryGroups(c.cctx)
    frames, counted = structure(on)
    assert len(frames) == 1 and groups == counted == 1 and len(frames[0]) == 5
    decodes_everywhere(gpu_lib, on, data, prefix=prefix)


# ---------------------------------------------------------------- 4. what an earlier block leaves behind ----------------------------------------------------------------
def glued(*pieces):
    return b"".join(pieces)


def text_piece(seed):
    return gen("text", B3, seed)


def one_frame(gpu_lib, data):
    on, _ = wrap(3, data, True)
    frames, _ = structure(on)
    assert len(frames) == 1
    decodes_everywhere(gpu_lib, on, data)
    return frames[0]


def test_behind_a_raw_first_block(gpu_lib):
    blocks = one_frame(gpu_lib, glued(gen("rand", B3), text_piece(1), text_piece(2)))
    assert blocks[0].type == 0, "void: the random piece was meant to come out raw"
    assert not blocks[1].carried, "behind a raw block that leads the group there is nothing to carry"
    assert blocks[1].type == 2 and blocks[2].type == 2


def test_across_a_raw_block(gpu_lib):
    blocks = one_frame(gpu_lib, glued(text_piece(1), gen("rand", B3), text_piece(2), text_piece(3)))
    assert blocks[1].type == 0, "void: the random piece was meant to come out raw"
    assert [b.type for b in blocks] == [2, 0, 2, 2]


def test_across_a_block_of_one_byte(gpu_lib):
    blocks = one_frame(gpu_lib, glued(text_piece(1), b"\x5A" * B3, text_piece(2)))
    assert blocks[1].type == 2 and blocks[1].lit_type in (0, 1), "void: the run was meant to leave the Huffman table alone"
    assert blocks[2].type == 2


def test_across_a_block_without_sequences(gpu_lib):
    blocks = one_frame(gpu_lib, glued(text_piece(1), no_match_piece(B3), text_piece(2)))
    assert blocks[1].type == 2 and blocks[1].nb_seq == 0 and blocks[1].lit_type == 2, "void: the piece was meant to have Huffman literals and no sequence"
    assert blocks[2].type == 2


def test_across_a_block_of_few_literals(gpu_lib):
    first = text_piece(1)
    blocks = one_frame(gpu_lib, glued(first, first[-KiB:] * 48, text_piece(2)))
    assert blocks[1].type == 2 and blocks[1].lit_type == 0 and blocks[1].lit_size <= 63 and blocks[1].nb_seq > 0, \
        "void: the repeated pattern was meant to leave at most 63 literals"
    assert blocks[2].type == 2


# ---------------------------------------------------------------- 5. repcodes ----------------------------------------------------------------
@pytest.mark.parametrize("level, params", [(1, W17), (3, None), (5, None)], ids=["L1w17", "L3", "L5"])
def test_fixed_stride_records(gpu_lib, level, params):
    data = records(300 * KiB)
    on, groups = wrap(level, data, True, params=params)
    off, _ = wrap(level, data, False, params=params)
    _, counted = structure(on)
    assert groups == counted
    print(f"records L{level}: off {len(off)} on {len(on)}")
    assert len(on) <= len(off)
    decodes_everywhere(gpu_lib, on, data)


# ---------------------------------------------------------------- 6. size, on named inputs ----------------------------------------------------------------
@pytest.mark.parametrize("kind, n, level, single", [("text", MiB, 3, False), ("text", MiB, 5, False), ("pysrc", PYSRC, 3, False), ("pysrc", PYSRC, 5, False),
                                                    ("text", 10 * MiB, 1, False), ("text", MiB, 3, True)])
def test_smaller_on_named_inputs(gpu_lib, kind, n, level, single):
    data = gen(kind, n)
    on, groups = wrap(level, data, True, single=single)
    off, _ = wrap(level, data, False, single=single)
    frames, counted = structure(on)
    assert groups == counted
    print(f"{kind} {n} L{level} single {single}: off {len(off)} on {len(on)} ({len(on) / len(off):.4f}) treeless / repeated tables {shares(frames)}")
    assert len(on) < len(off)
    if n <= 4 * MiB:
        decodes_everywhere(gpu_lib, on, data)
    else:
        with z.Decompressor() as d:
            assert d.Unwrap(on, maxDecompressedSize=n) == data
        assert oracle_lib.decompress(on, n) == data


# ---------------------------------------------------------------- 7. same bytes through every door ----------------------------------------------------------------
def test_same_bytes_through_every_door(gpu_lib):
    import torch
    lib = gpu_lib
    data = gen("text", 700001)
    ref, groups = wrap(3, data, True)
    assert groups == structure(ref)[1]
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    # ZSTDMI_compressDevice
    with compressor(3, True) as c:
        cap = lib.ZSTD_compressBound(len(data))
        dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r = lib.ZSTDMI_compressDevice(c.cctx, dst.data_ptr(), cap, src.data_ptr(), len(data))
        assert not is_error(r), get_error_code(r)
        assert dst[:r].cpu().numpy().tobytes() == ref
        assert lib.ZSTDMI_debugLastCarryGroups(c.cctx) == groups
    # the batch, with that buffer among short ones (entries of one block carry nothing; the long one's groups come from a leader list)
    with compressor(3, True) as c:
        items = [data[:100], data, data[:50000], data[:B3 + 1], data[:300000]]
        got = z.compress_batch(c, items)
        assert lib.ZSTDMI_debugLastBatchAlone(c.cctx) == 0
        batch_groups = lib.ZSTDMI_debugLastCarryGroups(c.cctx)
    want = [wrap(3, it, True) for it in items]
    assert [bytes(g) for g in got] == [w[0] for w in want]
    assert batch_groups == sum(w[1] for w in want)
    # device 0 listed twice: two workers, each with its share of the frames
    with compressor(3, True) as c:
        assert lib.ZSTDMI_CCtx_setDevices(c.cctx, (ctypes.c_int * 2)(0, 0), 2) == 0
        assert c.Wrap(data) == ref
        assert lib.ZSTDMI_debugLastCarryGroups(c.cctx) == groups
    # the default framing in passes of one frame each (7 chunks asked for: whole frames of 5 blocks)
    short, g0 = wrap(3, data, True, pass_chunks=7)
    assert short == ref and g0 == groups
    # a pack: every item's frames as the single call writes them, one seek table behind the last
    with compressor(3, True) as c:
        pack = z.compress_pack(c, [data, data[:300000]])
        assert lib.ZSTDMI_debugLastCarryGroups(c.cctx) == groups + 2
    assert b"".join(zb.frames_of(pack)) == ref + wrap(3, data[:300000], True)[0]
    # one frame: the bytes do not depend on the passes
    whole, g1 = wrap(3, data, True, single=True)
    cut, g2 = wrap(3, data, True, single=True, pass_chunks=2 * GROUP)
    assert cut == whole and g1 == g2 == structure(whole)[1]
    odd, _ = wrap(3, data, True, single=True, pass_chunks=2 * GROUP + 3)     # (rounded down to whole groups)
    assert odd == whole
    decodes_everywhere(lib, whole, data)


@pytest.mark.parametrize("single", [False, True])
def test_stream_round_trip_and_structure(gpu_lib, single):
    """ZSTD_compressStream2 in batches of 200000 bytes (ZSTD_e_flush).  Without the single frame every batch is a call of its own; with
    it a batch continues the ONE frame and ends a carry group where it ends — 200000 is no multiple of the block, so where the groups
    begin cannot be told from the frame, and the checker asks only what the format asks."""
    lib = gpu_lib
    data = gen("text", 700001)
    blob = bytearray()
    room = ctypes.create_string_buffer(1 << 20)
    with compressor(3, True, single=single) as c:
        for at in range(0, len(data), 200000):
            piece = data[at:at + 200000]
            keep = ctypes.create_string_buffer(piece, len(piece))
            inp = ZSTD_inBuffer(ctypes.addressof(keep), len(piece), 0)
            op = ZSTD_e_end if at + 200000 >= len(data) else ZSTD_e_flush
            while True:
                out = ZSTD_outBuffer(ctypes.addressof(room), len(room), 0)
                left = lib.ZSTD_compressStream2(c.cctx, ctypes.byref(out), ctypes.byref(inp), op)
                assert not is_error(left), get_error_code(left)
                blob += room.raw[:out.pos]
                if left == 0 and inp.pos == inp.size:
                    break
            assert lib.ZSTDMI_debugLastCarryGroups(c.cctx) > 0
    blob = bytes(blob)
    frames = zb.check_stream_state(blob, None if single else GROUP)
    assert (len(frames) == 1) == single
    assert any(b.carried for f in frames for b in f)
    decodes_everywhere(lib, blob, data)


# ---------------------------------------------------------------- 8. changes nothing ----------------------------------------------------------------
def same_with_and_without(make, run):
    """run(compressor) with a context that never set the switch and with one that has it on -> equal bytes, no group walked"""
    with make() as c:
        plain = run(c)
    with make() as c:
        c.entropy_carry = True
        on = run(c)
        assert c._lib.ZSTDMI_debugLastCarryGroups(c.cctx) == 0
    assert on == plain
    return plain


def test_changes_nothing_where_blocks_are_frames_of_their_own(gpu_lib):
    lib = gpu_lib
    text = gen("text", 300001)

    def independent_frames():
        c = z.Compressor(1)
        assert lib.ZSTDMI_CCtx_setHistory(c.cctx, 0, 0) == 0
        return c
    same_with_and_without(independent_frames, lambda c: c.Wrap(text))
    same_with_and_without(lambda: z.Compressor(3), lambda c: c.Wrap(text[:50000]))                                   # one block
    same_with_and_without(lambda: compressor(3, None, params={ZSTD_c_windowLog: 12}), lambda c: c.Wrap(text))       # independent windows


def test_changes_nothing_behind_a_dictionary(gpu_lib):
    text = gen("text", 300001)
    raw_dict = gen("text", 20000, 77)
    trained = open(os.path.join(GOLDEN, "trained_16k.dict"), "rb").read()

    def with_dict(d):
        def make():
            c = z.Compressor(3)
            c.LoadDictionary(d)
            return c
        return make
    same_with_and_without(with_dict(raw_dict), lambda c: c.Wrap(text))
    same_with_and_without(with_dict(trained), lambda c: c.Wrap(text))
    with z.CDict(trained, 3) as cd:
        def ref(c):
            c.RefCDict(cd)
            return c.Wrap(text)
        same_with_and_without(lambda: z.Compressor(3), ref)
        same_with_and_without(lambda: z.Compressor(3), lambda c: [bytes(b) for b in z.compress_batch(c, [text, text[:70000]], cdicts=[cd, cd])])


def test_changes_nothing_in_level_only_and_sample_calls(gpu_lib):
    lib = gpu_lib
    text = gen("text", 300001)

    def compress_cctx(c):
        cap = lib.ZSTD_compressBound(len(text))
        out = ctypes.create_string_buffer(cap)
        r = lib.ZSTD_compressCCtx(c.cctx, out, cap, text, len(text), 3)
        assert not is_error(r)
        return out.raw[:r]

    def samples(c):
        sizes = [70000, 150000, 80001]
        got = (ctypes.c_size_t * 3)()
        r = lib.ZSTDMI_debugCompressSamples(c.cctx, text, (ctypes.c_size_t * 3)(*sizes), 3, got)
        assert not is_error(r)
        return list(got)
    same_with_and_without(lambda: z.Compressor(3), compress_cctx)
    same_with_and_without(lambda: z.Compressor(3), samples)
    # on and off again
    plain, _ = wrap(3, text, None)
    with z.Compressor(3) as c:
        c.entropy_carry = True
        c.entropy_carry = False
        assert c.Wrap(text) == plain and lib.ZSTDMI_debugLastCarryGroups(c.cctx) == 0
        c.entropy_carry = True
        assert c.Wrap(text) != plain and lib.ZSTDMI_debugLastCarryGroups(c.cctx) > 0
        assert c.Wrap(text[:1000]) and lib.ZSTDMI_debugLastCarryGroups(c.cctx) == 0      # the counter speaks of the last call


# ---------------------------------------------------------------- 9. flags ----------------------------------------------------------------
@pytest.mark.parametrize("params", [{ZSTD_c_checksumFlag: 1}, {ZSTD_c_contentSizeFlag: 0}], ids=["checksum", "no-content-size"])
def test_frame_flags(gpu_lib, params):
    data = gen("text", 700001)
    on, groups = wrap(3, data, True, params=params)
    frames, counted = structure(on)
    assert groups == counted and shares(frames)[0] > 0
    decodes_everywhere(gpu_lib, on, data)


def test_seek_table_and_ranges_over_carried_blocks(gpu_lib):
    data = gen("text", 700001)
    with compressor(3, True) as c:
        c.seek_table = True
        blob = c.Wrap(data)
    frames, _ = structure(blob)
    assert len(frames) == 3 and any(b.carried for f in frames for b in f)
    with z.Decompressor() as d:
        for off, n in ((0, 1000), (240 * KiB - 7, 100), (300000, 250000), (700000, 1)):
            assert bytes(d.unwrap_range(blob, off, n)) == data[off:off + n]


def test_entropy_stage_bounds_a_poisoned_record_behind_carried_state(gpu_lib):
    """ZSTDMI_debugPoisonedChunk with the switch on files the record twice, as the two blocks of one frame, and the carry instance codes
    the second behind whatever the first left: garbage in, a bounded size out, and the context still works"""
    data = gen("text", 300001)
    with compressor(3, True) as c:
        for nbSeq, litSize, srcSize, fill in ((16384, 65536, 65536, 0xFF), (0xFFFFFFFF, 5, 65536, 0x00), (100, 0xFFFFFFFF, 65536, 0xA5),
                                              (16384, 0, 65536, 0xFF), (7, 7, 0xFFFFFFFF, 0x5A), (20000, 70000, 65536, 0x11), (16384, 65536, 65536, 0x80)):
            r = gpu_lib.ZSTDMI_debugPoisonedChunk(c.cctx, nbSeq, litSize, srcSize, fill)
            assert not is_error(r), (nbSeq, litSize, srcSize, fill, get_error_code(r))
            assert r <= 65536 + 512, r
        blob = c.Wrap(data)
    structure(blob)
    assert oracle_lib.decompress(blob, len(data)) == data
