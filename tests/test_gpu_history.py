"""GPU tests of cross-chunk history: blocks that match into the input in front of them, grouped into multi-block
frames — the window ZSTD_compress_frameChunk's block loop carries (U/ZstdCompress.cs:4705-4807).  The checker is the oracle's
decoder; the yardstick for size is the oracle's encoder on the same data with the same frame size."""
import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd.errors import is_error

pytestmark = pytest.mark.gpu

ZSTD_c_windowLog, ZSTD_c_checksumFlag = 101, 201


def walk_frames(lib, comp: bytes):
    """[(frame content size, [(block type, last, block size)...])] of a concatenation of single-segment frames"""
    out, pos = [], 0
    while pos < len(comp):
        fsz = lib.ZSTD_findFrameCompressedSize(comp[pos:], len(comp) - pos)
        assert not is_error(fsz)
        f = comp[pos:pos + fsz]
        fhd = f[4]
        assert (fhd >> 5) & 1, "single segment"
        did = (0, 1, 2, 4)[fhd & 3]
        fcs_bytes = (1, 2, 4, 8)[fhd >> 6]
        fcs = int.from_bytes(f[5 + did:5 + did + fcs_bytes], "little") + (256 if fcs_bytes == 2 else 0)
        p, blocks = 5 + did + fcs_bytes, []
        while True:
            bh = int.from_bytes(f[p:p + 3], "little")
            last, btype, bsz = bh & 1, (bh >> 1) & 3, bh >> 3
            blocks.append((btype, last, bsz))
            p += 3 + (1 if btype == 1 else bsz)
            if last:
                break
        assert p + (4 if fhd & 4 else 0) == fsz
        out.append((fcs, blocks))
        pos += fsz
    return out


def set_history(lib, c, hist, frame=0):
    assert lib.ZSTDMI_CCtx_setHistory(c.cctx, hist, frame) == 0


@pytest.mark.parametrize("level", [1, 3, 5])
@pytest.mark.parametrize("kind,n", [("text", 700001), ("mixed", 1 << 20), ("runs", 300000), ("zipf", 262144 + 5), ("period", 262144), ("rand", 200000),
                                    ("text", 65537), ("text", 32768 * 9)])
def test_history_frames_round_trip_under_both_decoders(gpu_lib, oracle, level, kind, n):
    data = datagen.gen(kind, n, 21)
    with z.Compressor(level) as c, z.Decompressor() as d:
        set_history(gpu_lib, c, 32 << 10)
        for chk in (0, 1):
            c.SetParameter(ZSTD_c_checksumFlag, chk)
            comp = c.Wrap(data)
            assert oracle.decompress(comp, n) == data, "the reference's decoder (oracle) must restore the input"
            assert d.Unwrap(comp) == data
            frames = walk_frames(gpu_lib, comp)
            assert sum(f[0] for f in frames) == n
            # 256 KiB of content per frame; the fast strategy keeps 64 KiB blocks (far candidates through its table), the others
            # take 32 KiB blocks behind 32 KiB of history in LDS; only the last block of a frame says so
            bs = 65536 if level < 3 else 32768
            assert all(f[0] == (256 << 10) for f in frames[:-1])
            for fcs, blocks in frames:
                assert len(blocks) == (fcs + bs - 1) // bs
                assert [b[1] for b in blocks] == [0] * (len(blocks) - 1) + [1]


def test_history_buys_ratio_on_text_and_stays_near_the_oracle_at_the_same_frame_size(gpu_lib, oracle):
    """Level 3 (dual-hash finder): with 32 KiB of the input in front of every block as history in LDS the frames shrink (matches
    reach back 32-64 KiB instead of 0-64 KiB); 48 KiB blocks with 16 KiB of history land in between."""
    data = datagen.gen("text", 2 << 20, 4)
    sizes = {}
    with z.Compressor(3) as c:
        for hist in (0, 16 << 10, 32 << 10):
            set_history(gpu_lib, c, hist)
            sizes[hist] = len(c.Wrap(data))
    assert sizes[32 << 10] < sizes[16 << 10] < sizes[0]
    assert sizes[32 << 10] <= 0.985 * sizes[0]
    ref = len(oracle.compress(data, 3, 0, 256 << 10))
    assert sizes[32 << 10] <= 1.09 * ref, (sizes, ref)


@pytest.mark.parametrize("kind", ["text", "pysrc"])
def test_fast_strategy_with_far_history_beats_independent_chunks(gpu_lib, oracle, kind):
    """Level 1 with cross-chunk history (64 KiB blocks, far candidates up to 188 KiB back through the block's table, 256 KiB
    frames) against independent chunks and against the oracle's level-1 output for the WHOLE input as one frame (window 512 KiB,
    U/Clevels.cs:22).  Measured: 2.4-2.7 % smaller than independent chunks; 6.5-10 % above the unchunked oracle — the table has
    8192 single-entry buckets filled at every position, so it remembers the last ~10 KiB well and the far history only while a
    block's first tiles have not overwritten it (what a global-memory table would buy).  The slack below is measured + 1 %."""
    if kind == "text":
        data = datagen.gen("text", 4 << 20, 6)
    else:                   # 4 MiB of CPython's standard library sources (tests/golden/make_pysrc.py)
        import hashlib, lzma, os
        data = lzma.decompress(open(os.path.join(os.path.dirname(__file__), "golden", "pysrc_4m.xz"), "rb").read())
        assert hashlib.sha256(data).hexdigest() == "4f4ad9c5e67f2b925dd24bc2d5d8ee185144c219368872e49f61095d8de5244d"
    with z.Compressor(1) as c, z.Decompressor() as d:
        plain = len(c.Wrap(data))
        set_history(gpu_lib, c, 32 << 10)
        comp = c.Wrap(data)
        assert oracle.decompress(comp, len(data)) == data and d.Unwrap(comp) == data
    ref = len(oracle.compress(data, 1, 0, 0))
    print(kind, "independent", plain / len(data), "history", len(comp) / len(data), "oracle unchunked", ref / len(data))
    assert len(comp) <= 0.98 * plain, (len(comp), plain)
    assert len(comp) <= (1.075 if kind == "text" else 1.11) * ref, (len(comp), ref, plain)


def test_history_is_on_by_level_and_by_window_log_and_off_with_a_dictionary(gpu_lib, oracle):
    data = datagen.gen("text", 600000, 8)

    def frame_sizes(c):
        return [f[0] for f in walk_frames(gpu_lib, c.Wrap(data))]

    with z.Compressor(1) as c:
        assert frame_sizes(c)[0] == 65536, "level 1 (fast strategy): independent 64 KiB frames, the throughput configuration"
        c.SetParameter(ZSTD_c_windowLog, 18)
        assert frame_sizes(c)[0] == (256 << 10), "a window above 64 KiB was asked for"
        c.SetParameter(ZSTD_c_windowLog, 16)
        assert frame_sizes(c)[0] == 65536
    with z.Compressor(5) as c:
        assert frame_sizes(c)[0] == (256 << 10), "greedy and above: eight 32 KiB blocks behind 32 KiB of history"
    with z.Compressor(3) as c:
        assert frame_sizes(c)[0] == 5 * (48 << 10), "strategies above fast (levels >= 3) carry history by default: doubleFast takes 48 KiB blocks behind 16 KiB"
        set_history(gpu_lib, c, 0)
        assert frame_sizes(c)[0] == 65536
        set_history(gpu_lib, c, -1)
        dic = datagen.gen("text", 20000, 8)
        c.LoadDictionary(dic)
        comp = c.Wrap(data)
        assert oracle.decompress(comp, len(data), dic) == data
        assert all(len(f[1]) == 1 for f in walk_frames(gpu_lib, comp)), "with a dictionary every chunk is its own frame behind the dictionary"


def test_history_frame_size_is_settable_and_frames_never_straddle_passes(gpu_lib, oracle):
    data = datagen.gen("text", (1 << 20) + 777, 9)
    with z.Compressor(3) as c, z.Decompressor() as d:
        set_history(gpu_lib, c, 32 << 10, 1 << 20)
        assert gpu_lib.ZSTDMI_CCtx_setPassChunks(c.cctx, 37) == 0          # not a multiple of the 32 blocks of a frame
        comp = c.Wrap(data)
        frames = walk_frames(gpu_lib, comp)
        assert [f[0] for f in frames] == [1 << 20, 777]
        assert oracle.decompress(comp, len(data)) == data and d.Unwrap(comp) == data
    with z.Compressor(1) as c:
        assert is_error(gpu_lib.ZSTDMI_CCtx_setHistory(c.cctx, 49 << 10, 0))
        assert is_error(gpu_lib.ZSTDMI_CCtx_setHistory(c.cctx, 0, 1000))


@pytest.mark.parametrize("level,hist", [(1, 0), (3, -1), (5, -1), (3, 0), (5, 0), (5, 16 << 10)])
@pytest.mark.parametrize("kind", ["text", "mixed", "pysrc"])
def test_region_parse_and_tile_loop_both_restore_the_input_and_never_lose_more_than_one_percent(gpu_lib, oracle, level, hist, kind):
    """ZSTDMI_CCtx_setParser: dense chunks are parsed region by region (one lane per 64 positions over precomputed candidates: the
    walk of U/ZstdFast.cs:130-260, at level >= 5 with the lazy step of U/ZstdLazy.cs:1836-1870) or by the tile loop like every
    other chunk.  Both are valid parses: the oracle's decoder restores the input from either, each is deterministic, and the
    sizes differ by well under one percent where both see the same candidates (levels below 5)."""
    n = (1 << 20) + 12345
    if kind == "pysrc":
        import inspect, collections, argparse, ast as _ast
        data = ("".join(inspect.getsource(m) for m in (collections, argparse, _ast, inspect)).encode() * 4)[:n]
        n = len(data)
    else:
        data = datagen.gen(kind, n, 33)
    sizes = {}
    with z.Compressor(level) as c, z.Decompressor() as d:
        set_history(gpu_lib, c, hist)
        for parser in (0, 1):
            assert gpu_lib.ZSTDMI_CCtx_setParser(c.cctx, parser) == 0
            comp = c.Wrap(data)
            assert comp == c.Wrap(data), "deterministic"
            assert oracle.decompress(comp, n) == data
            assert d.Unwrap(comp) == data
            sizes[parser] = len(comp)
        assert gpu_lib.ZSTDMI_CCtx_setParser(c.cctx, 2) != 0
    # (level >= 5: the region parse searches hash chains eight deep, the tile loop knows four candidates: it may only be smaller)
    assert sizes[0] <= 1.01 * sizes[1] and (level >= 5 or sizes[1] <= 1.01 * sizes[0]), sizes


def test_level5_and_9_search_deeper_and_stay_near_the_oracle_at_the_same_frame_size(gpu_lib, oracle):
    """Levels >= 5 (greedy / lazy behind a chain search, U/ZstdLazy.cs:619-760, 1743-2032): 1 << searchLog attempts per position —
    8 at levels 5-7, 32 at level 9 on 256 KiB frames (U/Clevels.cs:243-474), or what ZSTD_c_searchLog asks for.  More attempts
    never lose; the distance to the oracle's own level 5 at the same frame size is what the 64 KiB window costs."""
    data = datagen.gen("text", 2 << 20, 4)
    sizes = {}
    for level in (3, 5, 9):
        with z.Compressor(level) as c:
            comp = c.Wrap(data)
            assert oracle.decompress(comp, len(data)) == data
            sizes[level] = len(comp)
    with z.Compressor(5) as c:
        c.SetParameter(104, 5)                                   # ZSTD_c_searchLog
        sizes["5+sl5"] = len(c.Wrap(data))
    ref = len(oracle.compress(data, 5, 0, 256 << 10))
    print("level sizes", sizes, "oracle level 5, 256 KiB frames", ref, {k: round(v / ref, 4) for k, v in sizes.items()})
    assert sizes[5] <= 0.97 * sizes[3] and sizes[9] <= sizes[5] and sizes["5+sl5"] <= sizes[5]
    assert sizes[5] <= 1.09 * ref and sizes[9] <= 1.08 * ref, (sizes, ref)       # measured 1.069 / 1.058 (+ 2 %)


def test_search_log_buys_ratio_monotonically(gpu_lib, oracle):
    """ZSTD_c_searchLog at level 5: 1 << searchLog attempts down the hash chain (4 .. 32 used): every doubling may only shrink the
    output (a longer match among more candidates), and all of them decode under the oracle."""
    data = datagen.gen("text", 1 << 20, 9)
    sizes = []
    with z.Compressor(5) as c:
        for sl in (2, 3, 4, 5):
            c.SetParameter(104, sl)
            comp = c.Wrap(data)
            assert oracle.decompress(comp, len(data)) == data
            sizes.append(len(comp))
    assert sizes == sorted(sizes, reverse=True) and sizes[-1] < sizes[0], sizes


def test_levels_above_2_fall_back_to_level_1_where_a_match_finder_finds_nothing(gpu_lib, oracle):
    """on Zipf bytes level >= 3 must not be both slower and larger than level 1.  A call of 4 MiB or more that leaves
    strategy, window and history to the level samples 64 tiles of the input first (lz_probe_kernel); where next to nothing repeats,
    level 1's finder and framing take the call: byte-identical to level 1.  Dense input, smaller calls and calls that set the
    history themselves keep the level's own path."""
    n = 4 << 20
    for kind, falls_back in (("zipf", True), ("rand", True), ("text", False), ("mixed", False), ("runs", False)):
        data = datagen.gen(kind, n, 17)
        with z.Compressor(1) as c1, z.Compressor(5) as c5, z.Compressor(3) as c3:
            a, b, c = c1.Wrap(data), c5.Wrap(data), c3.Wrap(data)
            assert oracle.decompress(b, n) == data and oracle.decompress(c, n) == data
            assert (a == b) == falls_back and (a == c) == falls_back, kind
            if falls_back:
                set_history(gpu_lib, c5, 32 << 10)              # asked for explicitly: multi-block frames whatever the data
                forced = c5.Wrap(data)
                assert forced != a and oracle.decompress(forced, n) == data
                assert walk_frames(gpu_lib, forced)[0][0] == (256 << 10)
        small = data[:(4 << 20) - 65536]                       # below the probe's floor: the level's own framing
        with z.Compressor(5) as c5:
            fr = walk_frames(gpu_lib, c5.Wrap(small))
            assert len(fr[0][1]) == 8, "256 KiB frames of eight 32 KiB blocks"


def test_a_long_stretch_without_matches_inside_a_call_is_compressed_as_level_1_would(gpu_lib, oracle):
    """The sampling works per group of 16 frames; a stretch of 8 MiB or more without matches becomes a range of its own (level 1's
    finder and framing), the rest keeps the level: the output is the concatenation of what the parts give on their own — also when
    the kinds alternate (the ranges of a kind are compressed together and their pieces put back in the input's order).
    Shorter stretches stay with their surroundings."""
    sparse = datagen.gen("zipf", 72 << 20, 5)
    dense = datagen.gen("text", 8 << 20, 6)
    with z.Compressor(5) as c5, z.Compressor(1) as c1:
        whole = c5.Wrap(sparse + dense)
        assert whole == c1.Wrap(sparse) + c5.Wrap(dense)
        assert oracle.decompress(whole, len(sparse) + len(dense)) == sparse + dense
        # alternating kinds, pieces of 40 MiB (parameters are resolved for the call's size: every piece above the 32 MiB of small calls)
        a, b, c2, d2 = sparse[:40 << 20], datagen.gen("text", 40 << 20, 7), datagen.gen("rand", 40 << 20, 8), datagen.gen("text", (40 << 20) + 12345, 9)
        mixed = a + b + c2 + d2
        out = c5.Wrap(mixed)
        assert out == c1.Wrap(a) + c5.Wrap(b) + c1.Wrap(c2) + c5.Wrap(d2)
        with z.Decompressor() as d:
            assert d.Unwrap(out) == mixed
        short = datagen.gen("zipf", 4 << 20, 5) + dense                # 4 MiB of it: one range, the level's own path throughout
        out = c5.Wrap(short)
        assert out != c1.Wrap(short[:4 << 20]) + c5.Wrap(dense)
        assert walk_frames(gpu_lib, out)[0][0] == (256 << 10) and len(walk_frames(gpu_lib, out)[0][1]) == 8


@pytest.mark.parametrize("kind,n", [("text", 10 << 20), ("mixed", 3 << 20), ("text", 65537), ("runs", 200000), ("zipf", 1 << 20), ("text", (32 << 20))])
def test_small_calls_get_short_blocks_in_64_kib_frames(gpu_lib, oracle, kind, n):
    """Level 1, 64 KiB < size <= 32 MiB, everything left to the level: frames stay 64 KiB (match execution is ordered per frame) but
    hold four 16 KiB blocks, each matching into the frame's earlier blocks — four times as many serial chains (tANS, Huffman) a
    quarter as long, which is what a call of this size waits for.  The price in size against single-block 64 KiB frames is small
    (block header, Huffman table and the unknown-repcode start per 16 KiB); calls above 32 MiB keep single-block frames."""
    data = datagen.gen(kind, n, 17)
    with z.Compressor(1) as c, z.Decompressor() as d:
        comp = c.Wrap(data)
        set_history(gpu_lib, c, 0)
        single = c.Wrap(data)
    assert oracle.decompress(comp, n) == data
    with z.Decompressor() as d:
        assert d.Unwrap(comp) == data
    frames = walk_frames(gpu_lib, comp)
    assert all(f[0] == 65536 for f in frames[:-1]) and sum(f[0] for f in frames) == n
    for fcs, blocks in frames:
        assert len(blocks) == (fcs + 16383) // 16384 and [b[1] for b in blocks] == [0] * (len(blocks) - 1) + [1]
    print(f"small call {kind} {n}: 16 KiB blocks {len(comp)} vs single-block frames {len(single)} = {len(comp) / len(single):.4f}")
    assert len(comp) <= len(single) * (1.03 if kind != "runs" else 1.10), (len(comp), len(single))
    big = datagen.gen("text", (32 << 20) + 65536, 17) if kind == "text" and n == (32 << 20) else None
    if big is not None:
        with z.Compressor(1) as c:
            fr = walk_frames(gpu_lib, c.Wrap(big))
        assert all(len(b) == 1 for _, b in fr), "above 32 MiB: one block per frame"
