"""The smallest inputs that reach each edge of the long-distance stage (zstdsharp_amd/csrc/ldm.hip), for tests/ldm_model.py and the
exact GPU check in tests/test_gpu_ldm_model.py.  No GPU and no oracle here; tests/test_ldm_model_cpu.py proves every claim of the table.

A case is a dict:
  name, level, wlog (ZSTD_c_windowLog, 0 = unset), mm / hlog / blog / hrl (the four ZSTD_c_ldm* parameters, always set),
  history (ZSTDMI_CCtx_setHistory bytes, None = the level's), pass_chunks (ZSTDMI_CCtx_setPassChunks, None = default),
  prefix (bytes, None = none), sliding (single frame + sliding window), data (bytes),
  labels: labels of ldm_model.stage() the case must reach, absent: labels it must NOT reach (a copy that must not be matched),
  merge: True for the cases whose merged blocks matter (their finder output is not quiet)
framing(case) restates resolve_framing / ldm_resolve for these settings: the model's Layout and Params of the call's LAST pass and
the bytes the stage sees there (what lies in front of the pass, then the pass).

Inputs are seeded random bytes with planted copies: the block finders find nothing in them, so F is empty wherever it does not
matter.  A copy's exact lengths are cut with the model in the loop (plant, look where the first searching split of the copy falls,
then put the mismatches where the wanted forward and backward lengths end): the construction is deterministic, the seeds are below.
"""
import numpy as np

import datagen
import ldm_model as lm

KiB = 1024
CHUNK = {1: 64 * KiB, 3: 48 * KiB, 5: 32 * KiB}        # bytes per block at windowLog >= 17: fast: whole blocks; 16 / 32 KiB of history


def rnd(n, seed):
    return bytearray(np.random.RandomState(seed).bytes(n))


def framing(case):
    """-> (Layout, Params, buf): the last pass of the call in the stage's coordinate"""
    data, level = case["data"], case["level"]
    chunk = CHUNK[level]
    if case.get("history") is not None and level != 1:
        chunk = 64 * KiB - ((case["history"] + 4095) & ~4095)
    n = len(data)
    pfx = case.get("prefix")
    if pfx:
        wl = 17
        while (1 << wl) < len(pfx) + n: wl += 1
        size = len(pfx) + n
    else:
        wl, size = case["wlog"], n
    need = 10
    while (1 << need) < size: need += 1
    wl = min(wl, need)
    hlog = case["hlog"] or (wl - 7 if wl > 13 else 6)
    blog = min(case["blog"] or 3, hlog)
    hrl = max(case["hrl"] or (wl - hlog if wl > hlog else 0), 5)
    p = lm.Params(case["mm"] or 64, hlog, blog, hrl)
    if pfx:
        base = (len(pfx) + 16383) // 16384 * 16384
        vlo = base - len(pfx)
        return lm.Layout(base + n, base, vlo, 0, chunk, 0), p, bytes(vlo) + bytes(pfx) + bytes(data)
    if case.get("sliding"):
        pc = case["pass_chunks"] * chunk
        at = (n - 1) // pc * pc
        keep = min(at, 1 << case["wlog"])
        base = (keep + 16383) // 16384 * 16384
        vlo = base - keep
        return lm.Layout(base + n - at, base, vlo, 0, chunk, 1 << case["wlog"]), p, bytes(vlo) + bytes(data[at - keep:])
    blocks = max((1 << case["wlog"]) // chunk, 2)
    return lm.Layout(n, 0, 0, blocks * chunk, chunk, 0), p, bytes(data)


def case(name, data, labels=(), level=1, wlog=17, mm=64, hlog=14, blog=3, hrl=7, absent=(), **kw):
    c = dict(name=name, data=bytes(data), labels=tuple(labels), absent=tuple(absent), level=level, wlog=wlog, mm=mm, hlog=hlog, blog=blog,
             hrl=hrl, history=None, pass_chunks=None, prefix=None, sliding=False, merge=False)
    c.update(kw)
    return c


def copy(d, dst, src, n):
    d[dst:dst + n] = d[src:src + n]


def cut_lengths(d, settings, dst, src, n, fwd, back, seed):
    """d[dst:dst+n] is a copy of d[src:src+n]: cut it so that its first searching split has exactly `fwd` bytes forward and `back`
    backward.  The split is one with no other split in the `back` bytes in front of it; what lies further in front is replaced (a
    byte changes the gear hash of the next 64 positions only, so neither that split nor the gap in front of it moves)."""
    lay, p, buf = framing(case("tmp", d, **settings))
    pos = lm.splits(buf, lay, p)[0][0]
    for w in pos:
        if dst + back + 1 <= w and w + fwd < dst + n and not any(w - back <= v < w for v in pos):
            break
    else:
        raise AssertionError("no split of the copy at %d has %d free bytes in front" % (dst, back))
    d[dst:w - back] = rnd(w - back - dst, seed)
    d[w - back - 1] = d[w - back - 1 - dst + src] ^ 0x55
    d[w + fwd] = d[w + fwd - dst + src] ^ 0x55


def force_stop(d, a, k, mm, hrl, seed, warm_stops=False):
    """write k + 1 bytes at the frame start a, so that the gear hash that starts from 0 at a stops at a + k, and one warmed up on the
    64 bytes in front of a does not (warm_stops: the other way round) -> the restart shows in the splits"""
    mask = lm.stop_mask(lm.Params(mm, 0, 0, hrl))
    r = np.random.RandomState(seed)
    while True:
        t = r.bytes(k + 1)
        cold = lm._stops_loop(t, 0, k + 1, mask)
        warm = lm._stops_loop(bytes(d[a - 64:a]) + t, 0, 64 + k + 1, mask)
        if ((k in cold) != warm_stops) and ((64 + k in warm) == warm_stops):
            d[a:a + k + 1] = t
            return


def _min_match_cases():
    out = []
    for mm, hrl in ((4, 5), (16, 7), (63, 7), (64, 7), (65, 7), (1024, 7), (4096, 7)):
        d = rnd(256 * KiB, 100 + mm)
        n = mm + 700
        a = 3000                                     # the planted content: in the middle of a tile ...
        copy(d, 40000, a, n)
        # ... and where the windows of its first splits start in front of the tile the splits end in (by more than 64 from minMatch 129 on)
        copy(d, 3 * 16384 - mm - 100 + 60, a, n)
        copy(d, 131072 + 5 * 16384 - mm // 2, 131072 + 2000, n)
        labels = ["match", "mask-low" if hrl > min(mm, 64) else "mask-high"]
        if mm > 128: labels.append("window-front-of-tile")
        if mm > 128: labels.append("near-block-end")
        out.append(case("minmatch_%d" % mm, d, labels, mm=mm, hrl=hrl, hlog=10))
    return out


def _rate_cases():
    out = []
    for name, mm, hrl in (("below", 16, 5), ("equal", 5, 5), ("above", 4, 7)):
        d = rnd(256 * KiB + 1000, 120 + mm)
        copy(d, 70000, 100, 600)
        copy(d, 131072 + 9000, 131072 + 10, 500)      # the first positions of the second frame, copied: the hash starts from 0 there
        labels = ["match", "cap-drop", "stop-k0", "stop-k63", "tile-first-lane"]
        if hrl > mm:          # the stop mask looks further back than the window: in a frame's first positions the start from 0 decides
            force_stop(d, 131072, 3, mm, hrl, 125)
        labels += ["mask-low", "frame-head-stop"] if hrl > mm else ["mask-high"]
        out.append(case("rate_%s_min" % name, d, labels, mm=mm, hrl=hrl))
    return out


def _frame_cases():
    out = []
    # four frames of 128 KiB in one pass; a copy across a frame boundary must not be matched, the same copy inside a frame must
    d = rnd(512 * KiB, 130)
    copy(d, 131072 + 5000, 131072 - 3000, 2500)           # frame 0 -> frame 1: not matched
    copy(d, 2 * 131072 + 70000, 2 * 131072 + 500, 2500)   # inside frame 2
    copy(d, 3 * 131072 - 1000, 2 * 131072 + 20000, 2000)  # frame 2 -> straddles into frame 3: matched up to the frame's end only
    out.append(case("four_frames", d, ["match", "fwd-to-block-end"]))
    # ZSTDMI_CCtx_setHistory(4096) at level 3: blocks of 60 KiB, frames of 120 KiB = 7.5 split tiles.  The hash restarts at each frame
    # start and no window straddles one, also where a frame starts in the middle of a tile.
    for mm, hrl in ((4, 7), (16, 5), (64, 7)):
        d = rnd(480 * KiB - 37, 140 + mm)
        span = 120 * KiB
        for f in (1, 2, 3):
            copy(d, f * span + 30000, f * span, 1500)             # the frame's first bytes, copied inside the frame
            copy(d, f * span + 8, (f - 1) * span + 50000, 300)    # the frame in front, copied to the frame's head: not matched
        if mm == 4:
            force_stop(d, 1 * span, 3, mm, hrl, 145)                    # a stop only the hash from 0 has: the split at the frame's first byte
            force_stop(d, 2 * span, 4, mm, hrl, 146, warm_stops=True)   # one only a hash warmed up on the frame in front has
            force_stop(d, 3 * span, 2, mm, hrl, 147)                    # a stop whose window would begin in front of the frame
        labels = ["match", "frame-start-inside-tile", "window-before-frame"]
        if mm == 4: labels += ["mask-low", "frame-head-stop"]
        if hrl == 5: labels += ["cap-drop"]
        out.append(case("span_120k_min%d" % mm, d, labels, level=3, mm=mm, hrl=hrl, history=4096))
    return out


def _count_cases():
    """split counts at the sort's edges: the input ends right behind the wanted split's last byte (hashRateLog 5: a split per 32 bytes)"""
    out = []
    base = rnd(600 * KiB, 150)
    copy(base, 66000, 2000, 1500); copy(base, 100000, 30000, 1500)
    for want, hrl in ((130, 9), (4095, 5), (4096, 5), (4097, 5), (13000, 5)):
        lay, p, buf = framing(case("tmp", base[:262144 if want < 5000 else len(base)], hrl=hrl, hlog=12))
        pos = lm.splits(buf, lay, p)[0][0]
        d = base[:pos[want - 1] + p.minMatch]
        assert len(d) > 65 * KiB and len(d) % 64
        out.append(case("count_%d" % want, d, ["match"] + (["cap-drop"] if hrl == 5 else []), hrl=hrl, hlog=12, want_splits=want))
    return out


def _key_cases():
    out = []
    d = rnd(128 * KiB, 160)
    for k in range(12):
        copy(d, 66000 + k * 5000, 1000 + (k % 3) * 4000, 1200)
    for k in range(6):        # near copies: what a table of one or two buckets still holds
        copy(d, 20000 + k * 3000 + 700, 20000 + k * 3000, 500)
    for hb, blog in ((0, 6), (1, 5), (2, 4), (3, 3), (5, 3), (8, 3), (9, 3), (17, 3)):       # (ZSTD_c_ldmHashLog is 6 at least)
        labels = ["match"] + (["bucket-evict", "slot-other-checksum"] if hb <= 3 else [])
        out.append(case("key_bits_%d" % hb, d, labels, hlog=hb + blog, blog=blog, hrl=6))
    d2 = rnd(256 * KiB, 161)
    for k in range(12):
        copy(d2, 140000 + k * 5000, 1000 + (k % 3) * 4000, 1200)       # (second frame from first: not matched; same frame:)
        copy(d2, 70000 + k * 4000, 1000 + (k % 3) * 4000, 1200)
    out.append(case("key_bits_17_two_frames", d2, ["match"], hlog=20, blog=3, hrl=6))
    # periodic data: every split has the same window, so all share one key; distance smaller than the length
    per = bytes(rnd(97, 162))
    d3 = bytearray((per * (200 * KiB // 97 + 1))[:200 * KiB])
    out.append(case("periodic_one_key", d3, ["match", "dist-lt-len", "bucket-evict", "before-anchor", "fwd-to-block-end"], hrl=5, blog=2))
    return out


def _bucket_cases():
    out = []
    for blog in (1, 8):
        d = rnd(128 * KiB, 170 + blog)
        reps = 6 if blog == 1 else 300
        for k in range(reps):                       # the same 300 bytes more often than a bucket holds entries
            copy(d, 20000 + k * 330, 1000, 300)
        out.append(case("bucket_log_%d" % blog, d, ["match", "bucket-evict", "bucket-full"], blog=blog, hlog=12, hrl=5))
    return out


def _walk_cases():
    out = []
    settings = dict(mm=64, hrl=9, hlog=14)
    # forward and backward lengths around the 256-byte compare step, each residue of a lane's four bytes
    d = rnd(128 * KiB, 180)
    edges = lm.LEN_EDGES
    for i, f in enumerate(edges):
        dst, src = 65536 + i * 8000, i * 8000
        copy(d, dst, src, 7900)
        cut_lengths(d, settings, dst, src, 7900, f, edges[len(edges) - 1 - i], 1800 + i)
    out.append(case("length_edges", d, ["fwd-%d" % e for e in edges] + ["back-%d" % e for e in edges], **settings))
    # forward < minMatch <= forward + backward: rejected (minMatch above the 64 hashed bytes, the mismatch behind them)
    s2 = dict(mm=1024, hrl=7, hlog=14)
    d = rnd(128 * KiB, 181)
    copy(d, 70000, 1000, 6000)
    lay, p, buf = framing(case("tmp", d, **s2))
    w = [v for v in lm.splits(buf, lay, p)[0][0] if v >= 73000][0]
    d[70000:w - 530] = rnd(w - 530 - 70000, 1811)       # the copy starts 530 bytes in front of the split ...
    d[w - 531] = d[w - 531 - 69000] ^ 0x55
    d[w + 500] ^= 0x55                                  # ... and ends 500 behind it: 1030 in all
    out.append(case("forward_short_total_long", d, ["fwd-short-total-long"], **s2))
    # a forward part that ends at the block's end, the rest found again in the next block; backward stops at anchor / block start
    d = rnd(256 * KiB, 182)
    copy(d, 65536 - 1500, 3000, 4000)               # across the block boundary inside frame 0
    copy(d, 131072 + 65536, 131072, 65536)          # frame 1: block 1 is block 0 again: one match of 65536 bytes
    copy(d, 40000, 10000, 900); copy(d, 40900, 20000, 900)     # two copies back to back: the second's backward part stops at the anchor
    out.append(case("block_end_and_whole_block", d, ["fwd-to-block-end", "back-stop-block-start", "whole-block", "back-stop-anchor", "before-anchor"],
                    hrl=6))
    # backward extension stopped by the frame start: the frame's first bytes copied later in the frame
    d = rnd(128 * KiB, 183)
    copy(d, 50000, 0, 1500)
    out.append(case("back_to_frame_start", d, ["back-stop-frame"], hrl=6))
    # candidates: equal totals go to the nearest, a strictly longer far one wins
    d = rnd(128 * KiB, 184)
    copy(d, 30000, 1000, 800); copy(d, 70000, 1000, 800)            # two equal earlier copies: the nearest is kept
    copy(d, 40000, 5000, 800); d[40400] ^= 0x55                     # a nearer copy that is shorter ...
    copy(d, 80000, 5000, 800)                                       # ... than the far original
    out.append(case("candidate_order", d, ["tie-keeps-nearest", "far-longer-wins"], hrl=6))
    # a split too close to its block's end to be searched (its window ends in the next block) that is later the candidate: the copy's
    # first split finds it, and without it a later split would find the same bytes (the seed: the first from 1860 with such a split)
    d = rnd(128 * KiB, 1860)
    copy(d, 100000, 65536 - 40, 1040)
    out.append(case("near_end_candidate", d, ["near-block-end", "match"], hrl=5))
    # more than 64 searching splits in one block, with matches in the later batches and none in between
    d = rnd(128 * KiB, 185)
    copy(d, 65536 + 100, 100, 400); copy(d, 65536 + 30000, 9000, 400); copy(d, 65536 + 60000, 20000, 400)
    out.append(case("batches_of_splits", d, ["batch-over-64", "match-in-later-batch"], hrl=5, hlog=12))
    return out


def _prefix_cases():
    out = []
    for plen in (40, 16384, 100000):
        pre = rnd(plen, 190 + plen % 97)
        d = rnd(160 * KiB + 123, 191 + plen % 97)
        labels = ["match"]
        if plen >= 16384:
            x = 3000
            d[20000:20000 + x] = pre[1000:1000 + x]                     # a copy out of the prefix's middle
            for k, delta in enumerate((-1, 0, 1)):                      # the prefix's tail, copied: the forward part ends around the seam
                at = 70000 + k * 9000
                d[at:at + 1500] = pre[-1500:]
                if delta == -1: d[at + 1499] = pre[-1] ^ 0x55
                if delta >= 0: d[at + 1500] = d[0] ^ (0x55 if delta == 0 else 0)
                if delta == 1: d[at + 1501] = d[1] ^ 0x55
            labels += ["cand-in-prefix", "fwd-ends-before-seam", "fwd-ends-at-seam", "fwd-ends-behind-seam", "window-straddles-seam"][:4 if plen == 16384 else 5]
        # prefix + the source's head, copied: candidates in the source whose backward part runs into the prefix, to its first byte
        keep = min(plen, 3000)
        d[120000:120000 + keep] = pre[-keep:] if keep < plen else pre
        d[120000 + keep:120000 + keep + 2000] = d[0:2000]
        if plen == 40: labels += ["back-crosses-seam", "back-stop-prefix-start"]
        out.append(case("prefix_%d" % plen, d, labels, wlog=0, hrl=6, hlog=15, prefix=bytes(pre)))
    return out


def _sliding_cases():
    W = 1 << 18
    d = rnd(3 * W, 200)
    copy(d, 2 * W + 50000, W + 50000, 2000)          # candidates exactly maxDist back
    copy(d, 2 * W + 120001, W + 120000, 2000)        # one byte more: passed over
    copy(d, 2 * W + 200000, 2 * W - 30000, 2000)     # a pass boundary between original and copy
    copy(d, 2 * W + 230000, 2 * W + 1000, 2000)      # both in the pass
    return [case("sliding_window", d, ["match", "maxdist-exact", "maxdist-skip", "cand-in-prefix"], wlog=18, hlog=16, hrl=6, sliding=True, pass_chunks=4)]


def _merge_cases():
    """text (the finders' parse is dense) with planted long copies whose ends cut words; rare splits, so that finder matches stand on
    both sides of a long-distance match"""
    out = []
    for level in (1, 3, 5):
        t = bytearray(datagen.gen("text", 256 * KiB, 210 + level))
        r = np.random.RandomState(220 + level)
        for k in range(40):
            n = int(r.randint(70, 3000))
            src = int(r.randint(0, 60000)) + (131072 if k & 1 else 0)
            dst = src + int(r.randint(4000, 60000))
            copy(t, dst, src, n)
        t[200000:200000 + 20000] = rnd(20000, 230 + level)            # a stretch without finder matches (long literal runs) ...
        copy(t, 215000, 140000, 1000)                                 # ... with a long-distance match behind 15000 literals
        out.append(case("merge_text_l%d" % level, t, ["match"], level=level, hrl=6, merge=True))
    # literal runs of 255, 256 and 257 bytes between long-distance matches (random bytes: the copies end where they were planted)
    d = rnd(128 * KiB, 241)
    at = 70000
    for k, gap in enumerate((300, 255, 256, 257)):
        at += gap
        src = 2000 + k * 1000
        copy(d, at, src, 400)
        d[at - 1] = d[src - 1] ^ 0x55; d[at + 400] = d[src + 400] ^ 0x55
        at += 400
    out.append(case("merge_literal_runs", d, ["match"], hrl=5, merge=True))
    # a block without finder sequences (its literals are read from the source) that gets a long-distance match; one without any
    d = rnd(256 * KiB, 240)
    copy(d, 65536 + 61000, 500, 300)
    out.append(case("merge_lit_from_src", d, ["match"], merge=True))
    return out


# the merge labels each merge case reached on an MI355X (the finders' parses decide; tests/test_gpu_ldm_model.py asserts them still
# reached, so a finder change that loses coverage shows).  Labels no natural parse reached are covered by the CPU test's synthetic
# lists only.
MERGE_REACHED = {
    "merge_text_l1": ("L-whole", "F-whole", "F-under-L", "F-head-piece", "tie-Ls==ps", "F-over-64", "out-64", "out-65", "out-129"),
    "merge_text_l3": ("L-whole", "F-whole", "F-under-L", "F-head-piece", "F-tail-piece", "tie-Ls==ps", "piece-2-dropped", "piece-4-kept", "no-L",
                      "F-over-64", "out-64", "out-65", "out-129"),
    "merge_text_l5": ("L-whole", "F-whole", "F-under-L", "F-head-piece", "tie-Ls==ps", "piece-3-dropped", "piece-4-kept", "no-L", "F-over-64",
                      "out-64", "out-65", "out-129"),
    "merge_literal_runs": ("L-whole", "lit-255", "lit-256", "lit-257", "no-L"),
    "merge_lit_from_src": ("L-whole", "L-after-last-F", "lit-over-60000", "no-L"),
}


def cases():
    out = []
    for make in (_min_match_cases, _rate_cases, _frame_cases, _count_cases, _key_cases, _bucket_cases, _walk_cases, _prefix_cases,
                 _sliding_cases, _merge_cases):
        out += make()
    return out
