// zmi_batch_plan.h — the plan of a batch whose descriptors lie in HBM (ZSTDMI_compressBatchAsync), stated once: what an
// entry answers for its arguments, how many chunks it is cut into, which entries a chunk limit refuses, which entry owns a chunk, and
// what the stages read for that chunk.  It is compress_entries' host loop (zstd_mi355x.hip) in a form a lane can evaluate for one entry
// or one chunk.  Plain integer code without a HIP header: frame.hip's plan kernels include it under hipcc,
// tests/host/batch_plan_harness.cpp builds it for the CPU.  Below it, what differs for a pack of the same entries into one destination
// (ZSTDMI_compressPackAsync): tests/host/pack_plan_harness.cpp.
#pragma once
#include "zmi_common.h"
#include "zmi_frame.h"

namespace zmi {

// kAsyncBase: the "base pointer" huf_encode and gather get with absolute addresses (not null: a null dst is huf_encode's test hook);
// kAsyncSpan: their dstCapacity — above every device address, far from wrapping when a frame's size is added
constexpr u64 kAsyncBase = 4096, kAsyncSpan = (u64)1 << 62;
enum AsyncVerdict : u32 { kAsyncGood = 0, kAsyncEmpty = 0xFFFFFFFFu };      // (else: the zstd error code the entry answers)
constexpr u64 kAsyncBoundMax = ((u64)4 << 20) - 1;      // an entry of several chunks: below 4 MiB (chunk_frame_word's frame size)

// the argument checks, in compress_entries' order.  src, dst: the addresses as integers; bound: the prepared srcSizeBound; emptyLen:
// the bytes of the empty frame under the call's parameters
ZMI_HD u32 plan_verdict(u64 src, u64 S, u64 dst, u64 cap, u64 bound, u32 emptyLen)
{
    u32 v = kAsyncGood;
    if (S > bound || (S && !src)) v = kErrSrcSizeWrong;
    else if (dst < kAsyncBase) v = cap ? kErrDstBufferNull : kErrDstSizeTooSmall;        // (null; no device address lies below kAsyncBase)
    else if (!S) v = cap < emptyLen ? (u32)kErrDstSizeTooSmall : (u32)kAsyncEmpty;
    return v;
}
// chunks of an entry: failed and empty ones count for nothing (S <= bound <= kAsyncBoundMax for a good one)
ZMI_HD u32 plan_chunks(u32 verdict, u64 S, u32 chunkBytes) { return verdict == kAsyncGood ? (u32)((S + chunkBytes - 1) / chunkBytes) : 0u; }
// the chunk limit: a good entry is refused (workSpace_tooSmall) iff the chunks of the good entries up to and including it exceed
// maxChunks.  The sums never decrease, so every good entry behind a refused one is refused too, and the entries in front of the first
// refused one own the chunks [0, its exclusive sum): entFirst[e] = min(exclusive sum of e, exclusive sum of the first refused entry).
ZMI_HD bool plan_refused(u64 inclusiveChunks, u32 maxChunks) { return inclusiveChunks > maxChunks; }
// is an entry of cnt chunks behind `exclusive` chunks the first refused one?  (one entry of a call at most; its exclusive sum is the cut)
ZMI_HD bool plan_is_cut(u64 exclusive, u32 cnt, u32 maxChunks) { return cnt && plan_refused(exclusive + cnt, maxChunks) && !plan_refused(exclusive, maxChunks); }
constexpr u32 kPlanNoCut = 0xFFFFFFFFu;
ZMI_HD u32 plan_first(u32 exclusive, u32 cut) { return exclusive < cut ? exclusive : cut; }
// what an entry answers behind the limit
ZMI_HD u32 plan_limited(u32 verdict, u64 exclusive, u32 cnt, u32 maxChunks) { return (cnt && plan_refused(exclusive + cnt, maxChunks)) ? (u32)kErrWorkSpaceTooSmall : verdict; }

// the entry that owns chunk c < entFirst[n]: the last e with entFirst[e] <= c (entries without chunks repeat their successor's first
// chunk and are stepped over).  entFirst[0 .. n] ascending, entFirst[0] = 0.
ZMI_HD u32 plan_owner(const u32* entFirst, u32 n, u32 c)
{
    u32 lo = 0, hi = n;             // the answer lies in [lo, hi)
    while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (entFirst[mid] <= c) lo = mid; else hi = mid; }
    return lo;
}

// chunk k of an entry of S bytes at src, cut into chunks of chunkBytes, frameBlocks of them to a frame (0: every chunk a frame of its
// own, no word): the bytes the stage copies and the chunk's place in its frame as the single call frames the entry
struct PlanChunk { u64 from; u32 len, frameWord; };
ZMI_HD PlanChunk plan_chunk(u64 src, u64 S, u32 k, u32 chunkBytes, u32 frameBlocks)
{
    const u64 o = (u64)k * chunkBytes;
    PlanChunk r;
    r.from = src + o;
    r.len = (u32)(S - o < chunkBytes ? S - o : chunkBytes);
    r.frameWord = 0;
    if (frameBlocks) {
        const BlockPlace at = block_place<kArith>(layout_arith(chunkBytes, frameBlocks, S), k);
        r.frameWord = chunk_frame_word(at.block, (u32)at.frameLen);
    }
    return r;
}
// a chunk slot at or beyond the call's total: one byte read from `dummy`, a frame of its own (the stages have never seen an empty chunk)
ZMI_HD PlanChunk plan_chunk_idle(u64 dummy) { return PlanChunk{ dummy, 1u, chunk_frame_word(0u, 1u) }; }

// ---- a pack (ZSTDMI_compressPackAsync): the same entries into ONE destination, densely, one seek table behind them ----
// An entry has no destination of its own, so plan_verdict's dst and cap checks fall away: what is left of it.
ZMI_HD u32 pack_verdict(u64 src, u64 S, u64 bound) { return (S > bound || (S && !src)) ? (u32)kErrSrcSizeWrong : S ? (u32)kAsyncGood : (u32)kAsyncEmpty; }
// does the entry fail the pack?  (the verdict behind plan_limited: an error code, workSpace_tooSmall included)
ZMI_HD bool pack_fails(u32 verdict) { return verdict != kAsyncGood && verdict != kAsyncEmpty; }
// the entry's frames = its rows in the table: frameBlocks chunks to a frame (0: every chunk a frame), an empty entry the one empty frame
ZMI_HD u32 pack_frames(u32 verdict, u32 cnt, u32 frameBlocks)
{
    const u32 fb = frameBlocks ? frameBlocks : 1u;
    return verdict == kAsyncGood ? (cnt + fb - 1) / fb : verdict == kAsyncEmpty ? 1u : 0u;
}
// the entry's bytes in the stream: the sum of its chunks' frame bytes, or the empty frame
ZMI_HD u64 pack_bytes(u32 verdict, u64 chunkSum, u32 emptyLen) { return verdict == kAsyncGood ? chunkSum : verdict == kAsyncEmpty ? (u64)emptyLen : 0; }
constexpr u32 kPackNoFail = 0xFFFFFFFFu;
constexpr u64 kSeekTableFixed = 17;         // skippable header (8) + footer (9)
// the one decision: failVerdict = the verdict of the lowest failing entry (kPackNoFail: none), total = the frames' bytes, frames = the
// rows.  The answer is the stream's length or the error code as a size_t holds it; nothing is written unless pack_answer_ok.
ZMI_HD u64 pack_answer(u32 failVerdict, u64 total, u64 frames, u64 cap)
{
    if (failVerdict != kPackNoFail) return (u64)0 - (u64)failVerdict;
    const u64 all = total + kSeekTableFixed + 8 * frames;
    return all <= cap ? all : (u64)0 - (u64)kErrDstSizeTooSmall;
}
ZMI_HD bool pack_answer_ok(u64 answer) { return !(answer > (u64)0 - (u64)kErrMaxCode); }     // (ZSTD_isError's comparison)
// chunk k of an entry: the table row of its frame, whether it is that frame's first chunk (the lane that files the row), and the
// address huf_encode and gather are given for it: the destination's offset from kAsyncBase + the entry's place + the chunks in front
ZMI_HD u32 pack_row(u32 entRow, u32 k, u32 frameBlocks) { return entRow + (frameBlocks ? k / frameBlocks : k); }
ZMI_HD bool pack_row_lead(u32 k, u32 frameBlocks) { return frameBlocks ? k % frameBlocks == 0 : true; }
ZMI_HD u64 pack_chunk_at(bool ok, u64 dst, u64 entAt, u64 inner) { return ok ? dst - kAsyncBase + entAt + inner : kAsyncSpan; }

} // namespace zmi
