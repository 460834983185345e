// zmi_batch_plan.h — the plan of a batch whose descriptors lie in HBM (ZSTDMI_compressBatchAsync), stated once: what an
// entry answers for its arguments, how many chunks it is cut into, which entries a chunk limit refuses, which entry owns a chunk, and
// what the stages read for that chunk.  It is compress_entries' host loop (zstd_mi355x.hip) in a form a lane can evaluate for one entry
// or one chunk.  Plain integer code without a HIP header: frame.hip's plan kernels include it under hipcc,
// tests/host/batch_plan_harness.cpp builds it for the CPU.
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

} // namespace zmi
