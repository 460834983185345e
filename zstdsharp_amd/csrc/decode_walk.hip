// decode_walk.hip — the decoder's work lists on gfx950 (SURVEY.md §8 a-13, a-14, a-16's headers).
//
//   frame walk      : ZSTD_findFrameSizeInfo over the whole input (U/ZstdDecompress.cs:877-951, 971-993), headers only.
//                     Parallel form: the input is cut into 128 KiB segments; one wave per segment scans for the first frame
//                     magic, validates it by chaining frame -> frame until it leaves the segment, and a scan kernel checks
//                     that every segment's exit is the next segment's entry (anything else — embedded frames inside raw
//                     blocks, a corrupt header, a frame naming a dictionary — falls back to the exact serial walk, which
//                     also produces the reference's error).  Both forms count first (the host sizes the lists), then emit
//                     one FrameDesc per frame and one BlockDesc per block.
//   block_parse     : one lane per compressed block: the literals section header (ZSTD_decodeLiteralsBlock's header parse,
//                     U/ZstdDecompressBlock.cs:88-396) and the sequences section header (ZSTD_decodeSeqHeaders, :1845-1943) up
//                     to where the bitstream starts; the NCount descriptions are measured, not stored.
//   block_link      : one lane per frame: which earlier block a treeless literals section takes its Huffman table from
//                     (:197-207) and which one defines each FSE table used in repeat mode (:1780-1786) — the only state
//                     besides repcodes and history that the reference carries from block to block; literal offsets.
//   seq_scan        : exclusive scan of the blocks' sequence counts -> where each block's records go.
//   block_offsets   : one wave per frame, after seq_decode: output offset and starting repcodes of every block (prefix sums;
//                     repcodes by composing the blocks' transfer functions), regenerated size against the header's
//                     (U/ZstdDecompress.cs:1177-1184).
//   frame_rescan    : only when some frame carries no content size: output offsets of the frames from their regenerated sizes.
//   batch_rescan    : the same per entry of a batch (ZSTDMI_DCtx_setBatchUnsized): one wave per entry that holds such a frame.
#include "zmi_decode.h"
#include "zmi_fse.h"
#include "zmi_host.h"
#include "zmi_batch_rescan.h"

namespace zmi {

// ------------------------------------------------------------------------------------------------
// one frame of the chain
// ------------------------------------------------------------------------------------------------
// frame (or skippable frame) at pos -> next position.  Returns 0 frame, 1 skippable, or an error code >= 2 (the reference's).
// `strict`: the parallel walk's view — a frame that names a dictionary is left to the serial walk (which knows the loaded one).
struct ChainOut { u64 next; u64 content; u64 window; u32 nbBlocks; u32 hdrSize; u32 checksum; u32 unsized; u32 dictID; };
// EMIT: the frame was validated by an earlier walk; this one also writes its blocks' descriptors (block header walks are chains of
// dependent loads — 0.3 us a block — so a walk that emits must not be a walk of its own behind the one that validates)
template <bool EMIT>
__device__ inline u32 chain_step_t(const u8* __restrict__ src, u64 srcSize, u64 pos, ChainOut& o, u32 frameIdx, u32 firstBlock, BlockDesc* __restrict__ blocks)
{
    o.content = 0; o.nbBlocks = 0; o.hdrSize = 0; o.checksum = 0; o.unsized = 0; o.dictID = 0; o.window = 0; o.next = pos;
    if (srcSize - pos < 5) return kErrSrcSizeWrong;
    const u8* p = src + pos; const u64 avail = srcSize - pos;
    const u32 magic = readLE32(p);
    if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
        if (avail < 8) return kErrSrcSizeWrong;
        const u64 sz = (u64)readLE32(p + 4) + 8;
        if (sz > avail) return kErrSrcSizeWrong;
        o.next = pos + sz; return 1;
    }
    const FrameHeader h = parse_frame_header(p, avail);
    if (h.err) return h.err;
    u64 q = pos + h.headerSize; u32 nb = 0;
    for (;;) {
        if (srcSize - q < 3) return kErrSrcSizeWrong;
        const u32 bh = readLE24(src + q);
        const u32 last = bh & 1, type = (bh >> 1) & 3; u32 cSize = bh >> 3;
        if (type == 3) return kErrCorruption;
        if (type == 1) cSize = 1;
        if (3 + (u64)cSize > srcSize - q) return kErrSrcSizeWrong;
        if (EMIT) {
            BlockDesc b = {};
            b.srcOff = q + 3; b.frame = frameIdx; b.type = (u8)type; b.last = (u8)last;
            b.bsz = cSize; b.outSize = type == 2 ? 0u : (bh >> 3);
            b.hufSrc = kNoBlock; b.tblSrc[0] = b.tblSrc[1] = b.tblSrc[2] = kNoBlock;
            blocks[firstBlock + nb] = b;
        }
        q += 3 + cSize;
        if (++nb == 0xFFFFFFFFu) return kErrMemoryAllocation;
        if (last) break;
    }
    if (h.checksum) { if (srcSize - q < 4) return kErrSrcSizeWrong; q += 4; }
    o.next = q; o.nbBlocks = nb; o.hdrSize = h.headerSize; o.checksum = h.checksum; o.dictID = h.dictID; o.window = h.windowSize;
    o.unsized = h.contentSize == ~0ull;
    // a frame without a content size gets the bound ZSTD_findFrameSizeInfo gives it: nbBlocks x min(window, 128 KiB)
    o.content = o.unsized ? (u64)nb * (h.windowSize < (1u << 17) ? h.windowSize : (u64)(1u << 17)) : h.contentSize;
    return 0;
}

__device__ inline u32 chain_step(const u8* __restrict__ src, u64 srcSize, u64 pos, ChainOut& o) { return chain_step_t<false>(src, srcSize, pos, o, 0, 0, nullptr); }

// the frame at `pos` (validated by an earlier walk) into the lists: ONE walk over its block headers.  -> chain_step's result
__device__ inline u32 emit_frame(const u8* __restrict__ src, u64 srcSize, u64 pos, ChainOut& o, u32 frameIdx, u32 firstBlock, u64 dstOff,
                                 FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks)
{
    const u32 st = chain_step_t<true>(src, srcSize, pos, o, frameIdx, firstBlock, blocks);
    if (st) return st;
    FrameDesc f; f.srcOff = pos; f.dstOff = dstOff; f.scratchOff = dstOff; f.srcSize = o.next - pos; f.dstSize = o.content;
    f.firstBlock = firstBlock; f.nbBlocks = o.nbBlocks; f.unsized = o.unsized; f.checksum = o.checksum; f.bad = 0; f.hasSeq = 0; f.viaOrigin = 0; f.dictSlot = 0; f.originOff = 0;
    frames[frameIdx] = f;
    return 0;
}

// the exact serial walk (ZSTD_decompressMultiFrame's loop, U/ZstdDecompress.cs:1216-1315), one lane.  emit = 0: count frames and
// blocks, sum the content sizes, find the first error; emit = 1 (same input, lists allocated): write the lists.
// kSet (ZSTD_d_refMultipleDDicts with two or more DDicts in the set): a frame's dictID is looked up in the slot table (dictset_select,
// zmi_dictset.h: nSet sorted records, the current DDict's behind them), the record's index goes into the frame's descriptor, and the
// frames found in the set are counted into the status words.  kSet = false is the kernel as it always was.
template <bool kSet>
__device__ __forceinline__ void frame_walk_serial_body(const u8* __restrict__ src, u64 srcSize, FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks,
                                                       u32 maxFrames, u32* __restrict__ status, u32 dictID, u32 emit, const DictSlot* __restrict__ slots, u32 nSet)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    u64 pos = 0, dstOff = 0; u32 n = 0, err = 0, nUnsized = 0; u64 nBlocks = 0; u32 nInSet = 0;
    while (srcSize - pos >= 5) {            // ZSTD_decompressMultiFrame loop condition (U/ZstdDecompress.cs:1228)
        ChainOut o;
        // (emit: the same input has been through the counting pass, which stopped at the first error and sized the lists)
        const u32 st = emit ? emit_frame(src, srcSize, pos, o, n, (u32)nBlocks, dstOff, frames, blocks) : chain_step(src, srcSize, pos, o);
        if (st == 1) { pos = o.next; continue; }
        if (st) { err = (st == kErrPrefixUnknown && n > 0) ? (u32)kErrSrcSizeWrong : st; break; }
        if constexpr (kSet) {
            u32 inSet, wrong;
            const u32 slot = dictset_select(slots, nSet, o.dictID, &inSet, &wrong);
            if (wrong) { err = kErrDictionaryWrong; break; }
            if (n >= maxFrames || nBlocks + o.nbBlocks > 0xFFFFFFF0ull) { err = kErrMemoryAllocation; break; }
            if (emit) frames[n].dictSlot = slot;            // (emit_frame has just written frames[n])
            nInSet += inSet;
        } else {
            if (o.dictID && o.dictID != dictID) { err = kErrDictionaryWrong; break; }       // U/ZstdDecompress.cs:1404-1412 (dictID 0 = none loaded)
            if (n >= maxFrames || nBlocks + o.nbBlocks > 0xFFFFFFF0ull) { err = kErrMemoryAllocation; break; }
        }
        n++; nUnsized += o.unsized; nBlocks += o.nbBlocks;
        dstOff += o.content; pos = o.next;
    }
    if (!err && pos != srcSize) err = kErrSrcSizeWrong;     // trailing garbage (U/ZstdDecompress.cs:1309-1312)
    if (emit) return;
    status[kStFrames] = n; status[kStErr] = err; status[kStTotalLo] = (u32)dstOff; status[kStTotalHi] = (u32)(dstOff >> 32);
    status[kStUnsized] = nUnsized; status[kStBlocks] = (u32)nBlocks;
    if constexpr (kSet) status[kStSetFrames] = err ? 0u : nInSet;
}
template <bool kSet>
__global__ void frame_walk_serial_kernel(const u8* __restrict__ src, u64 srcSize, FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks,
                                         u32 maxFrames, u32* __restrict__ status, u32 dictID, u32 emit, const DictSlot* __restrict__ slots, u32 nSet)
{
    frame_walk_serial_body<kSet>(src, srcSize, frames, blocks, maxFrames, status, kSet ? 0 : dictID, emit, kSet ? slots : nullptr, kSet ? nSet : 0);
}

// ------------------------------------------------------------------------------------------------
// parallel frame walk
// ------------------------------------------------------------------------------------------------
constexpr u32 kSegLog = 17;
struct SegInfo { u64 entry, exit, dstBytes; u32 count, valid, blocks, pad; };

// The scan for a segment's first frame start is a chain of dependent memory latencies (a window is tested before the next one is
// fetched), so a window is wide: kWalkU groups of 1 KiB, a group being one 16-byte load per lane, all issued before the first is tested.
#ifndef ZMI_WALK_U
#define ZMI_WALK_U 4
#endif
constexpr u32 kWalkU = ZMI_WALK_U;
constexpr u64 kWalkWindow = 1024ull * kWalkU;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(1))) u32x4u;

__device__ __forceinline__ bool is_frame_magic(u32 v) { return v == 0xFD2FB528u || (v >> 4) == 0x184D2A5u; }
// the n <= 16 bytes at src + off that lie inside the input, the others zero (no magic has a zero byte on top, so zeros never match)
__device__ inline u32x4 load_piece_bytes(const u8* __restrict__ src, u64 srcSize, u64 off)
{
    u64 lo = 0, hi = 0;
#pragma unroll
    for (u32 k = 0; k < 8; ++k) {
        if (off + k < srcSize) lo |= (u64)src[off + k] << (8 * k);
        if (off + 8 + k < srcSize) hi |= (u64)src[off + 8 + k] << (8 * k);
    }
    u32x4 v; v.x = (u32)lo; v.y = (u32)(lo >> 32); v.z = (u32)hi; v.w = (u32)(hi >> 32);
    return v;
}
// bit k: the dword at byte k of (v, next) is a frame or skippable-frame magic
__device__ __forceinline__ u32 magic_mask16(u32x4 v, u32 next)
{
    const u32 d[5] = { v.x, v.y, v.z, v.w, next };
    u32 mask = 0;
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        const u32 sh = 8 * (k & 3);
        const u32 w = sh ? (d[k >> 2] >> sh) | (d[(k >> 2) + 1] << (32 - sh)) : d[k >> 2];
        if (is_frame_magic(w)) mask |= 1u << k;
    }
    return mask;
}

__global__ __launch_bounds__(64) void walk_segments_kernel(const u8* __restrict__ src, u64 srcSize, SegInfo* __restrict__ segs, u32 nSeg)
{
    const u32 s = blockIdx.x, lane = threadIdx.x;
    if (s >= nSeg) return;
    const u64 segStart = (u64)s << kSegLog;
    const u64 segEnd = (segStart + (1ull << kSegLog)) < srcSize ? segStart + (1ull << kSegLog) : srcSize;
    SegInfo r; r.entry = 0; r.exit = 0; r.dstBytes = 0; r.count = 0; r.valid = 0; r.blocks = 0; r.pad = 0;
    // a position p is a candidate if the dword at p is a frame or skippable-frame magic; the position segEnd - 1 reads up to segEnd + 2
    const u64 readEnd = segEnd + 3;
    for (u64 win = segStart; win < segEnd && !r.valid; win += kWalkWindow) {
        // lane l of group g holds the 16 positions from win + 1024 g + 16 l.  A window that lies inside the input with the dword behind
        // it (every window but the last few of the input) is loaded without a condition in sight, so that nothing waits between the
        // loads; in the others a piece that would reach past the input is read bytewise, and one wholly past readEnd not at all.
        u32x4 v[kWalkU];
        u32 tail;                                               // the dword behind the window: what the last lane's positions run into
        if (win + kWalkWindow + 4 <= srcSize) {
            const u8* const p = src + win + 16 * lane;
#pragma unroll
            for (u32 g = 0; g < kWalkU; ++g) v[g] = *(const u32x4u*)(p + 1024 * g);
            tail = readLE32(src + win + kWalkWindow);
        } else {
#pragma unroll
            for (u32 g = 0; g < kWalkU; ++g) {
                const u64 off = win + 1024 * g + 16 * lane;
                v[g] = (u32x4)(0u);
                if (off < readEnd) { if (off + 16 <= srcSize) v[g] = *(const u32x4u*)(src + off); else v[g] = load_piece_bytes(src, srcSize, off); }
            }
            tail = load_piece_bytes(src, srcSize, win + kWalkWindow).x;
        }
        u32 hm[kWalkU];                                         // per lane and group: hit mask of its 16 positions
#pragma unroll
        for (u32 g = 0; g < kWalkU; ++g) {
            const u64 off = win + 1024 * g + 16 * lane;
            u32 next = __shfl_down(v[g].x, 1);
            const u32 carry = g + 1 < kWalkU ? read_lane(v[g + 1 < kWalkU ? g + 1 : g].x, 0) : tail;
            if (lane == 63) next = carry;
            u32 m = magic_mask16(v[g], next);
            if (off >= segEnd) m = 0; else if (segEnd - off < 16) m &= (1u << (u32)(segEnd - off)) - 1u;
            hm[g] = m;
        }
        for (;;) {
            // the lowest hit still in the masks: groups in order, then the first lane, then the lowest bit
            u64 cand = ~0ull;
#pragma unroll
            for (u32 g = 0; g < kWalkU; ++g) {
                if (cand != ~0ull) continue;
                const u64 m = ballot(hm[g] != 0);
                if (!m) continue;
                const u32 fl = ctz64(m), bits = read_lane(hm[g], fl);
                cand = win + 1024 * g + 16 * fl + (u32)__builtin_ctz(bits);
                if (lane == fl) hm[g] = bits & (bits - 1);
            }
            if (cand == ~0ull) break;
            // validate by chaining until the chain leaves the segment (every lane walks the same chain: uniform)
            u64 pos = cand, dstBytes = 0, nBlocks = 0; u32 count = 0; bool ok = true;
            while (pos < segEnd) {
                ChainOut o;
                const u32 st = chain_step(src, srcSize, pos, o);
                // frames naming a dictionary and frames without a content size take the serial walk (it knows the loaded dictionary,
                // and the regenerated sizes of unsized frames decide where everything behind them goes)
                if (st >= 2 || (st == 0 && (o.dictID || o.unsized))) { ok = false; break; }
                if (st == 0) { count++; dstBytes += o.content; nBlocks += o.nbBlocks; }
                pos = o.next;
            }
            // A magic that turns up by chance inside a frame's payload (the sixteen skippable-frame magics: once per 270 MB of
            // incompressible payload) can chain out of the segment too — a skippable frame of any size that stays inside the input is
            // "valid" — and, where it lies in front of the segment's first real frame, the link check then sends the whole call to the
            // serial walk (40 ms for 16 384 frames).  A real chain leaves the segment AT a frame (or at the end of the input): a
            // candidate whose chain lands anywhere else is not one.
            if (ok && pos != srcSize) {
                u32 w = 0;
                if (srcSize - pos >= 4) w = readLE32(src + pos);
                if (!is_frame_magic(w)) ok = false;
            }
            if (ok && nBlocks < 0xFFFFFFF0ull) { r.entry = cand; r.exit = pos; r.dstBytes = dstBytes; r.count = count; r.blocks = (u32)nBlocks; r.valid = 1; break; }
            // false positive (or a corrupt stream: the link check then sends us to the serial walk): on to the next hit
        }
    }
    if (lane == 0) segs[s] = r;
}

// The single-workgroup scans (walk_link, seq_scan, frame_rescan) take kScanItems consecutive items per thread and round, and a
// round's loads are issued before the round in front of it reaches its barrier: the barrier orders LDS only (lds_barrier; the
// per-wave totals are double-buffered, so one barrier a round is enough), so no load waits for a barrier and a round costs its
// arithmetic, not a memory latency.
constexpr u32 kScanItems = 4;
constexpr u32 kScanRound = 1024 * kScanItems;

// (walk_link carries a whole SegInfo per item: two per thread keep it in registers)
constexpr u32 kLinkItems = 2;
constexpr u32 kLinkRound = 1024 * kLinkItems;
// single workgroup: link check + prefix sums.  status: frames, total, blocks; [kStUsable] = 1 when the parallel walk is usable
// pinned (null: none): the host's pinned copy of the status words (zmi_host.h); the words written here are written there too, and they
// are all the host reads of the counting walk
__global__ __launch_bounds__(1024) void walk_link_kernel(const SegInfo* __restrict__ segs, u32 nSeg, u64 srcSize, u32 maxFrames,
                                                         u32* __restrict__ frameBase, u32* __restrict__ blockBase, u64* __restrict__ dstBase,
                                                         u32* __restrict__ status, u32* __restrict__ pinned)
{
    __shared__ u64 sh64[2][16], shBlk[2][16], shExit[2][16]; __shared__ u32 sh32[2][16]; __shared__ s32 shLast[2][16]; __shared__ u32 bad;
    const u32 tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    if (tid == 0) bad = 0;
    __syncthreads();
    u64 carryDst = 0, carryBlk = 0, carryExit = 0; u32 carryCnt = 0; s32 carryLast = -1;
    SegInfo g[kLinkItems], nx[kLinkItems];
    auto load = [&](u32 base, SegInfo (&o)[kLinkItems]) {
#pragma unroll
        for (u32 j = 0; j < kLinkItems; ++j) {
            const u32 i = base + tid * kLinkItems + j;
            o[j].valid = 0; o[j].count = 0; o[j].dstBytes = 0; o[j].entry = 0; o[j].exit = 0; o[j].blocks = 0; o[j].pad = 0;
            if (i < nSeg) o[j] = segs[i];
        }
    };
    load(0, g);
    u32 par = 0;
    for (u32 base = 0; base < nSeg; base += kLinkRound, par ^= 1) {
        if (base + kLinkRound < nSeg) load(base + kLinkRound, nx);
        // my valid segments: counts, bytes, blocks, and the last one's index and exit
        u32 c = 0; u64 b = 0, k = 0, ex = 0; s32 lastv = -1;
#pragma unroll
        for (u32 j = 0; j < kLinkItems; ++j)
            if (g[j].valid) { c += g[j].count; b += g[j].dstBytes; k += g[j].blocks; lastv = (s32)(base + tid * kLinkItems + j); ex = g[j].exit; }
        // inclusive scans inside the wave (the last valid segment so far travels with its exit: what the next valid one must enter at)
        u32 ci = c; u64 bi = b, ki = k, ei = ex; s32 li = lastv;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 tc = __shfl_up(ci, d); const u64 tb = __shfl_up(bi, d), tk = __shfl_up(ki, d), te = __shfl_up(ei, d); const s32 tl = __shfl_up(li, d);
            if ((int)lane >= d) { ci += tc; bi += tb; ki += tk; if (tl > li) { li = tl; ei = te; } }
        }
        if (lane == 63) { sh32[par][wave] = ci; sh64[par][wave] = bi; shBlk[par][wave] = ki; shLast[par][wave] = li; shExit[par][wave] = ei; }
        lds_barrier();
        u32 cb = carryCnt; u64 bb = carryDst, kb = carryBlk, eb = carryExit; s32 lb = carryLast; u32 call = 0; u64 ball = 0, kall = 0, eall = 0; s32 lall = -1;
#pragma unroll 2
        for (u32 w = 0; w < 16; w++) {
            const s32 lw = shLast[par][w]; const u64 ew = shExit[par][w];
            if (w < wave) { cb += sh32[par][w]; bb += sh64[par][w]; kb += shBlk[par][w]; if (lw > lb) { lb = lw; eb = ew; } }
            call += sh32[par][w]; ball += sh64[par][w]; kall += shBlk[par][w]; if (lw > lall) { lall = lw; eall = ew; }
        }
        // previous valid segment (exclusive): from the lanes before me in my wave, else from earlier waves / rounds
        s32 prev = __shfl_up(li, 1); u64 prevExit = __shfl_up(ei, 1);
        if (lane == 0 || prev <= lb) { prev = lb; prevExit = eb; }
        u32 fb = cb + ci - c; u64 db = bb + bi - b, kk = kb + ki - k;
#pragma unroll
        for (u32 j = 0; j < kLinkItems; ++j) {
            const u32 i = base + tid * kLinkItems + j;
            if (i < nSeg && g[j].valid) {
                const u64 expect = prev >= 0 ? prevExit : 0;
                if (g[j].entry != expect) atomicOr(&bad, 1u);
                frameBase[i] = fb; dstBase[i] = db; blockBase[i] = (u32)kk;
                fb += g[j].count; db += g[j].dstBytes; kk += g[j].blocks; prev = (s32)i; prevExit = g[j].exit;
            }
        }
        carryCnt += call; carryDst += ball; carryBlk += kall; if (lall > carryLast) { carryLast = lall; carryExit = eall; }
#pragma unroll
        for (u32 j = 0; j < kLinkItems; ++j) g[j] = nx[j];
    }
    __syncthreads();
    if (tid == 0) {
        u32 usable = !bad;
        if (carryLast < 0 || carryExit != srcSize) usable = 0;
        if (carryCnt > maxFrames || carryBlk > 0xFFFFFFF0ull) usable = 0;
        status[kStFrames] = carryCnt; status[kStErr] = 0; status[kStTotalLo] = (u32)carryDst; status[kStTotalHi] = (u32)(carryDst >> 32);
        status[kStUsable] = usable; status[kStUnsized] = 0; status[kStBlocks] = (u32)carryBlk;
        if (pinned) {
            pinned[kStFrames] = carryCnt; pinned[kStErr] = 0; pinned[kStTotalLo] = (u32)carryDst; pinned[kStTotalHi] = (u32)(carryDst >> 32);
            pinned[kStUsable] = usable; pinned[kStUnsized] = 0; pinned[kStBlocks] = (u32)carryBlk;
        }
    }
}

__global__ __launch_bounds__(256) void walk_emit_kernel(const u8* __restrict__ src, u64 srcSize, const SegInfo* __restrict__ segs, u32 nSeg,
                                                        const u32* __restrict__ frameBase, const u32* __restrict__ blockBase, const u64* __restrict__ dstBase,
                                                        FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks)
{
    const u32 s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nSeg) return;
    const SegInfo g = segs[s];
    if (!g.valid) return;
    u64 pos = g.entry, dstOff = dstBase[s]; u32 idx = frameBase[s], blk = blockBase[s];
    while (pos < g.exit) {
        ChainOut o;
        const u32 st = emit_frame(src, srcSize, pos, o, idx, blk, dstOff, frames, blocks);
        if (st >= 2) return;                                   // cannot happen: the chain was validated by walk_segments
        if (st == 0) { idx++; blk += o.nbBlocks; dstOff += o.content; }
        pos = o.next;
    }
}

// ------------------------------------------------------------------------------------------------
// batch walk (ZSTDMI_decompressBatch): one lane per entry runs the exact serial walk over that entry alone — every frame, skippable
// frames, trailing garbage, a dictID that is not the loaded one — in count-then-emit form like the walks above
// ------------------------------------------------------------------------------------------------
// count: what frame_walk_serial_kernel's counting pass and the host's checks behind it make of the entry
// kSet: as in frame_walk_serial_body; the frames found in the set are counted for the entries that are decoded here
// kOpen (ZSTDMI_DCtx_setBatchUnsized): an entry that holds a frame without a content size is decoded here too.  Where its frames go
// is settled by batch_rescan_kernel once their regenerated sizes are known, and only that kernel holds it to its capacity — the
// bounds that stand for the sizes here (chain_step) usually exceed it.  Such an entry is marked `open` and counted, and `result`
// carries the literal scratch it asks for: per frame the smaller of its content size (or bound) and the entry's capacity, since the
// literals of an entry that fits cannot outnumber its output.  kOpen = false is the kernel as it always was.
template <bool kSet, bool kOpen = false>
__device__ __forceinline__ void batch_walk_count_body(const u8* __restrict__ src, const BatchEntryIn* __restrict__ in, BatchEntryOut* __restrict__ out, u32 nEntries,
                                                      u32 dictID, u64 aloneAbove, const DictSlot* __restrict__ slots, u32 nSet, u32* __restrict__ status)
{
    const u32 e = blockIdx.x * 64 + threadIdx.x;
    if (e >= nEntries) return;
    const BatchEntryIn E = in[e];
    BatchEntryOut r = {};
    if (E.srcSize > aloneAbove) { r.state = kBatchAlone; out[e] = r; return; }
    const u64 end = E.srcOff + E.srcSize;
    const u32 maxFrames = (u32)((E.srcSize / 9 + 1) < (1u << 26) ? (E.srcSize / 9 + 1) : (1u << 26));
    u64 pos = E.srcOff, content = 0, nBlocks = 0; u32 n = 0, err = 0, nUnsized = 0, nInSet = 0;
    u64 room = 0;
    while (end - pos >= 5) {
        ChainOut o;
        const u32 st = chain_step(src, end, pos, o);
        if (st == 1) { pos = o.next; continue; }
        if (st) { err = (st == kErrPrefixUnknown && n > 0) ? (u32)kErrSrcSizeWrong : st; break; }
        if constexpr (kSet) {
            u32 inSet, wrong;
            (void)dictset_select(slots, nSet, o.dictID, &inSet, &wrong);
            if (wrong) { err = kErrDictionaryWrong; break; }
            nInSet += inSet;
        } else if (o.dictID && o.dictID != dictID) { err = kErrDictionaryWrong; break; }
        if (n >= maxFrames || nBlocks + o.nbBlocks > 0xFFFFFFF0ull) { err = kErrMemoryAllocation; break; }
        n++; nUnsized += o.unsized; nBlocks += o.nbBlocks;
        content += o.content; pos = o.next;
        if constexpr (kOpen) room += o.content < E.dstCap ? o.content : E.dstCap;
    }
    if (!err && pos != end) err = kErrSrcSizeWrong;
    if (err) { r.state = kBatchDone; r.result = (u64)0 - (u64)err; }
    else if (nUnsized && !kOpen) r.state = kBatchAlone;
    else if (!nUnsized && content > E.dstCap) { r.state = kBatchDone; r.result = (u64)0 - (u64)kErrDstSizeTooSmall; }
    else { r.state = kBatchDecode; r.result = content; r.nFrames = n; r.nBlocks = (u32)nBlocks; }
    if constexpr (kOpen) { if (r.state == kBatchDecode && nUnsized) { r.open = 1; r.result = room; atomicAdd(status + kStOpenEntries, 1u); } }
    out[e] = r;
    if constexpr (kSet) { if (r.state == kBatchDecode && nInSet) atomicAdd(status + kStSetFrames, nInSet); }
}
template <bool kSet, bool kOpen>
__global__ __launch_bounds__(64) void batch_walk_count_kernel(const u8* __restrict__ src, const BatchEntryIn* __restrict__ in, BatchEntryOut* __restrict__ out, u32 nEntries,
                                                              u32 dictID, u64 aloneAbove, const DictSlot* __restrict__ slots, u32 nSet, u32* __restrict__ status)
{
    batch_walk_count_body<kSet, kOpen>(src, in, out, nEntries, kSet ? 0 : dictID, aloneAbove, kSet ? slots : nullptr, kSet ? nSet : 0, kSet || kOpen ? status : nullptr);
}

// scan (single workgroup): every decoded entry's first frame, first block and literal-scratch offset; the totals go to the status
// words the single call's walk fills (a total beyond the lists' index range: memory_allocation for the whole call)
// kCap (ZSTDMI_decompressBatchAsync: the work buffers were sized once, from the caller's limits in the status words kStCap*): entry i is
// refused — workSpace_tooSmall, nothing of it in the lists — iff the INCLUSIVE sum over the entries 0 .. i of frames, blocks or
// literal-scratch bytes exceeds its limit.  The sums run over every entry the walk marked kBatchDecode, refused ones included, so every
// decodable entry behind a refused one is refused too, the admitted ones are a prefix whose places are the exclusive sums as always,
// and the counts filed are the largest inclusive sums inside the limits.  (The kernel itself is the template: kCap = false is the kernel
// as it always was, argument list included — which is why the limits ride in the status words.)
template <bool kCap = false>
__global__ __launch_bounds__(256) void batch_scan_kernel(BatchEntryOut* __restrict__ out, u32 nEntries, u32* __restrict__ status)
{
    __shared__ u64 shF[4], shB[4], shC[4];
    const u32 tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    u64 carryF = 0, carryB = 0, carryC = 0;
    u64 capF = 0, capB = 0, capC = 0, admF = 0, admB = 0, admC = 0;
    if constexpr (kCap) { capF = status[kStCapFrames]; capB = status[kStCapBlocks]; capC = (u64)status[kStCapContentLo] | ((u64)status[kStCapContentHi] << 32); }
    for (u32 base = 0; base < nEntries; base += 256) {
        const u32 i = base + tid;
        u64 f = 0, b = 0, c = 0;
        if (i < nEntries && out[i].state == kBatchDecode) { f = out[i].nFrames; b = out[i].nBlocks; c = out[i].result; }
        u64 fi = f, bi = b, ci = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 tf = __shfl_up(fi, d), tb = __shfl_up(bi, d), tc = __shfl_up(ci, d);
            if ((int)lane >= d) { fi += tf; bi += tb; ci += tc; }
        }
        if (lane == 63) { shF[wave] = fi; shB[wave] = bi; shC[wave] = ci; }
        __syncthreads();
        u64 bf = carryF, bb = carryB, bc = carryC, af = 0, ab = 0, ac = 0;
        for (u32 w = 0; w < 4; ++w) { if (w < wave) { bf += shF[w]; bb += shB[w]; bc += shC[w]; } af += shF[w]; ab += shB[w]; ac += shC[w]; }
        if (i < nEntries) { out[i].firstFrame = (u32)(bf + fi - f); out[i].firstBlock = (u32)(bb + bi - b); out[i].scratchOff = bc + ci - c; }
        carryF += af; carryB += ab; carryC += ac;
        __syncthreads();
        if constexpr (kCap) {
            const u64 inF = bf + fi, inB = bb + bi, inC = bc + ci;
            const bool within = inF <= capF && inB <= capB && inC <= capC;
            if (!within && i < nEntries && out[i].state == kBatchDecode) { out[i].state = kBatchDone; out[i].open = 0; out[i].result = (u64)0 - (u64)kErrWorkSpaceTooSmall; }
            // the largest inclusive sums inside the limits (each sum is monotone in the entry order): through the three arrays once more
            u64 mF = within ? inF : 0, mB = within ? inB : 0, mC = within ? inC : 0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const u64 tf = __shfl_xor(mF, d), tb = __shfl_xor(mB, d), tc = __shfl_xor(mC, d);
                mF = tf > mF ? tf : mF; mB = tb > mB ? tb : mB; mC = tc > mC ? tc : mC;
            }
            if (lane == 0) { shF[wave] = mF; shB[wave] = mB; shC[wave] = mC; }
            __syncthreads();
            for (u32 w = 0; w < 4; ++w) { admF = shF[w] > admF ? shF[w] : admF; admB = shB[w] > admB ? shB[w] : admB; admC = shC[w] > admC ? shC[w] : admC; }
            __syncthreads();
        }
    }
    if constexpr (kCap) { carryF = admF; carryB = admB; carryC = admC; }
    if (tid == 0) {
        const bool tooMany = carryF > (1u << 26) || carryB > 0xFFFFFFF0ull;
        status[kStFrames] = tooMany ? 0u : (u32)carryF; status[kStBlocks] = tooMany ? 0u : (u32)carryB; status[kStErr] = tooMany ? (u32)kErrMemoryAllocation : 0u;
        status[kStTotalLo] = (u32)carryC; status[kStTotalHi] = (u32)(carryC >> 32); status[kStUnsized] = 0; status[kStUsable] = 0;
    }
}

// emit: the same walk again, into the lists.  A frame's content goes to the entry's destination plus the frame's place inside the
// entry; its literal scratch is the scratch prefix sum (in a single call both are the same number; here they are not)
// kOpen: every frame's literal room goes to rooms[] (what the count summed: the scratch prefix advances by it), and in an open entry
// every frame whose place is not final yet is marked kFrameOpen: an unsized frame, every frame behind one — sized ones included: the
// dstOff they get here is computed from bounds —, and a frame the capacity does not admit (only batch_rescan refuses the entry, so that
// a failing block's error still outranks dstSize_tooSmall).  What is left — sized frames in front of the first unsized one, inside the
// capacity — is where it will stay.  An entry's first frame starts at the entry's destination whatever its header says, but an unsized
// one has not been held to the capacity: FrameDesc::unsized keeps it from being written early (block_link).
template <bool kSet, bool kOpen = false>
__device__ __forceinline__ void batch_walk_emit_body(const u8* __restrict__ src, const BatchEntryIn* __restrict__ in, const BatchEntryOut* __restrict__ out, u32 nEntries,
                                                     FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks, const DictSlot* __restrict__ slots, u32 nSet,
                                                     u64* __restrict__ rooms = nullptr)
{
    const u32 e = blockIdx.x * 64 + threadIdx.x;
    if (e >= nEntries) return;
    const BatchEntryOut R = out[e];
    if (R.state != kBatchDecode) return;
    const BatchEntryIn E = in[e];
    const u64 end = E.srcOff + E.srcSize;
    u64 pos = E.srcOff, dstOff = E.dstOff, scr = R.scratchOff; u32 idx = R.firstFrame, blk = R.firstBlock;
    bool behind = false;                                        // (kOpen) an unsized frame lies in front
    while (end - pos >= 5 && idx < R.firstFrame + R.nFrames) {
        ChainOut o;
        const u32 st = emit_frame(src, end, pos, o, idx, blk, dstOff, frames, blocks);
        if (st >= 2) return;                                   // cannot happen: the counting pass walked the same bytes
        if (st == 0) {
            frames[idx].scratchOff = scr;
            if constexpr (kSet) { u32 inSet, wrong; frames[idx].dictSlot = dictset_select(slots, nSet, o.dictID, &inSet, &wrong); }     // (the count refused a wrong one)
            u64 room = o.content;
            if constexpr (kOpen) {
                if (R.open) {
                    room = o.content < E.dstCap ? o.content : E.dstCap;
                    const bool final = !behind && !o.unsized && dstOff - E.dstOff + o.content <= E.dstCap;
                    if (!final) frames[idx].unsized = o.unsized | kFrameOpen;
                    behind |= o.unsized != 0;
                }
                rooms[idx] = room;
            }
            idx++; blk += o.nbBlocks; dstOff += o.content; scr += room;
        }
        pos = o.next;
    }
}
template <bool kSet, bool kOpen>
__global__ __launch_bounds__(64) void batch_walk_emit_kernel(const u8* __restrict__ src, const BatchEntryIn* __restrict__ in, const BatchEntryOut* __restrict__ out, u32 nEntries,
                                                             FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks, const DictSlot* __restrict__ slots, u32 nSet,
                                                             u64* __restrict__ rooms)
{
    batch_walk_emit_body<kSet, kOpen>(src, in, out, nEntries, frames, blocks, kSet ? slots : nullptr, kSet ? nSet : 0, kOpen ? rooms : nullptr);
}

// ------------------------------------------------------------------------------------------------
// batch_rescan (ZSTDMI_DCtx_setBatchUnsized): behind block_offsets, in front of everything that writes into a destination
// ------------------------------------------------------------------------------------------------
// One wave per entry; an entry without an unsized frame is left at once (its places have been final since the walk).  The others: 64
// frames a step, every lane one frame's regenerated size (block_offsets has put it into dstSize), the rule of zmi_batch_rescan.h:
// dstOff = the entry's destination + the sizes in front.  An entry that does not fit its capacity — or that had a block without room in
// the clamped literal scratch, which cannot fit — answers dstSize_tooSmall and every frame of it is marked bad, as is every frame of
// an entry with a failed frame: place_literals, exec_matches, the origin path and the literal decoder pass over bad frames, so nothing
// of such an entry is written behind this kernel.  A block's error, folded behind the run (batch_fold_kernel), replaces the answer.
__global__ __launch_bounds__(64) void batch_rescan_kernel(const BatchEntryIn* __restrict__ in, BatchEntryOut* __restrict__ out, u32 nEntries, FrameDesc* __restrict__ frames)
{
    const u32 e = blockIdx.x, lane = threadIdx.x;
    if (e >= nEntries) return;
    if (uniform(out[e].state) != kBatchDecode || !uniform(out[e].open)) return;
    const u32 first = uniform(out[e].firstFrame), n = uniform(out[e].nFrames);
    const u64 entryOff = in[e].dstOff, cap = in[e].dstCap;
    u64 carry = 0; bool anyBad = false, noRoom = false;
    for (u32 k0 = 0; k0 < n; k0 += kRescanStep) {
        const bool have = k0 + lane < n;
        u64 mine = 0; u32 bad = 0, flags = 0;
        if (have) { const FrameDesc& F = frames[first + k0 + lane]; mine = F.dstSize; bad = F.bad; flags = F.unsized; }
        anyBad |= ballot(bad != 0) != 0; noRoom |= ballot((flags & kFrameNoRoom) != 0) != 0;
        u64 incl = mine;
#pragma unroll
        for (u32 d = 1; d < kRescanStep; d <<= 1) incl = rescan_round(incl, __shfl_up(incl, d), lane, d);
        const u64 before = rescan_before(carry, __shfl_up(incl, 1), lane);
        if (have) frames[first + k0 + lane].dstOff = rescan_place(entryOff, before);
        carry = rescan_add(carry, __shfl(incl, 63));
    }
    const bool fits = rescan_fits(carry, cap) && !noRoom;
    if (!fits || anyBad) for (u32 k = lane; k < n; k += 64) frames[first + k].bad = 1;
    if (lane == 0) out[e].result = fits ? carry : (u64)0 - (u64)kErrDstSizeTooSmall;
}
void launch_batch_rescan(const BatchEntryIn* in, BatchEntryOut* out, u32 nEntries, FrameDesc* frames, hipStream_t stream)
{
    hipLaunchKernelGGL(batch_rescan_kernel, dim3(nEntries), dim3(64), 0, stream, in, out, nEntries, frames);
}

// fold: an entry's error is the smallest key of its blocks — its first failing block's first error, what the single call reports
__global__ __launch_bounds__(64) void batch_fold_kernel(BatchEntryOut* __restrict__ out, u32 nEntries, const u64* __restrict__ keys)
{
    const u32 e = blockIdx.x * 64 + threadIdx.x;
    if (e >= nEntries) return;
    if (out[e].state != kBatchDecode) return;
    const u32 first = out[e].firstBlock, nb = out[e].nBlocks;
    u64 key = ~0ull;
    for (u32 k = 0; k < nb; ++k) { const u64 v = keys[first + k]; key = v < key ? v : key; }
    if (key != ~0ull) out[e].result = (u64)0 - (key & 0xFFFFull);
}

void launch_batch_walk_count(const u8* src, const BatchEntryIn* in, BatchEntryOut* out, u32 nEntries, const DecodeDict& dd, u64 aloneAbove, u32* status, hipStream_t stream,
                             bool open, bool caps)
{
    // (a set instance finds each frame's dictionary by its dictID)
    with_flags([&](auto set, auto op) {
        hipLaunchKernelGGL((batch_walk_count_kernel<set(), op()>), dim3((nEntries + 63) / 64), dim3(64), 0, stream, src, in, out, nEntries, dd.dictID, aloneAbove, dd.slots, dd.nSet, status);
    }, dd.slots != nullptr, open);
    if (caps) hipLaunchKernelGGL(batch_scan_kernel<true>, dim3(1), dim3(256), 0, stream, out, nEntries, status);
    else hipLaunchKernelGGL(batch_scan_kernel<>, dim3(1), dim3(256), 0, stream, out, nEntries, status);
}

// ------------------------------------------------------------------------------------------------
// a batch enqueued from the device (ZSTDMI_decompressBatchAsync): what the host's loops over the entries and its small
// host -> device copies do in ZSTDMI_decompressBatch, as kernels
// ------------------------------------------------------------------------------------------------
// plan, one lane per entry: the caller's four arrays -> BatchEntryIn.  The bases are constants: sources and destinations are offsets
// from kAsyncBase (zmi_host.h; no decoder kernel treats a null base specially, but a base that is a valid non-null constant keeps
// every `base + offset` an ordinary address computation), so an offset is the device address minus kAsyncBase.  An entry that never
// reaches the walk gets its verdict here, in decompress_batch_impl's order — a size above `bound` (which includes an error code another
// call left in the sizes column), then a size without a source, both srcSize_wrong — and walks as an empty entry.  A null destination
// has no room, as in the host's loop.
__global__ __launch_bounds__(64) void batch_plan_d_kernel(const void* const* __restrict__ srcs, const size_t* __restrict__ sizes, void* const* __restrict__ dsts,
                                                          const size_t* __restrict__ caps, u32 n, u64 bound, BatchEntryIn* __restrict__ in, u32* __restrict__ verdict)
{
    const u32 e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    const u64 src = (u64)(uintptr_t)srcs[e], size = (u64)sizes[e], dst = (u64)(uintptr_t)dsts[e], cap = (u64)caps[e];
    const u32 v = (size > bound || (size && !src)) ? (u32)kErrSrcSizeWrong : 0u;
    const bool walk = !v && size != 0;
    BatchEntryIn E;
    E.srcOff = walk ? src - kAsyncBase : 0; E.srcSize = walk ? size : 0;
    E.dstOff = dst ? dst - kAsyncBase : 0; E.dstCap = dst ? cap : 0;
    in[e] = E; verdict[e] = v;
}
// init, one wave: the status words as status_reset leaves them, and what the host copies into them behind it: the block keys' address,
// the literal rooms' address and the dump area's offset, the caller's limits
__global__ __launch_bounds__(64) void batch_init_d_kernel(u32* __restrict__ status, u64 blockKeys, u64 rooms, u64 dumpOff, u32 capFrames, u32 capBlocks, u64 capContent, u64 capSeq)
{
    for (u32 w = threadIdx.x; w < kStWords; w += 64) {
        u32 v = 0;
        switch (w) {
        case kStErrKeyLo: case kStErrKeyHi: v = 0xFFFFFFFFu; break;
        case kStBlockKeysLo: v = (u32)blockKeys; break;
        case kStBlockKeysHi: v = (u32)(blockKeys >> 32); break;
        case kStRoomLo: v = (u32)rooms; break;
        case kStRoomHi: v = (u32)(rooms >> 32); break;
        case kStDumpLo: v = (u32)dumpOff; break;
        case kStDumpHi: v = (u32)(dumpOff >> 32); break;
        case kStCapFrames: v = capFrames; break;
        case kStCapBlocks: v = capBlocks; break;
        case kStCapContentLo: v = (u32)capContent; break;
        case kStCapContentHi: v = (u32)(capContent >> 32); break;
        case kStCapSeqLo: v = (u32)capSeq; break;
        case kStCapSeqHi: v = (u32)(capSeq >> 32); break;
        default: break;
        }
        status[w] = v;
    }
}
// finish, one lane per entry: the caller's sizes column from the plan's verdict or the entry's answer
__global__ __launch_bounds__(64) void batch_finish_d_kernel(const BatchEntryOut* __restrict__ out, const u32* __restrict__ verdict, u32 n, size_t* __restrict__ dstSizes)
{
    const u32 e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    const u32 v = verdict[e];
    dstSizes[e] = v ? (size_t)((u64)0 - (u64)v) : (size_t)out[e].result;
}
void launch_batch_plan_d(const void* const* srcs, const size_t* sizes, void* const* dsts, const size_t* caps, u32 n, u64 bound, BatchEntryIn* in, u32* verdict, hipStream_t stream)
{
    hipLaunchKernelGGL(batch_plan_d_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, srcs, sizes, dsts, caps, n, bound, in, verdict);
}
void launch_batch_init_d(u32* status, const u64* blockKeys, const u64* rooms, u64 dumpOff, const BatchLimitsD& lim, hipStream_t stream)
{
    hipLaunchKernelGGL(batch_init_d_kernel, dim3(1), dim3(64), 0, stream, status, (u64)(uintptr_t)blockKeys, (u64)(uintptr_t)rooms, dumpOff, lim.frames, lim.blocks, lim.content, lim.sequences);
}
void launch_batch_finish_d(const BatchEntryOut* out, const u32* verdict, u32 n, size_t* dstSizes, hipStream_t stream)
{
    hipLaunchKernelGGL(batch_finish_d_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, out, verdict, n, dstSizes);
}
void launch_batch_walk_emit(const u8* src, const BatchEntryIn* in, const BatchEntryOut* out, u32 nEntries, FrameDesc* frames, BlockDesc* blocks, hipStream_t stream,
                            const DecodeDict& dd, u64* rooms)
{
    with_flags([&](auto set, auto op) {          // (rooms: the open instances)
        hipLaunchKernelGGL((batch_walk_emit_kernel<set(), op()>), dim3((nEntries + 63) / 64), dim3(64), 0, stream, src, in, out, nEntries, frames, blocks, dd.slots, dd.nSet, rooms);
    }, dd.slots != nullptr, rooms != nullptr);
}
void launch_batch_fold(BatchEntryOut* out, u32 nEntries, const u64* keys, hipStream_t stream)
{
    hipLaunchKernelGGL(batch_fold_kernel, dim3((nEntries + 63) / 64), dim3(64), 0, stream, out, nEntries, keys);
}

// ------------------------------------------------------------------------------------------------
// a range of a seekable stream (ZSTDMI_decompressRange): seek table + (offset, length) -> the batch walk's entries
// ------------------------------------------------------------------------------------------------
// exclusive prefix of (a, b) over the 1024 lanes of a workgroup, and the workgroup's sums
__device__ inline void block_scan2(u64 a, u64 b, u64* __restrict__ shA, u64* __restrict__ shB, u64& exA, u64& exB, u64& allA, u64& allB)
{
    const u32 lane = lane_id(), wave = wave_id();
    u64 ai = a, bi = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 ta = __shfl_up(ai, d), tb = __shfl_up(bi, d);
        if ((int)lane >= d) { ai += ta; bi += tb; }
    }
    if (lane == 63) { shA[wave] = ai; shB[wave] = bi; }
    __syncthreads();
    exA = ai - a; exB = bi - b; allA = 0; allB = 0;
    for (u32 w = 0; w < 16; ++w) { if (w < wave) { exA += shA[w]; exB += shB[w]; } allA += shA[w]; allB += shB[w]; }
    __syncthreads();
}

// select (single workgroup): `tab` = the table's skippable frame (tableBytes of it: header, n entries of `stride` bytes — a checksum
// behind the two sizes is skipped —, footer; the host has read the footer).  Checks the header and that the compressed sizes add up to
// the bytes in front of the table — so every offset derived from them lies inside the stream —, sums both columns, and finds the
// entries with content that meet [offset, offset + length): their first and last, and those two's places.  -> the summary words.
__global__ __launch_bounds__(1024) void seek_select_kernel(const u8* __restrict__ tab, u64 tableBytes, u32 n, u32 stride, u64 srcSize,
                                                           u64 offset, u64 length, u64* __restrict__ sum)
{
    __shared__ u64 shA[16], shB[16], rec[6];
    __shared__ u32 tileFirst, tileLast, firstIdx, lastIdx, nMeet;
    const u32 tid = threadIdx.x;
    if (tid == 0) { firstIdx = 0xFFFFFFFFu; lastIdx = 0; nMeet = 0; for (u32 k = 0; k < 6; ++k) rec[k] = 0; }
    u64 end = offset + length; if (end < offset) end = ~0ull;
    u64 carryC = 0, carryD = 0;
    for (u32 base = 0; base < n; base += 1024) {
        if (tid == 0) { tileFirst = 0xFFFFFFFFu; tileLast = 0; }
        const u32 i = base + tid;
        u64 c = 0, d = 0;
        if (i < n) { const u8* p = tab + 8 + (u64)i * stride; c = readLE32(p); d = readLE32(p + 4); }
        u64 exC, exD, allC, allD;
        block_scan2(c, d, shA, shB, exC, exD, allC, allD);
        const u64 cOff = carryC + exC, dOff = carryD + exD;
        const bool meet = d > 0 && length > 0 && dOff < end && dOff + d > offset;
        if (meet) { atomicMin(&tileFirst, i); atomicMax(&tileLast, i + 1); atomicAdd(&nMeet, 1u); }
        carryC += allC; carryD += allD;
        __syncthreads();
        if (meet && i == tileFirst && firstIdx == 0xFFFFFFFFu) { firstIdx = i; rec[0] = cOff; rec[1] = dOff; rec[2] = d; }
        if (meet && i + 1 == tileLast) { lastIdx = i; rec[3] = cOff + c; rec[4] = dOff; rec[5] = d; }     // (a later tile's overwrites an earlier one's)
        __syncthreads();
    }
    if (tid == 0) {
        u32 err = 0;
        if (readLE32(tab) != 0x184D2A5Eu || (u64)readLE32(tab + 4) != tableBytes - 8) err = kErrPrefixUnknown;
        else if (carryC != srcSize - tableBytes) err = kErrCorruption;
        sum[kSeekErr] = err; sum[kSeekTotal] = carryD; sum[kSeekMeet] = nMeet; sum[kSeekFirst] = firstIdx; sum[kSeekLast] = lastIdx;
        sum[kSeekCLo] = rec[0]; sum[kSeekDFirst] = rec[1]; sum[kSeekSizeFirst] = rec[2];
        sum[kSeekCHi] = rec[3]; sum[kSeekDLast] = rec[4]; sum[kSeekSizeLast] = rec[5];
        sum[kSeekKey] = ~0ull; sum[kSeekAlone] = 0;
    }
}

// emit (single workgroup, the selected entries only): one BatchEntryIn per table entry first .. first + nSel - 1.  Sources are offsets
// from the first selected frame; a frame wholly inside the range decodes to its place in dst (dstBias + its content offset - offset),
// the first and the last one — where the range cuts them — to their slots in the edge buffer (edgeBias, edgeBias + slot1).  An entry
// without content (a skippable frame) becomes an empty entry.  Every entry's capacity is its table size: the walk refuses more.
__global__ __launch_bounds__(1024) void seek_emit_kernel(const u8* __restrict__ tab, u32 stride, u32 first, u32 nSel, u64 dFirst, u64 offset,
                                                         u64 dstBias, u64 edgeBias, u64 slot1, u32 cutFirst, u32 cutLast, BatchEntryIn* __restrict__ out)
{
    __shared__ u64 shA[16], shB[16];
    const u32 tid = threadIdx.x;
    u64 carryC = 0, carryD = dFirst;
    for (u32 base = 0; base < nSel; base += 1024) {
        const u32 i = base + tid;
        u64 c = 0, d = 0;
        if (i < nSel) { const u8* p = tab + 8 + (u64)(first + i) * stride; c = readLE32(p); d = readLE32(p + 4); }
        u64 exC, exD, allC, allD;
        block_scan2(c, d, shA, shB, exC, exD, allC, allD);
        if (i < nSel) {
            const u64 dOff = carryD + exD;
            BatchEntryIn e; e.srcOff = carryC + exC; e.srcSize = d ? c : 0; e.dstCap = d;
            if (i == 0 && cutFirst) e.dstOff = edgeBias;
            else if (i == nSel - 1 && cutLast) e.dstOff = edgeBias + slot1;
            else e.dstOff = dstBias + (d ? dOff - offset : 0);
            out[i] = e;
        }
        carryC += allC; carryD += allD;
    }
}

// check: an entry that failed, or whose content is not the size its table entry names, fails the call (the first such entry's error;
// a frame larger than its table size was refused by the walk with dstSize_tooSmall: corruption of the table); the others are counted
__global__ __launch_bounds__(256) void range_check_kernel(const BatchEntryIn* __restrict__ in, const BatchEntryOut* __restrict__ out, u32 nEntries, u64* __restrict__ sum)
{
    const u32 e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nEntries) return;
    const BatchEntryOut o = out[e];
    if (o.state == kBatchAlone) { atomicAdd((unsigned long long*)&sum[kSeekAlone], 1ull); return; }
    u32 err = 0;
    if (o.result > (u64)0 - (u64)kErrMaxCode) { err = (u32)((u64)0 - o.result); if (err == kErrDstSizeTooSmall) err = kErrCorruption; }
    else if (o.result != in[e].dstCap) err = kErrCorruption;
    if (err) atomicMin((unsigned long long*)&sum[kSeekKey], ((unsigned long long)e << 16) | err);
}

// clip: the wanted part of each edge frame from the edge buffer to its place in dst (blockIdx.y = the job)
__global__ __launch_bounds__(256) void range_clip_kernel(u8* __restrict__ dst, const u8* __restrict__ edge, ClipJob j0, ClipJob j1)
{
    const ClipJob j = blockIdx.y ? j1 : j0;
    if (!j.len) return;
    u8* const d = dst + j.to; const u8* const s = edge + j.from;
    const u64 gtid = (u64)blockIdx.x * 256 + threadIdx.x, nThreads = (u64)gridDim.x * 256;
    // head: bring d to 16-byte alignment, then 16 B stores fed by unaligned loads
    u64 head = (16 - ((uintptr_t)d & 15)) & 15;
    if (head > j.len) head = j.len;
    if (gtid < head) d[gtid] = s[gtid];
    const u64 body = (j.len - head) >> 4;
    uint4* const d4 = reinterpret_cast<uint4*>(d + head);
    const u8* const sb = s + head;
    for (u64 i = gtid; i < body; i += nThreads) {
        uint4 v;
        v.x = readLE32(sb + 16 * i); v.y = readLE32(sb + 16 * i + 4); v.z = readLE32(sb + 16 * i + 8); v.w = readLE32(sb + 16 * i + 12);
        d4[i] = v;
    }
    const u64 done = head + (body << 4);
    if (gtid < j.len - done) d[done + gtid] = s[done + gtid];
}

void launch_seek_select(const u8* tab, u64 tableBytes, u32 n, u32 stride, u64 srcSize, u64 offset, u64 length, u64* sum, hipStream_t stream)
{
    hipLaunchKernelGGL(seek_select_kernel, dim3(1), dim3(1024), 0, stream, tab, tableBytes, n, stride, srcSize, offset, length, sum);
}
void launch_seek_emit(const u8* tab, u32 stride, u32 first, u32 nSel, u64 dFirst, u64 offset, u64 dstBias, u64 edgeBias, u64 slot1, u32 cutFirst, u32 cutLast,
                      BatchEntryIn* out, hipStream_t stream)
{
    hipLaunchKernelGGL(seek_emit_kernel, dim3(1), dim3(1024), 0, stream, tab, stride, first, nSel, dFirst, offset, dstBias, edgeBias, slot1, cutFirst, cutLast, out);
}
void launch_range_check(const BatchEntryIn* in, const BatchEntryOut* out, u32 nEntries, u64* sum, hipStream_t stream)
{
    hipLaunchKernelGGL(range_check_kernel, dim3((nEntries + 255) / 256), dim3(256), 0, stream, in, out, nEntries, sum);
}
void launch_range_clip(u8* dst, const u8* edge, ClipJob j0, ClipJob j1, hipStream_t stream)
{
    const u64 most = j0.len > j1.len ? j0.len : j1.len;
    if (!most) return;
    const u64 want = (most / 16 + 255) / 256 + 1;
    hipLaunchKernelGGL(range_clip_kernel, dim3((u32)(want < 2048 ? want : 2048), 2), dim3(256), 0, stream, dst, edge, j0, j1);
}

// ---- the status words at both ends of a call: set by a store per word, handed to the host through its pinned block (zmi_host.h) ----
__global__ __launch_bounds__(128) void status_reset_kernel(u32* __restrict__ status)
{
    const u32 w = threadIdx.x;
    if (w < kStWords) status[w] = (w == kStErrKeyLo || w == kStErrKeyHi) ? 0xFFFFFFFFu : 0u;
}
__global__ __launch_bounds__(128) void status_mirror_kernel(const u32* __restrict__ status, u32* __restrict__ pinned)
{
    const u32 w = threadIdx.x;
    if (w < kStWords) pinned[w] = status[w];
}
void launch_status_reset(u32* status, hipStream_t stream) { hipLaunchKernelGGL(status_reset_kernel, dim3(1), dim3(128), 0, stream, status); }
void launch_status_mirror(const u32* status, u32* pinned, hipStream_t stream) { hipLaunchKernelGGL(status_mirror_kernel, dim3(1), dim3(128), 0, stream, status, pinned); }

size_t decode_walk_workspace_bytes(u64 srcSize)
{
    const u64 nSeg = (srcSize + (1ull << kSegLog) - 1) >> kSegLog;
    return (size_t)(nSeg * (sizeof(SegInfo) + 2 * sizeof(u32) + sizeof(u64)) + 256);
}

struct WalkWs { SegInfo* segs; u64* dstBase; u32* frameBase; u32* blockBase; u32 nSeg; };
static WalkWs walk_ws(u8* walkWs, u64 srcSize)
{
    WalkWs w; w.nSeg = (u32)((srcSize + (1ull << kSegLog) - 1) >> kSegLog);
    w.segs = reinterpret_cast<SegInfo*>(walkWs);
    w.dstBase = reinterpret_cast<u64*>(walkWs + (size_t)w.nSeg * sizeof(SegInfo));
    w.frameBase = reinterpret_cast<u32*>(walkWs + (size_t)w.nSeg * (sizeof(SegInfo) + sizeof(u64)));
    w.blockBase = w.frameBase + w.nSeg;
    return w;
}
// count: frames, blocks, content bytes -> status (the host then sizes the lists)
void launch_frame_walk_count(const u8* src, u64 srcSize, u32 maxFrames, u32* status, u8* walkWs, hipStream_t stream, u32* pinned)
{
    const WalkWs w = walk_ws(walkWs, srcSize);
    hipLaunchKernelGGL(walk_segments_kernel, dim3(w.nSeg), dim3(64), 0, stream, src, srcSize, w.segs, w.nSeg);
    hipLaunchKernelGGL(walk_link_kernel, dim3(1), dim3(1024), 0, stream, w.segs, w.nSeg, srcSize, maxFrames, w.frameBase, w.blockBase, w.dstBase, status, pinned);
}
void launch_frame_walk_emit(const u8* src, u64 srcSize, FrameDesc* frames, BlockDesc* blocks, u8* walkWs, hipStream_t stream)
{
    const WalkWs w = walk_ws(walkWs, srcSize);
    hipLaunchKernelGGL(walk_emit_kernel, dim3((w.nSeg + 255) / 256), dim3(256), 0, stream, src, srcSize, w.segs, w.nSeg, w.frameBase, w.blockBase, w.dstBase, frames, blocks);
}
void launch_frame_walk_serial(const u8* src, u64 srcSize, FrameDesc* frames, BlockDesc* blocks, u32 maxFrames, u32* status, const DecodeDict& dd, u32 emit, hipStream_t stream)
{
    with_flags([&](auto set) {
        hipLaunchKernelGGL(frame_walk_serial_kernel<set()>, dim3(1), dim3(64), 0, stream, src, srcSize, frames, blocks, maxFrames, status, dd.dictID, emit, dd.slots, dd.nSet);
    }, dd.slots != nullptr);
}

// ------------------------------------------------------------------------------------------------
// block_parse: the two section headers of every compressed block, one lane per block
// ------------------------------------------------------------------------------------------------
// (kDev: list_count, zmi_decode.h — the kernel itself is the template, so that kDev = false stays the kernel it always was)
// seqPlane (null: none; seq_scan_kernel): one u32 per block, the sequences it will file records for — nbSeq of a compressed block
// without an error, else 0.  Every block's word is written here; block_link zeroes the word of a block it fails or makes a phantom.
template <bool kDev = false>
__global__ __launch_bounds__(256) void block_parse_kernel(const u8* __restrict__ src, BlockDesc* __restrict__ blocks, u32 nBlocks, u32* __restrict__ status,
                                                          u32* __restrict__ seqPlane)
{
    const u32 bi = blockIdx.x * 256 + threadIdx.x;
    if (bi >= list_count<kDev>(nBlocks, status, kStBlocks)) return;
    BlockDesc& B = blocks[bi];
    if (B.type != 2) { if (seqPlane) seqPlane[bi] = 0; return; }
    const u32 bsz = B.bsz;
    u32 err = 0;
    do {
        if (bsz >= kBlockMax) { err = kErrSrcSizeWrong; break; }          // ZSTD_decompressBlock_internal, U/ZstdDecompressBlock.cs:3095-3098
        if (bsz < 3) { err = kErrCorruption; break; }                     // MIN_CBLOCK_SIZE, :90-93
        const u8* const b = src + B.srcOff;
        const LitHeader lh = parse_lit_header(b, bsz);
        if (lh.err) { err = lh.err; break; }
        B.litType = (u8)lh.type; B.litSingle = (u8)lh.single; B.litSize = lh.litSize; B.litCSize = lh.litCSize; B.lhSize = lh.lhSize;
        u32 bp = lh.type >= 2 ? lh.lhSize + lh.litCSize : lh.type == 0 ? lh.lhSize + lh.litSize : lh.lhSize + 1;
        // ---- sequences header (ZSTD_decodeSeqHeaders, :1845-1943) ----
        if (bp >= bsz) { err = kErrSrcSizeWrong; break; }
        u32 nbSeq = b[bp++];
        if (!nbSeq) { if (bp != bsz) { err = kErrSrcSizeWrong; break; } B.nbSeq = 0; B.outSize = lh.litSize; break; }
        if (nbSeq > 0x7F) {
            if (nbSeq == 0xFF) { if (bp + 2 > bsz) { err = kErrSrcSizeWrong; break; } nbSeq = readLE16(b + bp) + 0x7F00; bp += 2; }
            else { if (bp >= bsz) { err = kErrSrcSizeWrong; break; } nbSeq = ((nbSeq - 0x80) << 8) + b[bp++]; }
        }
        if (bp + 1 > bsz) { err = kErrSrcSizeWrong; break; }
        const u32 modes = b[bp++];
        B.nbSeq = nbSeq; B.modes = modes;
        const u32 maxSym[3] = { 35, 31, 52 };
#pragma unroll
        for (u32 t = 0; t < 3; ++t) {                                      // LL, OF, ML in that order
            const u32 mode = (modes >> (6 - 2 * t)) & 3;
            B.tblOff[t] = bp;
            if (mode == 1) { if (bp >= bsz) { err = kErrCorruption; break; } bp += 1; }
            else if (mode == 2) {
                u32 maxSV = maxSym[t], tableLog = 0;
                const u32 hs = read_ncount_t<false>(nullptr, &maxSV, &tableLog, b + bp, bsz - bp);
                if (!hs) { err = kErrCorruption; break; }
                bp += hs;
            }
        }
        if (err) break;
        B.bitsOff = bp;
    } while (false);
    if (err) { B.err = err; report_error(status, bi, kStageParse, err); }
    if (seqPlane) seqPlane[bi] = (err || B.err) ? 0u : B.nbSeq;
}

// ------------------------------------------------------------------------------------------------
// block_link: table provenance inside a frame, literal offsets; one wave per frame, 64 blocks at a time
// ------------------------------------------------------------------------------------------------
// frames of up to kLinkSmall blocks (a stream of single-block 64 KiB frames has 16 384 of them per GiB): one LANE per frame, the
// blocks one after the other — a wave per frame costs three times as much there; longer frames: block_link_kernel below
constexpr u32 kLinkSmall = 4;
// kSet: "a formatted dictionary" is a property of the frame's own dictionary (slots[F.dictSlot]); a lane has a frame of its own here,
// so haveDict is per lane.  (The kernel itself is the template: as a wrapper around an inlined body the parent's instance took one SGPR more.)
// kOpen (a batch with entries that hold unsized frames, ZSTDMI_DCtx_setBatchUnsized): a frame's scratch is not dstSize long but as
// long as the walk's rooms[] says (the status words name the array): for a frame of such an entry the smaller of dstSize and the
// entry's capacity.  dstSize stays the bound: literals beyond IT are corruption.  Literals that fit the bound but not the room mean
// that the entry does not fit its capacity (its output holds at least its literals): the block is sent to the scratch's dump area
// (kStDumpLo), where its literals are decoded for their errors' sake and never read, and the frame is marked kFrameNoRoom, on which
// batch_rescan answers dstSize_tooSmall for the entry unless a block's error outranks it.  kOpen = false is the kernel as it always was.
// a block's litRel that makes scratch + scratchOff + litRel + frame x kLitSkew the dump area (offsets are sums modulo 2^64)
__device__ __forceinline__ u64 dump_lit_rel(const u32* __restrict__ status, u64 scratchOff, u32 frame)
{
    return ((u64)status[kStDumpLo] | ((u64)status[kStDumpHi] << 32)) - scratchOff - (u64)frame * kLitSkew;
}
__device__ __forceinline__ const u64* lit_rooms(const u32* __restrict__ status)
{
    return reinterpret_cast<const u64*>((uintptr_t)((u64)status[kStRoomLo] | ((u64)status[kStRoomHi] << 32)));
}
template <bool kSet, bool kOpen = false, bool kDev = false>
__global__ __launch_bounds__(64) void block_link_small_kernel(FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks, u32 nFrames, u32 haveDict,
                                                              u32 earlyLiterals, u32* __restrict__ status, const DictSlot* __restrict__ slots,
                                                              u32* __restrict__ seqPlane)
{
    const u32 f = blockIdx.x * 64 + threadIdx.x;
    if (f >= list_count<kDev>(nFrames, status, kStFrames)) return;
    FrameDesc& F = frames[f];
    if (F.nbBlocks > kLinkSmall) return;                       // (a wave of block_link_kernel takes it)
    if constexpr (kSet) haveDict = slots[F.dictSlot].formatted;
    u64 room = 0; u32 noRoom = 0;
    if constexpr (kOpen) room = lit_rooms(status)[f];
    // a formatted dictionary: every frame starts from its Huffman table and its three FSE tables (ZSTD_decompressBegin_usingDict,
    // U/ZstdDecompress.cs:1956-1990); without one nothing is defined before the frame's first block defines it
    u32 lastHuf = haveDict ? kDictBlock : kNoBlock;
    u32 lastTbl[3] = { lastHuf, lastHuf, lastHuf };
    u64 litAcc = 0; u32 hasSeq = 0;
    for (u32 k = 0; k < F.nbBlocks; ++k) {
        const u32 bi = F.firstBlock + k;
        BlockDesc& B = blocks[bi];
        if (B.type != 2 || B.err) continue;
        u32 err = 0;
        if (B.litType == 2) { lastHuf = bi; B.hufSrc = bi; }
        else if (B.litType == 3) { B.hufSrc = lastHuf; if (lastHuf == kNoBlock) err = kErrDictionaryCorrupted; }     // U/ZstdDecompressBlock.cs:197-207
        if (B.litType >= 2) {
            bool dumped = false;
            if (B.litSize > F.dstSize - litAcc) { err = err ? err : (u32)kErrCorruption; B.litRel = 0; }
            else if (kOpen && (litAcc > room || B.litSize > room - litAcc)) { B.litRel = dump_lit_rel(status, F.scratchOff, f); dumped = true; noRoom = 1; }
            else { B.litRel = litAcc; litAcc += B.litSize; }
            // (F.unsized: without a content size, or — a batch entry with such a frame — at a place that is not final yet)
            B.litInPlace = (B.nbSeq == 0 && !dumped && (!earlyLiterals || (k == 0 && !F.unsized))) ? 1u : 0u;
        }
        if (B.nbSeq) {
            hasSeq = 1;
#pragma unroll
            for (u32 t = 0; t < 3; ++t) {
                const u32 mode = (B.modes >> (6 - 2 * t)) & 3;
                if (mode == 3) { B.tblSrc[t] = lastTbl[t]; if (lastTbl[t] == kNoBlock) err = err ? err : (u32)kErrCorruption; }   // :1780-1786
                else { B.tblSrc[t] = bi; lastTbl[t] = bi; }
            }
        }
        if (err) {
            B.err = err; report_error(status, bi, B.litType >= 2 && (err == kErrDictionaryCorrupted || B.litSize > F.dstSize) ? kStageLiterals : kStageSequences, err);
            if (seqPlane) seqPlane[bi] = 0;     // (block_parse_kernel)
        }
    }
    F.hasSeq = hasSeq;
    if constexpr (kOpen) { if (noRoom) F.unsized |= kFrameNoRoom; }
    if (litAcc) atomicAdd(reinterpret_cast<unsigned long long*>(status + kStLitLo), (unsigned long long)litAcc);
    if (hasSeq && F.dstSize >= (1u << 20) && F.dstSize < (1ull << 30))
        atomicAdd(reinterpret_cast<unsigned long long*>(status + kStBigBins) + highbit32((u32)(F.dstSize >> 20)), (unsigned long long)F.dstSize);
}

// "the latest earlier block that ..." over the 64 blocks of a batch: the highest lane below mine in `mask`, else what earlier batches left
__device__ __forceinline__ u32 latest_before(u64 mask, u32 firstOfBatch, u32 carried, u32 lane)
{
    const u64 prior = mask & lanemask_lt();
    return prior ? firstOfBatch + (63u - (u32)__builtin_clzll(prior)) : carried;
}
// PH (a fragment of a segmented stream, ZSTDMI_DCtx_setStreamSegment): the frame's first `phantoms` blocks are earlier
// blocks of the stream, put in front again only because they DEFINE a table some later block may still use.  They are linked like
// any block — later blocks' hufSrc / tblSrc may name them — and then made to regenerate nothing: an RLE block of no bytes, which
// every later stage passes over; what they themselves lack (a table defined before the oldest carried block) is no error.  A fragment
// is one frame, linked by this kernel whatever its number of blocks.
// kSet: haveDict is the frame's own dictionary's (one frame per wave: uniform)
// kOpen: as in block_link_small_kernel (a block behind one without room has none either: the prefix sum counts them all)
template <bool PH, bool kSet = false, bool kOpen = false>
__device__ __forceinline__ void block_link_body(FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks, u32 nFrames, u32 haveDict,
                                                u32 earlyLiterals, u32* __restrict__ status, u32 phantoms, const DictSlot* __restrict__ slots, u32* __restrict__ seqPlane)
{
    const u32 f = blockIdx.x, lane = threadIdx.x;
    if (f >= nFrames) return;
    FrameDesc& F = frames[f];
    if constexpr (kSet) haveDict = uniform(slots[uniform(F.dictSlot)].formatted);
    const u32 first = uniform(F.firstBlock), nb = uniform(F.nbBlocks);
    if (!PH && nb <= kLinkSmall) return;                       // (a lane of block_link_small_kernel takes it)
    const u64 dstSize = F.dstSize;
    u64 room = 0, dumpRel = 0; u32 noRoom = 0;
    if constexpr (kOpen) { room = lit_rooms(status)[f]; dumpRel = dump_lit_rel(status, F.scratchOff, f); }
    // a formatted dictionary: every frame starts from its Huffman table and its three FSE tables (ZSTD_decompressBegin_usingDict,
    // U/ZstdDecompress.cs:1956-1990); without one nothing is defined before the frame's first block defines it
    u32 lastHuf = haveDict ? kDictBlock : kNoBlock;
    u32 lastTbl0 = lastHuf, lastTbl1 = lastHuf, lastTbl2 = lastHuf;
    u64 litAcc = 0; u32 hasSeq = 0;
    for (u32 k0 = 0; k0 < nb; k0 += 64) {
        const u32 bi = first + k0 + lane;
        const bool have = k0 + lane < nb;
        u32 litType = 0, litSize = 0, nbSeq = 0, modes = 0; bool live = false;
        if (have) {
            const BlockDesc& B = blocks[bi];
            live = B.type == 2 && !B.err;
            if (live) { litType = B.litType; litSize = B.litSize; nbSeq = B.nbSeq; modes = B.modes; }
        }
        const bool ph = PH && k0 + lane < phantoms;
        u32 err = 0;
        // the Huffman table of a treeless literals section is the latest one defined in front of it (U/ZstdDecompressBlock.cs:197-207)
        const u64 defHuf = ballot(live && litType == 2);
        u32 hufSrc = kNoBlock;
        if (live && litType == 2) hufSrc = bi;
        else if (live && litType == 3) { hufSrc = latest_before(defHuf, first + k0, lastHuf, lane); if (hufSrc == kNoBlock && !ph) err = kErrDictionaryCorrupted; }
        if (defHuf) lastHuf = first + k0 + (63u - (u32)__builtin_clzll(defHuf));
        // regenerated literals of Huffman-coded sections, one after the other in the frame's scratch (dstSize long: a block that does
        // not fit takes none of it and is an error, so the bound holds for every block whatever later kernels do with the frame)
        const bool coded = live && litType >= 2 && !ph;
        const u64 mine = coded ? litSize : 0u;
        u64 incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const u64 t = __shfl_up(incl, d); if ((int)lane >= d) incl += t; }
        u64 litRel = litAcc + incl - mine;
        bool dumped = false;
        if (coded && litRel + mine > dstSize) { err = err ? err : (u32)kErrCorruption; litRel = 0; }
        else if (kOpen && coded && litRel + mine > room) { litRel = dumpRel; dumped = true; }
        if constexpr (kOpen) { if (ballot(dumped)) noRoom = 1; }
        litAcc += __shfl(incl, 63);
        // repeat-mode FSE tables: the latest table of that kind defined in front of the block (:1780-1786)
        const bool seqs = live && nbSeq != 0;
        if (ballot(seqs && !ph)) hasSeq = 1;
        u32 src3[3];
#pragma unroll
        for (u32 t = 0; t < 3; ++t) {
            const u32 mode = (modes >> (6 - 2 * t)) & 3;
            const u64 def = ballot(seqs && mode != 3);
            u32& last = t == 0 ? lastTbl0 : t == 1 ? lastTbl1 : lastTbl2;
            src3[t] = bi;
            if (seqs && mode == 3) { src3[t] = latest_before(def, first + k0, last, lane); if (src3[t] == kNoBlock && !ph) err = err ? err : (u32)kErrCorruption; }
            if (def) last = first + k0 + (63u - (u32)__builtin_clzll(def));
        }
        if (ph && have) { BlockDesc& B = blocks[bi]; B.type = 1; B.outSize = 0; B.nbSeq = 0; if (seqPlane) seqPlane[bi] = 0; }
        else if (live) {
            BlockDesc& B = blocks[bi];
            if (litType >= 2) {
                B.hufSrc = hufSrc; B.litRel = litRel;
                // earlyLiterals: the literal decoder runs beside seq_decode, i.e. before block_offsets: only where the output offset is
                // known by now — the first block of a frame with a content size — can it write the output itself
                B.litInPlace = (nbSeq == 0 && !dumped && (!earlyLiterals || (k0 + lane == 0 && !F.unsized))) ? 1u : 0u;
            }
            if (seqs) { B.tblSrc[0] = src3[0]; B.tblSrc[1] = src3[1]; B.tblSrc[2] = src3[2]; }
            if (err) {
                B.err = err; report_error(status, bi, litType >= 2 && (err == kErrDictionaryCorrupted || litSize > dstSize) ? kStageLiterals : kStageSequences, err);
                if (seqPlane) seqPlane[bi] = 0;     // (block_parse_kernel)
            }
        }
    }
    if (lane == 0) {
        F.hasSeq = hasSeq;
        if constexpr (kOpen) { if (noRoom) F.unsized |= kFrameNoRoom; }
        if (litAcc) atomicAdd(reinterpret_cast<unsigned long long*>(status + kStLitLo), (unsigned long long)litAcc);
        // long frames by size class: what the host decides the origin path from (decode_origin.hip); a frame without a content size counts with its bound
        if (hasSeq && dstSize >= (1u << 20) && dstSize < (1ull << 30))
            atomicAdd(reinterpret_cast<unsigned long long*>(status + kStBigBins) + highbit32((u32)(dstSize >> 20)), (unsigned long long)dstSize);
    }
}
// (kStream: a fragment of a segmented stream, whose first `phantoms` blocks are carried definers — never a set, open or kDev instance)
template <bool kSet, bool kOpen, bool kDev, bool kStream>
__global__ __launch_bounds__(64) void block_link_kernel(FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks, u32 nFrames, u32 haveDict,
                                                        u32 earlyLiterals, u32* __restrict__ status, u32 phantoms, const DictSlot* __restrict__ slots,
                                                        u32* __restrict__ seqPlane)
{
    static_assert(!kStream || !(kSet || kOpen || kDev), "a stream fragment has one dictionary and a content size");
    block_link_body<kStream, kSet, kOpen>(frames, blocks, list_count<kDev>(nFrames, status, kStFrames), kSet ? 0 : haveDict, earlyLiterals, status,
                                          kStream ? phantoms : 0, kSet ? slots : nullptr, kDev ? nullptr : seqPlane);
}

// ------------------------------------------------------------------------------------------------
// seq_scan: where every block's sequence records go (exclusive scan of nbSeq), single workgroup
// ------------------------------------------------------------------------------------------------
// exclusive scan over n items of a single workgroup: fetch(i0, o) -> the values of the thread's kScanItems consecutive items from i0 on
// (0 for an item at or beyond n), store(i, sum of the items before it); -> the total, in every thread
template <class Fetch, class Store>
__device__ __forceinline__ u64 workgroup_scan_items(u32 n, u64 (*shW)[16], Fetch fetchItems, Store store)
{
    const u32 tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    u64 carry = 0;
    u64 v[kScanItems], nx[kScanItems];
    auto fetch = [&](u32 base, u64 (&o)[kScanItems]) { fetchItems(base + tid * kScanItems, o); };
    fetch(0, v);
    u32 par = 0;
    for (u32 base = 0; base < n; base += kScanRound, par ^= 1) {
        if (base + kScanRound < n) fetch(base + kScanRound, nx);
        u64 mine = 0;
#pragma unroll
        for (u32 j = 0; j < kScanItems; ++j) mine += v[j];
        u64 incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const u64 t = __shfl_up(incl, d); if ((int)lane >= d) incl += t; }
        if (lane == 63) shW[par][wave] = incl;
        lds_barrier();
        u64 before = carry, all = 0;
        for (u32 w = 0; w < 16; ++w) { if (w < wave) before += shW[par][w]; all += shW[par][w]; }
        u64 run = before + incl - mine;
#pragma unroll
        for (u32 j = 0; j < kScanItems; ++j) { const u32 i = base + tid * kScanItems + j; if (i < n) store(i, run); run += v[j]; }
        carry += all;
#pragma unroll
        for (u32 j = 0; j < kScanItems; ++j) v[j] = nx[j];
    }
    return carry;
}
// (the items one by one: load(i) -> the item's value)
template <class Load, class Store>
__device__ __forceinline__ u64 workgroup_scan(u32 n, u64 (*shW)[16], Load load, Store store)
{
    return workgroup_scan_items(n, shW, [&](u32 i0, u64 (&o)[kScanItems]) {
#pragma unroll
        for (u32 j = 0; j < kScanItems; ++j) o[j] = i0 + j < n ? load(i0 + j) : 0;
    }, store);
}

// kDev (ZSTDMI_decompressBatchAsync): the number of blocks comes from the status words, and so does the limit the caller set for the
// sequence records (kStCapSeq*: the record buffer was sized from it, once).  A block with sequences whose records would end beyond the
// limit fails with workSpace_tooSmall: its err keeps every later stage off it, and its key — block and stage fields zero, so that it
// outranks whatever else the entry's blocks report — folds into the entry's answer (batch_fold).  The sums run over such blocks too:
// every block with sequences behind one is refused as well.
// kDev = false reads no BlockDesc: an item is a word of seqPlane (block_parse_kernel), the dense image of what the kDev instance
// gathers at BlockDesc's stride, a cache line per item; a thread's four consecutive items are one 16-byte load (the plane is 16-byte
// aligned and kScanItems is 4).  pinned (null: none): the host's pinned copy of the status words (zmi_host.h) — this kernel is the last
// of the pre-pass to write them, so it hands all of them over and the host needs no copy behind it.
template <bool kDev = false>
__global__ __launch_bounds__(1024) void seq_scan_kernel(BlockDesc* __restrict__ blocks, u32 nBlocks, u32* __restrict__ status, const u32* __restrict__ seqPlane,
                                                        u32* __restrict__ pinned)
{
    __shared__ u64 shW[2][16];
    u64 total;
    if constexpr (kDev) {
        nBlocks = status[kStBlocks];
        const u64 capSeq = (u64)status[kStCapSeqLo] | ((u64)status[kStCapSeqHi] << 32);
        unsigned long long* const keys = reinterpret_cast<unsigned long long*>((uintptr_t)((u64)status[kStBlockKeysLo] | ((u64)status[kStBlockKeysHi] << 32)));
        total = workgroup_scan(nBlocks, shW,
            [&](u32 i) -> u64 { const BlockDesc& B = blocks[i]; return (B.type == 2 && !B.err) ? B.nbSeq : 0u; },
            [&](u32 i, u64 before) {
                BlockDesc& B = blocks[i];
                B.seqBase = before;
                if (B.type == 2 && !B.err && B.nbSeq && before + B.nbSeq > capSeq) { B.err = kErrWorkSpaceTooSmall; atomicMin(keys + i, (unsigned long long)kErrWorkSpaceTooSmall); }
            });
    } else {
        static_assert(kScanItems == 4, "a thread's items are one uint4");
        total = workgroup_scan_items(nBlocks, shW,
            [&](u32 i0, u64 (&o)[kScanItems]) {
                if (i0 + kScanItems <= nBlocks) { const uint4 q = *reinterpret_cast<const uint4*>(seqPlane + i0); o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w; }
                else {
#pragma unroll
                    for (u32 j = 0; j < kScanItems; ++j) o[j] = i0 + j < nBlocks ? seqPlane[i0 + j] : 0u;
                }
            },
            [&](u32 i, u64 before) { blocks[i].seqBase = before; });
    }
    if (threadIdx.x == 0) { status[kStSeqLo] = (u32)total; status[kStSeqHi] = (u32)(total >> 32); }
    if constexpr (!kDev) {
        // (the total is the same in every thread; the other words were written by kernels in front of this one)
        const u32 w = threadIdx.x;
        if (pinned && w < kStWords) pinned[w] = w == kStSeqLo ? (u32)total : w == kStSeqHi ? (u32)(total >> 32) : status[w];
    }
}

void launch_block_prepass(const u8* src, FrameDesc* frames, BlockDesc* blocks, u32 nFrames, u32 nBlocks, const DecodeDict& dd, u32 earlyLiterals, u32* status, hipStream_t stream,
                          u32* seqPlane, u32* pinned, u32 phantoms, bool open)
{
    // (a set instance reads whether its frame has a formatted dictionary from the frame's slot)
    const DictSlot* const slots = dd.slots; const u32 haveDict = !slots && dd.fmt ? 1u : 0u;
    hipLaunchKernelGGL(block_parse_kernel<>, dim3((nBlocks + 255) / 256), dim3(256), 0, stream, src, blocks, nBlocks, status, seqPlane);
    // a fragment of a segmented stream: one frame whose first blocks are carried definers (never a batch, and the host refuses it with a set)
    if (phantoms && !open && !slots) hipLaunchKernelGGL((block_link_kernel<false, false, false, true>), dim3(nFrames), dim3(64), 0, stream, frames, blocks, nFrames, haveDict, earlyLiterals, status, phantoms, slots, seqPlane);
    else with_flags([&](auto set, auto op) {
        hipLaunchKernelGGL((block_link_small_kernel<set(), op()>), dim3((nFrames + 63) / 64), dim3(64), 0, stream, frames, blocks, nFrames, haveDict, earlyLiterals, status, slots, seqPlane);
        if (nBlocks > nFrames)          // (some frame has several blocks)
            hipLaunchKernelGGL((block_link_kernel<set(), op(), false, false>), dim3(nFrames), dim3(64), 0, stream, frames, blocks, nFrames, haveDict, earlyLiterals, status, 0u, slots, seqPlane);
    }, slots != nullptr, open);
    hipLaunchKernelGGL(seq_scan_kernel<>, dim3(1), dim3(1024), 0, stream, blocks, nBlocks, status, (const u32*)seqPlane, pinned);
}

// the pre-pass of a batch enqueued from the device: the open instances, the counts from the status words, grids over the caller's limits
// (block_link_open always runs: whether some frame has more than kLinkSmall blocks is not known here)
void launch_block_prepass_d(const u8* src, FrameDesc* frames, BlockDesc* blocks, u32 capFrames, u32 capBlocks, const DecodeDict& dd, u32* status, hipStream_t stream)
{
    const DictSlot* const slots = dd.slots; const u32 haveDict = !slots && dd.fmt ? 1u : 0u;        // (as launch_block_prepass)
    hipLaunchKernelGGL(block_parse_kernel<true>, dim3((capBlocks + 255) / 256), dim3(256), 0, stream, src, blocks, 0u, status, (u32*)nullptr);
    with_flags([&](auto set) {
        hipLaunchKernelGGL((block_link_small_kernel<set(), true, true>), dim3((capFrames + 63) / 64), dim3(64), 0, stream, frames, blocks, 0u, haveDict, 0u, status, slots, (u32*)nullptr);
        hipLaunchKernelGGL((block_link_kernel<set(), true, true, false>), dim3(capFrames), dim3(64), 0, stream, frames, blocks, 0u, haveDict, 0u, status, 0u, slots, (u32*)nullptr);
    }, slots != nullptr);
    hipLaunchKernelGGL(seq_scan_kernel<true>, dim3(1), dim3(1024), 0, stream, blocks, 0u, status, (const u32*)nullptr, (u32*)nullptr);
}

// ------------------------------------------------------------------------------------------------
// block_offsets: output offsets and starting repcodes of the blocks of a frame (one wave per frame, after seq_decode)
// ------------------------------------------------------------------------------------------------
// kSet: the repcodes a frame starts from are its own dictionary's (one frame per wave: the record's fields are wave-uniform)
// kOpen (a batch with entries that hold unsized frames): FrameDesc::unsized carries flags beside "no content size" (kFrameOpen)
// sizePlane (null: none; a call that runs frame_rescan_kernel behind this one): one u64 per frame, its dstSize as this kernel leaves it
template <bool kSet, bool kOpen = false>
__device__ __forceinline__ void block_offsets_body(FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks, u32 nFrames,
                                                   const DictInfo* __restrict__ di, u32* __restrict__ status, const DictSlot* __restrict__ slots,
                                                   u64* __restrict__ sizePlane)
{
    const u32 f = blockIdx.x, lane = threadIdx.x;
    if (f >= nFrames) return;
    const u32 first = frames[f].firstBlock, nb = frames[f].nbBlocks;
    u32 r0 = 1, r1 = 4, r2 = 8;                                // ZSTD_decompressBegin, U/ZstdDecompress.cs:1933-1954
    if constexpr (kSet) {
        const DictSlot& D = slots[uniform(frames[f].dictSlot)];
        if (uniform(D.formatted)) { r0 = uniform(D.rep[0]); r1 = uniform(D.rep[1]); r2 = uniform(D.rep[2]); }
    } else
    if (di) { r0 = uniform(di->rep[0]); r1 = uniform(di->rep[1]); r2 = uniform(di->rep[2]); }
    u64 acc = 0; u32 bad = 0;
    for (u32 k0 = 0; k0 < nb; k0 += 64) {
        const u32 k = k0 + lane; const bool have = k < nb;
        const u32 bi = first + (have ? k : 0);
        u32 outSize = 0, err = 0, kinds = 0, v0 = 0, v1 = 0, v2 = 0; bool hasRep = false;
        if (have) {
            const BlockDesc& B = blocks[bi];
            outSize = B.outSize; err = B.err;
            hasRep = B.type == 2 && B.nbSeq != 0 && !B.err;
            if (hasRep) { kinds = B.repKind[0] | (B.repKind[1] << 2) | (B.repKind[2] << 4); v0 = B.repVal[0]; v1 = B.repVal[1]; v2 = B.repVal[2]; }
        }
        if (ballot(err != 0)) bad = 1;
        // output offsets: exclusive prefix sum of the regenerated sizes
        u64 incl = outSize;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const u64 t = __shfl_up(incl, d); if ((int)lane >= d) incl += t; }
        if (have) blocks[bi].dstRel = acc + incl - outSize;
        acc += __shfl(incl, 63);
        // repcodes: the blocks' transfer functions applied in order (wave-uniform; blocks without sequences pass them through)
        u32 in0 = r0, in1 = r1, in2 = r2;                      // what this lane's block starts from
        u64 m = ballot(have);
        while (m) {
            const u32 l = ctz64(m); m &= m - 1;
            if (lane == l) { in0 = r0; in1 = r1; in2 = r2; }
            if (read_lane((u32)hasRep, l)) {
                const u32 kk = read_lane(kinds, l), a0 = read_lane(v0, l), a1 = read_lane(v1, l), a2 = read_lane(v2, l);
                auto apply = [&](u32 kind, u32 val) -> u32 {
                    if (kind == 0) return val;
                    const u32 in = kind == 1 ? r0 : kind == 2 ? r1 : r2;
                    return in > val ? in - val : 1u;
                };
                const u32 n0 = apply(kk & 3, a0), n1 = apply((kk >> 2) & 3, a1), n2 = apply((kk >> 4) & 3, a2);
                r0 = n0; r1 = n1; r2 = n2;
            }
        }
        if (have) { BlockDesc& B = blocks[bi]; B.repIn[0] = in0; B.repIn[1] = in1; B.repIn[2] = in2; }
    }
    if (lane == 0) {
        FrameDesc& F = frames[f];
        const u32 unsized = kOpen ? F.unsized & kFrameUnsized : F.unsized;
        if (bad) F.bad = 1;
        else if (!unsized && acc != F.dstSize) {              // regenerated size must equal the header's (U/ZstdDecompress.cs:1177-1184)
            F.bad = 1; report_error(status, (u64)first + nb - 1, kStageFrameEnd, kErrCorruption);
        } else if (unsized) {
            if (acc > F.dstSize) { F.bad = 1; report_error(status, (u64)first + nb - 1, kStageFrameEnd, kErrCorruption); }   // more than nbBlocks x blockSizeMax: no valid encoder
            else F.dstSize = acc;
        }
        if (sizePlane) sizePlane[f] = F.dstSize;
    }
}
template <bool kSet, bool kOpen, bool kDev>
__global__ __launch_bounds__(64) void block_offsets_kernel(FrameDesc* __restrict__ frames, BlockDesc* __restrict__ blocks, u32 nFrames,
                                                           const DictInfo* __restrict__ di, u32* __restrict__ status, const DictSlot* __restrict__ slots,
                                                           u64* __restrict__ sizePlane)
{
    static_assert(kOpen || !kDev, "a batch enqueued from the device runs the open instances");
    block_offsets_body<kSet, kOpen>(frames, blocks, list_count<kDev>(nFrames, status, kStFrames), kSet ? nullptr : di, status, kSet ? slots : nullptr,
                                    kOpen ? nullptr : sizePlane);
}

// frames without a content size: the frames' output offsets from their regenerated sizes (single workgroup); the total goes to
// status, and a total beyond the destination's capacity stops everything behind this kernel.  The sizes are read from sizePlane
// (block_offsets_body), dense, a thread's four as two 16-byte loads, not at FrameDesc's stride.
__global__ __launch_bounds__(1024) void frame_rescan_kernel(FrameDesc* __restrict__ frames, u32 nFrames, u64 dstCapacity, u32* __restrict__ status,
                                                            const u64* __restrict__ sizePlane)
{
    __shared__ u64 shW[2][16];
    static_assert(kScanItems == 4, "a thread's items are two ulonglong2");
    const u64 total = workgroup_scan_items(nFrames, shW,
        [&](u32 i0, u64 (&o)[kScanItems]) {
            if (i0 + kScanItems <= nFrames) {
                const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(sizePlane + i0), b = *reinterpret_cast<const ulonglong2*>(sizePlane + i0 + 2);
                o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
            } else {
#pragma unroll
                for (u32 j = 0; j < kScanItems; ++j) o[j] = i0 + j < nFrames ? sizePlane[i0 + j] : 0u;
            }
        },
        [&](u32 i, u64 before) { frames[i].dstOff = before; });
    if (threadIdx.x == 0) {
        status[kStActualLo] = (u32)total; status[kStActualHi] = (u32)(total >> 32);
        if (total > dstCapacity) status[kStErr] = kErrDstSizeTooSmall;
    }
}

void launch_block_offsets(FrameDesc* frames, BlockDesc* blocks, u32 nFrames, const DecodeDict& dd, const DictInfo* reps, u64* sizePlane, u64 dstCapacity, u32* status, hipStream_t stream,
                          bool open)
{
    // (a set instance starts from its frame's slot)
    with_flags([&](auto set, auto op) {
        hipLaunchKernelGGL((block_offsets_kernel<set(), op(), false>), dim3(nFrames), dim3(64), 0, stream, frames, blocks, nFrames, reps, status, dd.slots, sizePlane);
    }, dd.slots != nullptr, open);
    if (sizePlane) hipLaunchKernelGGL(frame_rescan_kernel, dim3(1), dim3(1024), 0, stream, frames, nFrames, dstCapacity, status, (const u64*)sizePlane);
}

void launch_block_offsets_d(FrameDesc* frames, BlockDesc* blocks, u32 capFrames, const DecodeDict& dd, u32* status, hipStream_t stream)
{
    with_flags([&](auto set) {
        hipLaunchKernelGGL((block_offsets_kernel<set(), true, true>), dim3(capFrames), dim3(64), 0, stream, frames, blocks, 0u, dd.dinfo, status, dd.slots, (u64*)nullptr);
    }, dd.slots != nullptr);
}

// ZSTD_loadDEntropy's checks (U/ZstdDecompress.cs:1773-1875) on one lane: where the Huffman description and the three NCounts
// sit, the repcodes, where the content starts; err = dictionary_corrupted if anything is off.
struct DictScratch { u8 weights[256]; s16 norm[256]; u16 symbolNext[256]; u16 wNewState[64]; u8 wSymbol[64]; u8 wNbBits[64]; };
__global__ __launch_bounds__(64) void dict_parse_kernel(const u8* __restrict__ dict, u32 dictSize, DictInfo* __restrict__ out)
{
    __shared__ DictScratch L;
    __shared__ s16 norm[64];
    const u32 lane = threadIdx.x;
    if (lane != 0) return;
    DictInfo d = {}; d.err = kErrDictionaryCorrupted;
    do {
        if (dictSize <= 8) break;
        d.dictID = readLE32(dict + 4);
        u32 nbSymbols = 0, tableLog = 0;
        const u32 hs = huf_read_stats(L, dict + 8, dictSize - 8, &nbSymbols, &tableLog);
        if (!hs || tableLog > 12) break;
        d.hufOff = 8; d.hufSize = hs;
        u32 p = 8 + hs, maxSV, log, h;
        maxSV = 31; h = read_ncount(norm, &maxSV, &log, dict + p, dictSize - p);
        if (!h || maxSV > 31 || log > 8) break;
        d.ofOff = p; p += h;
        maxSV = 52; h = read_ncount(norm, &maxSV, &log, dict + p, dictSize - p);
        if (!h || maxSV > 52 || log > 9) break;
        d.mlOff = p; p += h;
        maxSV = 35; h = read_ncount(norm, &maxSV, &log, dict + p, dictSize - p);
        if (!h || maxSV > 35 || log > 9) break;
        d.llOff = p; p += h;
        if (p + 12 > dictSize) break;
        d.repOff = p;
        d.contentOff = p + 12; d.contentSize = dictSize - d.contentOff;
        bool ok = true;
        for (u32 i = 0; i < 3; i++) { d.rep[i] = readLE32(dict + p + 4 * i); if (d.rep[i] == 0 || d.rep[i] > d.contentSize) ok = false; }
        if (!ok) break;
        d.err = 0;
    } while (false);
    *out = d;
}
void launch_dict_parse(const u8* dict, u32 dictSize, DictInfo* out, hipStream_t stream)
{
    hipLaunchKernelGGL(dict_parse_kernel, dim3(1), dim3(64), 0, stream, dict, dictSize, out);
}

// The same header as the COMPRESSOR uses it (ZSTD_loadCEntropy, U/ZstdCompress.cs:5259-5400), one wave, once per dictionary load:
// the Huffman description becomes a code table (HUF_readCTable, U/HufCompress.cs:237-290: weights -> lengths -> canonical codes in
// symbol order), the three NCounts become compression tables (FSE_buildCTable_wksp by the wave, straight into the record), and the
// four repeat states say what a block may rely on: the Huffman table is `valid` without a zero weight and otherwise needs a look at
// the block's literals; an FSE table is `valid` when every symbol up to the alphabet's maximum has a probability
// (ZSTD_dictNCountRepeat, :5239-5257; for offsets the maximum follows from the content size).  The weights and NCount readers are
// the decoder's.  `info` is what dict_parse_kernel left: the offsets are inside the dictionary.
struct DictCtabScratch { DictScratch hs; s16 norm[3][64]; u32 dictMax[3], log[3], nbSymbols, hufLog, ok, valPerRank[14]; u16 cum[64]; u8 tableSymbol[512]; };
__global__ __launch_bounds__(64) void dict_ctables_kernel(const u8* __restrict__ dict, u32 dictSize, const DictInfo* __restrict__ info,
                                                          DictCTables* __restrict__ out)
{
    __shared__ DictCtabScratch S;
    const u32 lane = threadIdx.x;
    const DictInfo d = *info;
    const bool sane = !d.err && d.hufOff < d.ofOff && d.ofOff < d.mlOff && d.mlOff < d.llOff && d.llOff < d.repOff && d.repOff <= dictSize;
    for (u32 t = 0; t < 3; ++t) S.norm[t][lane] = 0;
    if (lane == 0) { S.ok = 0; S.nbSymbols = 0; S.hufLog = 0; for (u32 t = 0; t < 3; ++t) { S.dictMax[t] = 0; S.log[t] = 5; } }
    wave_lds_sync();
    if (lane == 0 && sane) {
        u32 nbSymbols = 0, hufLog = 0;
        const u32 hs = huf_read_stats(S.hs, dict + d.hufOff, d.ofOff - d.hufOff, &nbSymbols, &hufLog);
        // order of the record: LL, OF, ML
        u32 mOF = 31, mML = 52, mLL = 35, lOF = 0, lML = 0, lLL = 0;
        const u32 hOF = read_ncount(S.norm[1], &mOF, &lOF, dict + d.ofOff, d.mlOff - d.ofOff);
        const u32 hML = read_ncount(S.norm[2], &mML, &lML, dict + d.mlOff, d.llOff - d.mlOff);
        const u32 hLL = read_ncount(S.norm[0], &mLL, &lLL, dict + d.llOff, d.repOff - d.llOff);
        if (hs && hufLog <= 12 && nbSymbols <= 256 && hOF && hML && hLL && mOF <= 31 && mML <= 52 && mLL <= 35 && lOF <= 8 && lML <= 9 && lLL <= 9) {
            S.ok = 1; S.nbSymbols = nbSymbols; S.hufLog = hufLog;
            S.dictMax[0] = mLL; S.dictMax[1] = mOF; S.dictMax[2] = mML; S.log[0] = lLL; S.log[1] = lOF; S.log[2] = lML;
        }
    }
    wave_lds_sync();
    const u32 ok = S.ok, nbSym = S.nbSymbols, hl = S.hufLog;
    if (!ok) for (u32 t = 0; t < 3; ++t) S.norm[t][lane] = lane == 0 ? (s16)32 : (s16)0;      // (a table of one symbol: never used, never out of range)
    wave_lds_sync();
    {   // HUF_readCTable
        u32 nb[4], pre[4]; bool zero = false;
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            const u32 sIdx = k * 64 + lane;
            const u32 w = (ok && sIdx < nbSym) ? S.hs.weights[sIdx] : 0u;
            nb[k] = w ? hl + 1 - w : 0u; pre[k] = 0;
            zero |= ballot(sIdx < nbSym && w == 0) != 0;
        }
        u32 mn = 0;
        for (u32 r = 12; r >= 1; r--) {
            const u32 n = popc64(ballot(nb[0] == r)) + popc64(ballot(nb[1] == r)) + popc64(ballot(nb[2] == r)) + popc64(ballot(nb[3] == r));
            if (lane == 0) S.valPerRank[r] = mn;
            mn = (mn + n) >> 1;
            u32 acc = 0;
#pragma unroll
            for (u32 k = 0; k < 4; ++k) {
                const u64 b = ballot(nb[k] == r);
                if (nb[k] == r) pre[k] = acc + popc64(b & lanemask_lt());
                acc += popc64(b);
            }
        }
        if (lane == 0) S.valPerRank[0] = 0;
        wave_lds_sync();
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            const u32 sIdx = k * 64 + lane;
            out->hufNbBits[sIdx] = (u8)nb[k];
            out->hufCode[sIdx] = (u16)(nb[k] ? S.valPerRank[nb[k]] + pre[k] : 0u);
        }
        // (the encoder's tiles are sized for codes of at most 11 bits, the longest its own trees have: a longer table is not used)
        if (lane == 0) out->hufMode = (ok && nbSym == 256 && hl <= 11) ? (zero ? kDictHufCheck : kDictHufValid) : kDictHufNone;
    }
    const u32 content = d.contentSize < (1u << 30) ? d.contentSize : (1u << 30);
    u32 ofMax = highbit32(content + (128u << 10)); if (ofMax > 31) ofMax = 31;
    for (u32 t = 0; t < 3; ++t) {
        const u32 full = t == 0 ? 35u : t == 1 ? 31u : 52u, need = t == 1 ? ofMax : full;
        u16* const st = t == 0 ? out->llState : t == 1 ? out->ofState : out->mlState;
        SymTT* const tt = t == 0 ? out->llTT : t == 1 ? out->ofTT : out->mlTT;
        const u32 log = ok ? S.log[t] : 5u;
        const u64 present = ballot(lane <= S.dictMax[t] && S.norm[t][lane] != 0);
        const u64 needMask = (2ull << need) - 1ull;
        fse_build_ctable_wave(st, tt, S.norm[t], full, log, S.cum, S.tableSymbol, lane);
        if (lane == 0) {
            out->seqValid[t] = (ok && S.dictMax[t] >= need && (present & needMask) == needMask) ? 1u : 0u;
            out->seqLog[t] = log; out->seqPresent[t] = ok ? present : 0ull;
            if (t == 0) out->pad = 0;
        }
    }
}
void launch_dict_ctables(const u8* dict, u32 dictSize, const DictInfo* info, DictCTables* out, hipStream_t stream)
{
    hipLaunchKernelGGL(dict_ctables_kernel, dim3(1), dim3(64), 0, stream, dict, dictSize, info, out);
}

} // namespace zmi
