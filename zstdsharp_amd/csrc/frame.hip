// frame.hip — output assembly on gfx950: per-chunk frame sizes -> exclusive scan -> gather into one contiguous
// stream (the "variable-length output" step of SURVEY.md §7), plus the optional XXH64 content checksum
// (U/Xxhash.cs:378-600, written by ZSTD_writeEpilogue U/ZstdCompress.cs:5641-5652).
#include "zmi_device.h"
#include "zmi_host.h"

namespace zmi {

// ---- exclusive scan of ChunkMeta::outSize (one workgroup; nChunks is at most a few hundred thousand) ----
// pinned (null: none): the context's pinned block (PinBuf, zmi_host.h), where the host reads what it wants of the pass behind its wait:
// word 0 the total, word 1 + i the offset of chunk marks.chunk[i]
__global__ __launch_bounds__(1024) void scan_sizes_kernel(const ChunkMeta* __restrict__ meta, u32 nChunks,
                                                          u64* __restrict__ offsets, u64* __restrict__ total, u64* __restrict__ pinned, PassMarks marks)
{
    __shared__ u32 waveSum[16];
    const u32 tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    u64 carry = 0;
    for (u32 base = 0; base < nChunks; base += 1024) {
        const u32 i = base + tid;
        const u32 v = i < nChunks ? meta[i].outSize : 0;
        const u32 incl = wave_scan_incl(v);
        if (lane == 63) waveSum[wave] = incl;
        __syncthreads();
        u32 before = 0, all = 0;
#pragma unroll
        for (u32 k = 0; k < 16; k++) { const u32 s = waveSum[k]; all += s; if (k < wave) before += s; }
        if (i < nChunks) offsets[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
    if (pinned) {       // (the last round's barrier stands between the offsets' stores and these loads)
        if (tid == 0) pinned[0] = carry;
        if (tid < marks.n && marks.chunk[tid] < nChunks) pinned[1 + tid] = offsets[marks.chunk[tid]];
    }
}

// ---- gather: copy each chunk's frame from its slot (or, for stored blocks, header + source bytes) to dst ----
__device__ __forceinline__ void copy_bytes(u8* __restrict__ d, const u8* __restrict__ s, u32 n, u32 tid, u32 nthreads)
{
    // head: bring d to 16-byte alignment, then 16 B stores fed by unaligned loads
    u32 head = (u32)((16 - ((uintptr_t)d & 15)) & 15);
    if (head > n) head = n;
    if (tid < head) d[tid] = s[tid];
    const u32 body = (n - head) >> 4;
    uint4* d4 = reinterpret_cast<uint4*>(d + head);
    const u8* sb = s + head;
    for (u32 i = tid; i < body; i += nthreads) {
        uint4 v;
        v.x = readLE32(sb + 16 * i); v.y = readLE32(sb + 16 * i + 4); v.z = readLE32(sb + 16 * i + 8); v.w = readLE32(sb + 16 * i + 12);
        d4[i] = v;
    }
    const u32 done = head + (body << 4);
    if (tid < n - done) d[done + tid] = s[done + tid];
}

__global__ __launch_bounds__(256) void gather_kernel(const u8* __restrict__ src, u64 srcSize, const u8* __restrict__ slots,
                                                     const ChunkMeta* __restrict__ meta, const u64* __restrict__ offsets,
                                                     u8* __restrict__ dst, u64 dstCapacity, u32 chunkBytes)
{
    const u32 c = blockIdx.x, tid = threadIdx.x;
    const ChunkMeta m = meta_checked(meta[c]);
    const u64 off = offsets[c];
    if (off + m.outSize > dstCapacity) return;           // host reports dstSize_tooSmall from the scanned total
    const u8* slot = slots + (u64)c * kSlotStride;
    u8* d = dst + off;
    const u32 tail = m.outSize - (m.fhSize + 3) - (m.blockType == 2 ? m.bodySize : m.srcSize);   // 0 or 4 (checksum)
    if (m.blockType == 2) {
        // the literals section is already in place (huf_encode writes it there); headers and the sequences section follow
        const u32 head = m.fhSize + 3, seqAt = head + m.litSectionSize;
        if (tid < head) d[tid] = slot[tid];
        copy_bytes(d + seqAt, slot + seqAt, head + m.bodySize - seqAt, tid, 256);
    } else {
        if (tid < m.fhSize + 3) d[tid] = slot[tid];
        copy_bytes(d + m.fhSize + 3, src + (u64)c * chunkBytes, m.srcSize, tid, 256);
    }
    if (tail && tid < 4) d[m.outSize - 4 + tid] = (u8)(m.checksum >> (8 * tid));
}

// ---- a batch of independent inputs (ZSTDMI_compressBatch; the trainer's samples): staging and placement ----
// stage: chunk c = bytes [from[c], from[c] + len[c]) — any address in HBM, any alignment — to its own chunk boundary c * chunkBytes
__global__ __launch_bounds__(256) void batch_stage_kernel(const u64* __restrict__ from, const u32* __restrict__ len, u8* __restrict__ stage, u32 chunkBytes)
{
    const u32 c = blockIdx.x;
    copy_bytes(stage + (u64)c * chunkBytes, reinterpret_cast<const u8*>((uintptr_t)from[c]), len[c], threadIdx.x, 256);
}

// place (instead of scan_sizes): entry e owns the chunks [entFirst[e], entFirst[e + 1]); its frames lie one behind the other from
// entDst[e], an offset from the one base pointer huf_encode and gather are given.  An entry whose frames exceed entCap[e] gets
// dstSize_tooSmall and its chunks the offset `span` (the end of everything the base pointer may reach), which fails both kernels'
// capacity comparison: nothing of it is written.  One lane per entry.
__global__ __launch_bounds__(256) void batch_place_kernel(const ChunkMeta* __restrict__ meta, u32 nEntries, const u32* __restrict__ entFirst,
                                                          const u64* __restrict__ entDst, const u64* __restrict__ entCap, u64 span,
                                                          u64* __restrict__ offsets, u64* __restrict__ entSize)
{
    const u32 e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nEntries) return;
    const u32 c0 = entFirst[e], c1 = entFirst[e + 1];
    u64 sum = 0;
    for (u32 c = c0; c < c1; ++c) sum += meta[c].outSize;
    const bool fits = sum <= entCap[e];
    u64 at = entDst[e];
    for (u32 c = c0; c < c1; ++c) { offsets[c] = fits ? at : span; at += meta[c].outSize; }
    entSize[e] = fits ? sum : (u64)0 - (u64)kErrDstSizeTooSmall;
}

// ---- a batch whose descriptors lie in HBM (ZSTDMI_compressBatchAsync): the plan and the placement, no host in between ----
// plan: entry e is chunk e.  The caller's arrays are read here, once, and checked as compress_entries checks them on the host; what the
// stages read comes out in their layout: from[e], len[e], entFirst[e] = e (and entFirst[n] = n), entDst[e] = the destination's offset
// from kAsyncBase, entCap[e].  verdict[e]: kAsyncGood, kAsyncEmpty (size 0: the placement writes the empty frame), or the error code
// the entry answers.  The stages have never seen an empty or an oversize chunk, so every entry that is not kAsyncGood becomes the one
// byte at `dummy` (context memory); the placement overrides whatever that chunk compressed to.  One lane per entry.
__global__ __launch_bounds__(256) void batch_plan_kernel(const void* const* __restrict__ srcs, const size_t* __restrict__ sizes,
                                                         void* const* __restrict__ dsts, const size_t* __restrict__ caps, u32 n, u64 bound,
                                                         u32 emptyLen, const u8* __restrict__ dummy, u64* __restrict__ from,
                                                         u64* __restrict__ entDst, u64* __restrict__ entCap, u32* __restrict__ len,
                                                         u32* __restrict__ entFirst, u32* __restrict__ verdict)
{
    const u32 e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const u64 S = (u64)sizes[e], cap = (u64)caps[e];
    const u64 src = (u64)(uintptr_t)srcs[e], dst = (u64)(uintptr_t)dsts[e];
    const u32 v = plan_verdict(src, S, dst, cap, bound, emptyLen);          // (zmi_batch_plan.h)
    const bool good = v == kAsyncGood;
    from[e] = good ? src : (u64)(uintptr_t)dummy;
    len[e] = good ? (u32)S : 1u;
    entDst[e] = dst >= kAsyncBase ? dst - kAsyncBase : 0;
    entCap[e] = cap;
    entFirst[e] = e;
    if (e == n - 1) entFirst[n] = n;
    verdict[e] = v;
}

// place (batch_place_kernel's part for such a batch): entry e = chunk e; its size or its error code goes straight into the caller's
// column.  A good entry that fits lies at entDst[e]; everything else gets the offset kAsyncSpan, which fails huf_encode's and gather's
// capacity comparison (off + outSize > kAsyncSpan), so nothing of it is written.  An empty entry's frame — the bytes the single call
// writes under the call's parameters, a launch constant — is written here (the plan compared it with the capacity).  One lane per entry.
__global__ __launch_bounds__(256) void batch_place_async_kernel(const ChunkMeta* __restrict__ meta, u32 n, const u64* __restrict__ entDst,
                                                                const u64* __restrict__ entCap, const u32* __restrict__ verdict,
                                                                const AsyncEmptyFrame empty, u64* __restrict__ offsets, size_t* __restrict__ dstSizes)
{
    const u32 e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const u32 v = verdict[e];
    const u64 out = meta[e].outSize;
    u64 at = kAsyncSpan, answer;
    if (v == kAsyncGood) {
        const bool fits = out <= entCap[e];
        if (fits) at = entDst[e];
        answer = fits ? out : (u64)0 - (u64)kErrDstSizeTooSmall;
    } else if (v == kAsyncEmpty) {
        u8* const d = reinterpret_cast<u8*>((uintptr_t)(entDst[e] + kAsyncBase));
        for (u32 i = 0; i < empty.len; ++i) d[i] = empty.bytes[i];
        answer = empty.len;
    } else answer = (u64)0 - (u64)v;
    offsets[e] = at;
    dstSizes[e] = (size_t)answer;
}

// ---- the same batch with entries of several chunks (ZSTDMI_CCtx_prepareBatchAsyncLimits): the host knows the number of entries and a
// chunk limit, never a size; the arithmetic is zmi_batch_plan.h's, which tests/host/batch_plan_harness.cpp holds against the host loop ----
// plan, entries -> chunk ranges.  ONE workgroup of 1024 lanes, 16 consecutive entries per lane (n <= 16384, the pass limit): a lane's
// verdicts and chunk counts stay in registers; the lanes' sums are scanned by wave (cross-lane shifts), the wave totals go through LDS.
// The lane that holds the first refused entry (plan_refused) publishes its exclusive sum, the cut: every entFirst is held to it, so
// refused, failed and empty entries own no chunk.  The caller's arrays are read here, once; the other two kernels read the copies.
// kPack (ZSTDMI_compressPackAsync): the entries share one destination, so dsts and caps are not read (null), the dst and cap columns
// are not written, and the verdict is pack_verdict's.
constexpr u32 kPlanPerLane = 16;
template <bool kPack>
__global__ __launch_bounds__(1024) void batch_plan_entries_kernel(const void* const* __restrict__ srcs, const size_t* __restrict__ sizes,
                                                                  void* const* __restrict__ dsts, const size_t* __restrict__ caps, u32 n, u64 bound,
                                                                  u32 emptyLen, u32 chunkBytes, u32 maxChunks, const AsyncEntryTab tab)
{
    __shared__ u32 waveSum[16];
    __shared__ u32 cutAt;
    const u32 tid = threadIdx.x, lane = lane_id(), wave = wave_id(), e0 = tid * kPlanPerLane;
    if (tid == 0) cutAt = kPlanNoCut;
    u32 cnt[kPlanPerLane], verdict[kPlanPerLane], mine = 0;
#pragma unroll
    for (u32 k = 0; k < kPlanPerLane; ++k) {
        const u32 e = e0 + k;
        cnt[k] = 0; verdict[k] = kAsyncEmpty;
        if (e < n) {
            const u64 S = (u64)sizes[e], src = (u64)(uintptr_t)srcs[e];
            tab.src[e] = src; tab.size[e] = S;
            if constexpr (kPack) verdict[k] = pack_verdict(src, S, bound);
            else {
                const u64 cap = (u64)caps[e], dst = (u64)(uintptr_t)dsts[e];
                verdict[k] = plan_verdict(src, S, dst, cap, bound, emptyLen);
                tab.cap[e] = cap;
                tab.dst[e] = dst >= kAsyncBase ? dst - kAsyncBase : 0;
            }
            cnt[k] = plan_chunks(verdict[k], S, chunkBytes);
        }
        mine += cnt[k];
    }
    const u32 incl = wave_scan_incl(mine);
    if (lane == 63) waveSum[wave] = incl;
    __syncthreads();
    u32 before = 0, all = 0;
#pragma unroll
    for (u32 k = 0; k < 16; k++) { const u32 s = waveSum[k]; all += s; if (k < wave) before += s; }
    const u32 first = before + incl - mine;             // the exclusive sum in front of this lane's entries
    u32 run = first;
#pragma unroll
    for (u32 k = 0; k < kPlanPerLane; ++k) {
        if (plan_is_cut(run, cnt[k], maxChunks)) cutAt = run;     // (one entry at most)
        run += cnt[k];
    }
    __syncthreads();
    const u32 cut = cutAt;
    run = first;
#pragma unroll
    for (u32 k = 0; k < kPlanPerLane; ++k) {
        const u32 e = e0 + k;
        if (e < n) {
            tab.first[e] = plan_first(run, cut);
            tab.verdict[e] = plan_limited(verdict[k], run, cnt[k], maxChunks);
        }
        run += cnt[k];
    }
    if (tid == 0) tab.first[n] = plan_first(all, cut);
}

// plan, chunks: one lane per chunk slot of the grid.  A slot below the call's total finds its entry by a binary search in entFirst and
// writes what the stages read for that chunk; a slot at or beyond it becomes what an ineligible entry is in batch_plan_kernel: one byte
// read from `dummy`, a frame of its own (the placement gives it the offset kAsyncSpan).  frame: null where every chunk is a frame.
__global__ __launch_bounds__(256) void batch_plan_chunks_kernel(const AsyncEntryTab tab, u32 n, u32 nLaunch, u32 chunkBytes, u32 frameBlocks,
                                                                const u8* __restrict__ dummy, u64* __restrict__ from, u32* __restrict__ len,
                                                                u32* __restrict__ frame)
{
    const u32 c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nLaunch) return;
    PlanChunk r = plan_chunk_idle((u64)(uintptr_t)dummy);
    if (c < tab.first[n]) {
        const u32 e = plan_owner(tab.first, n, c);
        r = plan_chunk(tab.src[e], tab.size[e], c - tab.first[e], chunkBytes, frameBlocks);
    }
    from[c] = r.from;
    len[c] = r.len;
    if (frame) frame[c] = r.frameWord;
}

// place (batch_place_async_kernel for entries of several chunks): entry e's frames lie one behind the other from its destination; their
// sum is compared with the capacity, and the size or the error goes straight into the caller's column.  Every chunk of an entry that
// writes nothing, and every idle slot, gets the offset kAsyncSpan.  One lane per entry; the idle slots are dealt to the grid's lanes.
__global__ __launch_bounds__(256) void batch_place_async_frames_kernel(const ChunkMeta* __restrict__ meta, u32 n, u32 nLaunch, const AsyncEntryTab tab,
                                                                       const AsyncEmptyFrame empty, u64* __restrict__ offsets, size_t* __restrict__ dstSizes)
{
    const u32 e = blockIdx.x * 256 + threadIdx.x;
    for (u32 c = tab.first[n] + e; c < nLaunch; c += gridDim.x * 256) offsets[c] = kAsyncSpan;
    if (e >= n) return;
    const u32 v = tab.verdict[e];
    u64 answer;
    if (v == kAsyncGood) {
        const u32 c0 = tab.first[e], c1 = tab.first[e + 1];
        u64 sum = 0;
        for (u32 c = c0; c < c1; ++c) sum += meta[c].outSize;
        const bool fits = sum <= tab.cap[e];
        u64 at = tab.dst[e];
        for (u32 c = c0; c < c1; ++c) { offsets[c] = fits ? at : kAsyncSpan; at += meta[c].outSize; }
        answer = fits ? sum : (u64)0 - (u64)kErrDstSizeTooSmall;
    } else if (v == kAsyncEmpty) {
        u8* const d = reinterpret_cast<u8*>((uintptr_t)(tab.dst[e] + kAsyncBase));
        for (u32 i = 0; i < empty.len; ++i) d[i] = empty.bytes[i];
        answer = empty.len;
    } else answer = (u64)0 - (u64)v;
    dstSizes[e] = (size_t)answer;
}

// ---- seek table (ZSTDMI_CCtx_setSeekTable; the zstd seekable format) ----
// entries: one (compressed size, content size) pair per frame of the pass, from the scan's offsets.  A frame is frameBlocks chunks
// (the pass's last one may be shorter); the sizes are below 2^32 by construction (a frame holds at most 512 MiB of content).
__global__ __launch_bounds__(256) void seek_entries_kernel(const u64* __restrict__ offsets, const u64* __restrict__ total, u32 nChunks, const FrameLayout frames,
                                                           u32* __restrict__ entries)
{
    const u32 f = blockIdx.x * 256 + threadIdx.x;
    const u32 nFrames = (nChunks + frames.frameBlocks - 1) / frames.frameBlocks;
    if (f >= nFrames) return;
    const u64 first = (u64)f * frames.frameBlocks, next = first + frames.frameBlocks;
    const u64 cEnd = next < nChunks ? offsets[next] : *total;
    entries[2 * (u64)f] = (u32)(cEnd - offsets[first]);
    entries[2 * (u64)f + 1] = (u32)block_place<kArith>(frames, (u32)first).frameLen;
}

// table: skippable header | n entries of 8 bytes | footer, one byte per lane (dst has no alignment to speak of)
__device__ __forceinline__ u8 seek_table_byte(const u32* __restrict__ entries, u32 n, u64 i)       // byte i < 17 + 8 n of the table
{
    const u64 bytes = 17 + 8 * (u64)n;
    u32 word; u32 k;
    if (i < 8) { word = i < 4 ? 0x184D2A5Eu : (u32)(bytes - 8); k = (u32)i & 3; }
    else if (i < 8 + 8 * (u64)n) { word = entries[(i - 8) >> 2]; k = (u32)i & 3; }
    else {
        const u32 j = (u32)(i - 8 - 8 * (u64)n);        // footer: count (4) | descriptor 0 | magic (4)
        if (j == 4) return 0;
        word = j < 4 ? n : 0x8F92EAB1u; k = j < 4 ? j : j - 5;
    }
    return (u8)(word >> (8 * k));
}
__global__ __launch_bounds__(256) void seek_table_kernel(const u32* __restrict__ entries, u32 n, u8* __restrict__ dst)
{
    const u64 bytes = 17 + 8 * (u64)n;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= bytes) return;
    dst[i] = seek_table_byte(entries, n, i);
}

// ---- a pack (ZSTDMI_compressPack): n entries' frames side by side in ONE stream, one seek table behind them ----
// entries of a batched pass: entry e owns the chunks [entFirst[e], entFirst[e + 1]) and its frames the table rows from entSeek[e] on.
// A frame is frameBlocks consecutive chunks of the entry (its last one may be shorter), one chunk where frameBlocks is 0: compressed
// size = the chunks' frame bytes, content size = their lengths — seek_entries_kernel's pairs, from the per-chunk tables instead of the
// arithmetic form.  One lane per entry; a row at or beyond `cap` is not written (the host sized the rows from the same framing).
__global__ __launch_bounds__(256) void pack_entries_kernel(const ChunkMeta* __restrict__ meta, u32 nEntries, const u32* __restrict__ entFirst,
                                                           const u32* __restrict__ chunkLens, u32 frameBlocks, const u32* __restrict__ entSeek,
                                                           u32* __restrict__ entries, u32 cap)
{
    const u32 e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nEntries) return;
    const u32 c0 = entFirst[e], c1 = entFirst[e + 1], fb = frameBlocks ? frameBlocks : 1u;
    u32 row = entSeek[e];
    for (u32 c = c0; c < c1; ++row) {
        u32 cSize = 0, dSize = 0;
        for (u32 k = 0; k < fb && c < c1; ++k, ++c) { cSize += meta[c].outSize; dSize += chunkLens[c]; }
        if (row < cap) { entries[2 * (u64)row] = cSize; entries[2 * (u64)row + 1] = dSize; }
    }
}

// placement: at[e] = the exclusive sum of size[0 .. e), entry e's offset from the round's first byte in the stream.  One workgroup
// striding with a carry, as scan_sizes_kernel (a round holds at most a few hundred thousand entries); 64-bit sums throughout: 1024
// stored entries of 4 MiB do not fit 32 bits.
__device__ __forceinline__ u64 wave_scan_incl64(u64 v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u64 t = __shfl_up(v, d); if ((int)lane_id() >= d) v += t; }
    return v;
}
__global__ __launch_bounds__(1024) void pack_place_kernel(const u64* __restrict__ size, u32 nEntries, u64* __restrict__ at)
{
    __shared__ u64 waveSum[16];
    const u32 tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    u64 carry = 0;
    for (u32 base = 0; base < nEntries; base += 1024) {
        const u32 i = base + tid;
        const u64 v = i < nEntries ? size[i] : 0;
        const u64 incl = wave_scan_incl64(v);
        if (lane == 63) waveSum[wave] = incl;
        __syncthreads();
        u64 before = 0, all = 0;
#pragma unroll
        for (u32 k = 0; k < 16; k++) { const u64 s = waveSum[k]; all += s; if (k < wave) before += s; }
        if (i < nEntries) at[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
}

// gather: entry e's size[e] bytes from its arena slot (slot[e], 16-byte aligned; slot[e + 1] - slot[e] bytes long) to dst + at[e], any
// alignment, the entries densely side by side.  The unit of work is a wave and a slice: blockIdx.x = a group of kPackGroup entries,
// dealt to the workgroup's four waves in turn; blockIdx.y = the kPackSlice bytes of an entry this workgroup copies, so that a long
// entry (a stored one: megabytes) is spread over the chip and a group of short ones (20 bytes each) costs one workgroup, not sixteen.
// A slice goes as ranges_gather's pieces do, in 16-byte stores at the DESTINATION's alignment fed by unaligned 16-byte loads, the ragged
// head and tail byte by byte: every store lies in [dst + at[e] + lo, dst + at[e] + hi) with hi <= size[e], every load below size[e] in
// the slot.  An entry that does not fit its slot or `room` is not copied (the host compared the sum with the capacity before the launch).
constexpr u32 kPackGroup = 16, kPackSlice = 16u << 10;
__device__ __forceinline__ void wave_copy(u8* __restrict__ d, const u8* __restrict__ s, u32 n, u32 lane)
{
    u32 head = (u32)((16 - ((uintptr_t)d & 15)) & 15);
    if (head > n) head = n;
    if (lane < head) d[lane] = s[lane];
    const u32 body = (n - head) >> 4;
    uint4* d4 = reinterpret_cast<uint4*>(d + head);
    const u8* sb = s + head;
#pragma unroll 4
    for (u32 i = lane; i < body; i += kWave) {
        uint4 v;
        v.x = readLE32(sb + 16 * i); v.y = readLE32(sb + 16 * i + 4); v.z = readLE32(sb + 16 * i + 8); v.w = readLE32(sb + 16 * i + 12);
        d4[i] = v;
    }
    const u32 done = head + (body << 4);
    if (lane < n - done) d[done + lane] = s[done + lane];
}
__global__ __launch_bounds__(256) void pack_gather_kernel(const u8* __restrict__ arena, const u64* __restrict__ slot, const u64* __restrict__ size,
                                                          const u64* __restrict__ at, u32 nEntries, u8* __restrict__ dst, u64 room)
{
    const u32 lane = lane_id();
    const u64 lo = (u64)blockIdx.y * kPackSlice;
    for (u32 k = wave_id(); k < kPackGroup; k += 4) {
        const u32 e = blockIdx.x * kPackGroup + k;
        if (e >= nEntries) return;
        const u64 n = size[e];
        if (lo >= n) continue;
        const u64 s0 = slot[e], a = at[e];
        if (n > slot[e + 1] - s0 || a > room || n > room - a) continue;
        const u64 hi = n < lo + kPackSlice ? n : lo + kPackSlice;
        wave_copy(dst + a + lo, arena + s0 + lo, (u32)(hi - lo), lane);
    }
}

// ---- a pack enqueued from the device (ZSTDMI_compressPackAsync): the planned batch's pass with ONE destination ----
// The sizes are known behind seq_encode, before huf_encode and gather move a byte, and both write to absolute addresses through
// offsets[c]: so the placement below gives every chunk its final address in the stream, and there is no arena and no second copy.
// place, entries: in the place of batch_place_async_frames.  ONE workgroup of 1024 lanes, 16 consecutive entries per lane
// (batch_plan_entries_kernel's shape; n <= 16384).  A lane sums its entries' chunks (pack_bytes) and counts their frames (pack_frames)
// into registers; the lanes' sums go through a 64-bit scan of bytes and a 32-bit scan of rows by wave, the wave totals through LDS, and
// the lowest failing entry through a min reduction.  pack_answer is the one decision — the first failure's verdict, else frames plus
// table against the capacity — and from it every lane writes its entries' place and first row (entAt, entRow: what the chunk kernel
// reads), the empty frames byte by byte with their rows, and entryEnds; lane 0 writes *packSize and the state the other two kernels
// read.  After a failure nothing but *packSize and that state is written.  n == 0: the decision alone (the empty table).
__global__ __launch_bounds__(1024) void pack_place_async_kernel(const ChunkMeta* __restrict__ meta, u32 n, const AsyncEntryTab tab, u32 frameBlocks,
                                                                const AsyncEmptyFrame empty, u8* __restrict__ dst, u64 cap, const PackAsyncTab pk,
                                                                size_t* __restrict__ packSize, size_t* __restrict__ entryEnds)
{
    __shared__ u64 waveBytes[16];
    __shared__ u32 waveRows[16], waveFail[16];
    const u32 tid = threadIdx.x, lane = lane_id(), wave = wave_id(), e0 = tid * kPlanPerLane;
    u64 bytes[kPlanPerLane], mine = 0;
    u32 rows[kPlanPerLane], myRows = 0, fail = kPackNoFail, emptyMask = 0;
#pragma unroll
    for (u32 k = 0; k < kPlanPerLane; ++k) {
        const u32 e = e0 + k;
        bytes[k] = 0; rows[k] = 0;
        if (e < n) {
            const u32 v = tab.verdict[e], c0 = tab.first[e], c1 = tab.first[e + 1];
            u64 sum = 0;
            for (u32 c = c0; c < c1; ++c) sum += meta[c].outSize;
            bytes[k] = pack_bytes(v, sum, empty.len);
            rows[k] = pack_frames(v, c1 - c0, frameBlocks);
            if (v == kAsyncEmpty) emptyMask |= 1u << k;
            if (pack_fails(v) && fail == kPackNoFail) fail = e;
        }
        mine += bytes[k]; myRows += rows[k];
    }
    const u64 inclB = wave_scan_incl64(mine);
    const u32 inclR = wave_scan_incl(myRows);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u32 t = __shfl_xor(fail, d); fail = t < fail ? t : fail; }
    if (lane == 63) { waveBytes[wave] = inclB; waveRows[wave] = inclR; }
    if (lane == 0) waveFail[wave] = fail;
    __syncthreads();
    u64 beforeB = 0, allB = 0;
    u32 beforeR = 0, allR = 0, failAll = kPackNoFail;
#pragma unroll
    for (u32 k = 0; k < 16; k++) {
        const u64 b = waveBytes[k]; const u32 r = waveRows[k], f = waveFail[k];
        allB += b; allR += r; failAll = f < failAll ? f : failAll;
        if (k < wave) { beforeB += b; beforeR += r; }
    }
    const u64 answer = pack_answer(failAll == kPackNoFail ? kPackNoFail : tab.verdict[failAll], allB, allR, cap);
    const bool ok = pack_answer_ok(answer);
    if (tid == 0) { *packSize = (size_t)answer; pk.state[kPackStateOk] = ok; pk.state[kPackStateTableAt] = allB; pk.state[kPackStateRows] = allR; }
    if (!ok) return;
    u64 at = beforeB + inclB - mine;
    u32 row = beforeR + inclR - myRows;
#pragma unroll
    for (u32 k = 0; k < kPlanPerLane; ++k) {
        const u32 e = e0 + k;
        if (e < n) {
            pk.entAt[e] = at; pk.entRow[e] = row;
            if (emptyMask >> k & 1) {
                for (u32 i = 0; i < empty.len; ++i) dst[at + i] = empty.bytes[i];
                pk.rows[2 * (u64)row] = empty.len; pk.rows[2 * (u64)row + 1] = 0;
            }
            if (entryEnds) entryEnds[e] = (size_t)(at + bytes[k]);
        }
        at += bytes[k]; row += rows[k];
    }
}

// place, chunks: one lane per chunk slot of the grid.  A slot below the call's total finds its entry (plan_owner) and gets its address:
// the destination + the entry's place + the frame bytes of the entry's chunks in front of it; the lane of a frame's first chunk files
// the frame's row (pack_entries_kernel's pair: the chunks' frame bytes, the chunks' lengths).  An idle slot, and every slot of a failed
// pack, gets the offset kAsyncSpan.  A lane loops over chunks of its own entry only (at most 255).
__global__ __launch_bounds__(256) void pack_place_chunks_kernel(const ChunkMeta* __restrict__ meta, u32 n, u32 nLaunch, const AsyncEntryTab tab,
                                                                const u32* __restrict__ len, u32 frameBlocks, const u8* __restrict__ dst,
                                                                const PackAsyncTab pk, u64* __restrict__ offsets)
{
    const u32 c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nLaunch) return;
    u64 off = kAsyncSpan;
    if (pk.state[kPackStateOk] && c < tab.first[n]) {
        const u32 e = plan_owner(tab.first, n, c), c0 = tab.first[e], k = c - c0;
        u64 inner = 0;
        for (u32 j = c0; j < c; ++j) inner += meta[j].outSize;
        off = pack_chunk_at(true, (u64)(uintptr_t)dst, pk.entAt[e], inner);
        if (pack_row_lead(k, frameBlocks)) {
            const u32 c1 = tab.first[e + 1], fb = frameBlocks ? frameBlocks : 1u, row = pack_row(pk.entRow[e], k, frameBlocks);
            u32 cSize = 0, dSize = 0;
            for (u32 j = c; j < c + fb && j < c1; ++j) { cSize += meta[j].outSize; dSize += len[j]; }
            pk.rows[2 * (u64)row] = cSize; pk.rows[2 * (u64)row + 1] = dSize;
        }
    }
    offsets[c] = off;
}

// table: seek_table_kernel's byte-per-lane writer with the row count and the table's place read from the placement's state; the grid
// covers the most rows the prepare admits.  Nothing is written for a failed pack.
__global__ __launch_bounds__(256) void pack_table_async_kernel(const PackAsyncTab pk, u8* __restrict__ dst)
{
    if (!pk.state[kPackStateOk]) return;
    const u32 n = (u32)pk.state[kPackStateRows];
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= 17 + 8 * (u64)n) return;
    dst[pk.state[kPackStateTableAt] + i] = seek_table_byte(pk.rows, n, i);
}

// ---- XXH64 (seed 0): 4 lanes per chunk, one per accumulator ----
constexpr u64 P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL,
              P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
__device__ __forceinline__ u64 rotl64(u64 x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ u64 xxh_round(u64 acc, u64 in) { acc += in * P2; acc = rotl64(acc, 31); return acc * P1; }
__device__ __forceinline__ u64 xxh_merge(u64 acc, u64 v) { acc ^= xxh_round(0, v); return acc * P1 + P4; }

// (frames, zmi_frame.h: the frame's bytes lie in one piece from its first chunk on; the checksum is filed with the frame's last block,
// which carries it.  frames.frameBlocks >= 1.)
// chunkLens (optional; single-block frames only): chunk c holds chunkLens[c] bytes at c * chunkBytes (a batch of independent inputs)
// The table form (a batch's multi-block frames, see lz_kernel): one group of 4 lanes per CHUNK, of which the groups of the frames'
// first blocks hash and the others leave; else one group per frame.
__global__ __launch_bounds__(256) void xxh64_kernel(const u8* __restrict__ src, ChunkMeta* __restrict__ meta, u32 nChunks, const FrameLayout frames,
                                                    const u32* __restrict__ chunkLens)
{
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    const u32 f = t >> 2, j = t & 3;
    const u64 first = frames.form == kTable ? (u64)f : (u64)f * frames.frameBlocks;     // the chunk this group looks at
    if (first >= nChunks) return;                          // whole groups of 4 lanes leave together
    const BlockPlace at = frames.form == kTable ? block_place<kTable>(frames, (u32)first) : block_place<kArith>(frames, (u32)first);
    if (at.block) return;
    const u32 n = chunkLens ? chunkLens[f] : (u32)at.frameLen;
    const u32 c = (u32)first + (n ? (n - 1) / frames.chunkBytes : 0u);        // the frame's last block
    const u8* p = src + first * frames.chunkBytes;
    u64 h;
    const u32 stripes = n >> 5;
    u64 v = j == 0 ? P1 + P2 : j == 1 ? P2 : j == 2 ? 0 : 0 - P1;
    for (u32 i = 0; i < stripes; i++) v = xxh_round(v, readLE64(p + 32 * i + 8 * j));
    const u32 l0 = threadIdx.x & 60;    // first lane of this group within the wave (groups never straddle waves)
    const u64 v1 = __shfl(v, (l0 & 63) + 0), v2 = __shfl(v, (l0 & 63) + 1), v3 = __shfl(v, (l0 & 63) + 2), v4 = __shfl(v, (l0 & 63) + 3);
    if (j != 0) return;
    if (n >= 32) {
        h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        h = xxh_merge(h, v1); h = xxh_merge(h, v2); h = xxh_merge(h, v3); h = xxh_merge(h, v4);
    } else h = P5;
    h += (u64)n;
    const u8* q = p + (stripes << 5); const u8* const end = p + n;
    while (q + 8 <= end) { h ^= xxh_round(0, readLE64(q)); h = rotl64(h, 27) * P1 + P4; q += 8; }
    if (q + 4 <= end) { h ^= (u64)readLE32(q) * P1; h = rotl64(h, 23) * P2 + P3; q += 4; }
    while (q < end) { h ^= (*q) * P5; h = rotl64(h, 11) * P1; q++; }
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    meta[c].checksum = (u32)h;
}

// ---- XXH64 with carried state: a frame whose content arrives in pieces (a segmented stream's fragments on the decoder's side,
// DESIGN.md 5i; the passes and stream batches of the compressor's single frame) ----
// XXH64 update over data[0, n) (U/ZstdDecompress.cs:1186-1208 across calls: XXH64_update), accumulator j on lane j; final: the digest's
// low 32 bits into st->hash (XXH64_digest).  One wave.
__global__ __launch_bounds__(64) void stream_xxh_kernel(XxhCarry* __restrict__ st, const u8* __restrict__ data, u64 n, u32 final)
{
    const u64 P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL, P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
    auto rotl = [](u64 x, int r) { return (x << r) | (x >> (64 - r)); };
    auto rnd = [&](u64 acc, u64 in) { acc += in * P2; acc = rotl(acc, 31); return acc * P1; };
    const u32 lane = threadIdx.x, j = lane & 3;
    u64 v = st->acc[j];
    u32 tailLen = uniform(st->tailLen);
    if (tailLen > 31) tailLen = 31;                             // (never: the struct is only written here and by the host's reset)
    if ((u64)tailLen + n >= 32) {
        u64 used = 0;                                           // bytes of data consumed
        if (tailLen) {                                          // the stripe the carried bytes begin
            if (lane < 4) {
                u64 w = 0;
                for (u32 i = 0; i < 8; ++i) { const u32 x = 8 * j + i; const u8 b = x < tailLen ? st->tail[x] : data[x - tailLen]; w |= (u64)b << (8 * i); }
                v = rnd(v, w);
            }
            used = 32 - tailLen;
        }
        const u64 stripes = (n - used) >> 5;
        if (lane < 4) {
            const u8* p = data + used + 8 * j;
            u64 i = 0;
            for (; i + 4 <= stripes; i += 4) {                  // four loads in flight per accumulator
                const u64 a0 = readLE64(p + 32 * i), a1 = readLE64(p + 32 * i + 32), a2 = readLE64(p + 32 * i + 64), a3 = readLE64(p + 32 * i + 96);
                v = rnd(v, a0); v = rnd(v, a1); v = rnd(v, a2); v = rnd(v, a3);
            }
            for (; i < stripes; ++i) v = rnd(v, readLE64(p + 32 * i));
        }
        used += stripes << 5;
        __syncthreads();                                        // the carried bytes have been read
        tailLen = (u32)(n - used);
        if (lane < tailLen) st->tail[lane] = data[used + lane];
    } else {
        if (lane < n) st->tail[tailLen + lane] = data[lane];
        tailLen += (u32)n;
    }
    if (lane < 4) st->acc[j] = v;
    const u64 total = st->total + n;
    __syncthreads();
    if (lane == 0) { st->total = total; st->tailLen = tailLen; }
    if (!final) return;
    const u64 v1 = __shfl(v, 0), v2 = __shfl(v, 1), v3 = __shfl(v, 2), v4 = __shfl(v, 3);
    if (lane == 0) {
        u64 hh;
        if (total >= 32) {
            hh = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
            auto mrg = [&](u64 acc, u64 x) { acc ^= rnd(0, x); return acc * P1 + P4; };
            hh = mrg(hh, v1); hh = mrg(hh, v2); hh = mrg(hh, v3); hh = mrg(hh, v4);
        } else hh = P5;
        hh += total;
        const u8* q = st->tail; const u8* const end = st->tail + tailLen;
        while (q + 8 <= end) { hh ^= rnd(0, readLE64(q)); hh = rotl(hh, 27) * P1 + P4; q += 8; }
        if (q + 4 <= end) { hh ^= (u64)readLE32(q) * P1; hh = rotl(hh, 23) * P2 + P3; q += 4; }
        while (q < end) { hh ^= (*q) * P5; hh = rotl(hh, 11) * P1; q++; }
        hh ^= hh >> 33; hh *= P2; hh ^= hh >> 29; hh *= P3; hh ^= hh >> 32;
        st->hash = (u32)hh;
    }
}

// the finished hash into the chunk whose block carries the frame's checksum (gather writes it behind that block)
__global__ void xxh_carry_file_kernel(const XxhCarry* __restrict__ st, ChunkMeta* __restrict__ chunk)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) chunk->checksum = st->hash;
}

void launch_scan_sizes(const ChunkMeta* meta, u32 nChunks, u64* offsets, u64* total, hipStream_t stream, u64* pinned, const PassMarks& marks)
{
    hipLaunchKernelGGL(scan_sizes_kernel, dim3(1), dim3(1024), 0, stream, meta, nChunks, offsets, total, pinned, marks);
}
void launch_gather(const u8* src, u64 srcSize, const u8* slots, const ChunkMeta* meta, const u64* offsets, u8* dst, u64 dstCapacity,
                   u32 nChunks, u32 chunkBytes, hipStream_t stream)
{
    hipLaunchKernelGGL(gather_kernel, dim3(nChunks), dim3(256), 0, stream, src, srcSize, slots, meta, offsets, dst, dstCapacity, chunkBytes);
}
void launch_xxh64(const u8* src, ChunkMeta* meta, u32 nChunks, const FrameLayout& frames, hipStream_t stream, const u32* chunkLens)
{
    assert(frames.form != kSingle);                         // (one frame across passes: launch_stream_xxh)
    FrameLayout g = frames;
    if (!g.frameBlocks) g.frameBlocks = 1;
    assert(g.form == kArith || g.frameBlocks > 1);          // (the table states multi-block frames only)
    if (g.frameBlocks != 1) chunkLens = nullptr;
    const u32 nFrames = g.form == kTable ? nChunks : (nChunks + g.frameBlocks - 1) / g.frameBlocks;
    hipLaunchKernelGGL(xxh64_kernel, dim3((nFrames * 4 + 255) / 256), dim3(256), 0, stream, src, meta, nChunks, g, chunkLens);
}
void launch_stream_xxh(XxhCarry* st, const u8* data, u64 n, u32 final, hipStream_t stream)
{
    hipLaunchKernelGGL(stream_xxh_kernel, dim3(1), dim3(64), 0, stream, st, data, n, final);
}
void launch_xxh_carry_file(const XxhCarry* st, ChunkMeta* chunk, hipStream_t stream)
{
    hipLaunchKernelGGL(xxh_carry_file_kernel, dim3(1), dim3(64), 0, stream, st, chunk);
}
void launch_seek_entries(const u64* offsets, const u64* total, u32 nChunks, const FrameLayout& frames, u32* entries, hipStream_t stream)
{
    assert(frames.form == kArith);
    FrameLayout g = frames;
    if (!g.frameBlocks) g.frameBlocks = 1;
    const u32 nFrames = (nChunks + g.frameBlocks - 1) / g.frameBlocks;
    hipLaunchKernelGGL(seek_entries_kernel, dim3((nFrames + 255) / 256), dim3(256), 0, stream, offsets, total, nChunks, g, entries);
}
void launch_seek_table(const u32* entries, u32 n, u8* dst, hipStream_t stream)
{
    const u64 bytes = 17 + 8 * (u64)n;
    hipLaunchKernelGGL(seek_table_kernel, dim3((u32)((bytes + 255) / 256)), dim3(256), 0, stream, entries, n, dst);
}
void launch_pack_entries(const ChunkMeta* meta, u32 nEntries, const u32* entFirst, const u32* chunkLens, u32 frameBlocks, const u32* entSeek, u32* entries,
                         u32 cap, hipStream_t stream)
{
    hipLaunchKernelGGL(pack_entries_kernel, dim3((nEntries + 255) / 256), dim3(256), 0, stream, meta, nEntries, entFirst, chunkLens, frameBlocks, entSeek, entries, cap);
}
void launch_pack_place(const u64* size, u32 nEntries, u64* at, hipStream_t stream)
{
    hipLaunchKernelGGL(pack_place_kernel, dim3(1), dim3(1024), 0, stream, size, nEntries, at);
}
void launch_pack_gather(const u8* arena, const u64* slot, const u64* size, const u64* at, u32 nEntries, u64 longest, u8* dst, u64 room, hipStream_t stream)
{
    const u32 nSlices = (u32)((longest + kPackSlice - 1) / kPackSlice);
    hipLaunchKernelGGL(pack_gather_kernel, dim3((nEntries + kPackGroup - 1) / kPackGroup, nSlices ? nSlices : 1), dim3(256), 0, stream, arena, slot, size, at,
                       nEntries, dst, room);
}
void launch_pack_place_async(const ChunkMeta* meta, u32 n, u32 nLaunch, const AsyncEntryTab& tab, const u32* len, u32 frameBlocks, AsyncEmptyFrame empty, u8* dst,
                             u64 cap, const PackAsyncTab& pk, u64* offsets, size_t* packSize, size_t* entryEnds, hipStream_t stream)
{
    assert(empty.len <= sizeof empty.bytes && n <= 1024 * kPlanPerLane);
    hipLaunchKernelGGL(pack_place_async_kernel, dim3(1), dim3(1024), 0, stream, meta, n, tab, frameBlocks, empty, dst, cap, pk, packSize, entryEnds);
    if (nLaunch) hipLaunchKernelGGL(pack_place_chunks_kernel, dim3((nLaunch + 255) / 256), dim3(256), 0, stream, meta, n, nLaunch, tab, len, frameBlocks, dst, pk, offsets);
}
void launch_pack_table_async(const PackAsyncTab& pk, u64 maxRows, u8* dst, hipStream_t stream)
{
    const u64 bytes = 17 + 8 * maxRows;
    hipLaunchKernelGGL(pack_table_async_kernel, dim3((u32)((bytes + 255) / 256)), dim3(256), 0, stream, pk, dst);
}
void launch_batch_stage(const u64* from, const u32* len, u8* stage, u32 nChunks, u32 chunkBytes, hipStream_t stream)
{
    hipLaunchKernelGGL(batch_stage_kernel, dim3(nChunks), dim3(256), 0, stream, from, len, stage, chunkBytes);
}
void launch_batch_place(const ChunkMeta* meta, u32 nEntries, const u32* entFirst, const u64* entDst, const u64* entCap, u64 span, u64* offsets, u64* entSize,
                        hipStream_t stream)
{
    hipLaunchKernelGGL(batch_place_kernel, dim3((nEntries + 255) / 256), dim3(256), 0, stream, meta, nEntries, entFirst, entDst, entCap, span, offsets, entSize);
}
void launch_batch_plan(const void* const* srcs, const size_t* sizes, void* const* dsts, const size_t* caps, u32 n, u64 bound, u32 emptyLen, const u8* dummy,
                       u64* from, u64* entDst, u64* entCap, u32* len, u32* entFirst, u32* verdict, hipStream_t stream)
{
    hipLaunchKernelGGL(batch_plan_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, srcs, sizes, dsts, caps, n, bound, emptyLen, dummy, from, entDst, entCap, len,
                       entFirst, verdict);
}
void launch_batch_place_async(const ChunkMeta* meta, u32 n, const u64* entDst, const u64* entCap, const u32* verdict, AsyncEmptyFrame empty,
                              u64* offsets, size_t* dstSizes, hipStream_t stream)
{
    assert(empty.len <= sizeof empty.bytes);
    hipLaunchKernelGGL(batch_place_async_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, meta, n, entDst, entCap, verdict, empty, offsets, dstSizes);
}
void launch_batch_plan_entries(const void* const* srcs, const size_t* sizes, void* const* dsts, const size_t* caps, u32 n, u64 bound, u32 emptyLen,
                               u32 chunkBytes, u32 maxChunks, const AsyncEntryTab& tab, hipStream_t stream)
{
    assert(n && n <= 1024 * kPlanPerLane && bound <= kAsyncBoundMax && chunkBytes);
    hipLaunchKernelGGL(batch_plan_entries_kernel<false>, dim3(1), dim3(1024), 0, stream, srcs, sizes, dsts, caps, n, bound, emptyLen, chunkBytes, maxChunks, tab);
}
void launch_pack_plan_entries(const void* const* srcs, const size_t* sizes, u32 n, u64 bound, u32 chunkBytes, u32 maxChunks, const AsyncEntryTab& tab, hipStream_t stream)
{
    assert(n && n <= 1024 * kPlanPerLane && bound <= kAsyncBoundMax && chunkBytes);
    hipLaunchKernelGGL(batch_plan_entries_kernel<true>, dim3(1), dim3(1024), 0, stream, srcs, sizes, (void* const*)nullptr, (const size_t*)nullptr, n, bound, 0u, chunkBytes,
                       maxChunks, tab);
}
void launch_batch_plan_chunks(const AsyncEntryTab& tab, u32 n, u32 nLaunch, u32 chunkBytes, u32 frameBlocks, const u8* dummy, u64* from, u32* len, u32* frame,
                              hipStream_t stream)
{
    assert(!frameBlocks == !frame);
    hipLaunchKernelGGL(batch_plan_chunks_kernel, dim3((nLaunch + 255) / 256), dim3(256), 0, stream, tab, n, nLaunch, chunkBytes, frameBlocks, dummy, from, len, frame);
}
void launch_batch_place_async_frames(const ChunkMeta* meta, u32 n, u32 nLaunch, const AsyncEntryTab& tab, AsyncEmptyFrame empty, u64* offsets, size_t* dstSizes,
                                     hipStream_t stream)
{
    assert(empty.len <= sizeof empty.bytes);
    hipLaunchKernelGGL(batch_place_async_frames_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, meta, n, nLaunch, tab, empty, offsets, dstSizes);
}

} // namespace zmi
