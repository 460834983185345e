// decode_ranges.hip — many ranges of a seekable stream in one call (ZSTDMI_decompressRanges) on gfx950: the front and the back of the
// pass around the batch's core (decode_entries).  DESIGN.md §5h.
//
//   seek_index     : the seek table -> two exclusive prefix arrays of N + 1 words (compressed offset, content offset) and the table's
//                    validation, as a grid-wide reduce-then-scan: tile sums, one workgroup scans the sums, tile scans.
//   ranges_select  : one lane per range: clip, decide tooSmall / empty / alone, else find the first and last entry with content by
//                    two binary searches in the content offsets and mark [first, last] with +1 / -1 on a difference array.
//   ranges_plan    : two grid-wide scans over the entries: ranges over each entry (the difference array's prefix sum), then, over the
//                    touched entries (covered, with content), their index in the decode table, their arena slot and their place in
//                    the compacted source.  Writes the batch walk's table, and the runs of touched entries for a host source.
//   ranges_gather  : per served range: every met entry decoded to the size its table entry names, or nothing is copied; then its
//                    bytes from the arena slots to its destination, one workgroup per 64 KiB slice of its output.
//   ranges_select_d, ranges_plan_d : the select and the plan's emit of ZSTDMI_decompressRangesAsync: the caller's
//                    arrays lie in device memory, the index is a prepare's, the decode table has a fixed number of rows.
#include "zmi_device.h"
#include "zmi_host.h"

namespace zmi {

// exclusive prefix of K columns over the 1024 lanes of a workgroup, and the workgroup's sums (sh: K x kScanSh words: the 16 waves'
// sums, scanned by the first wave, and their total)
constexpr u32 kScanSh = 17;
template <int K> __device__ inline void block_scan(const u64 (&v)[K], u64 (&ex)[K], u64 (&all)[K], u64* __restrict__ sh)
{
    const u32 lane = lane_id(), wave = wave_id();
    u64 inc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) inc[k] = v[k];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) { const u64 t = __shfl_up(inc[k], d); if ((int)lane >= d) inc[k] += t; }
    }
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh[k * kScanSh + wave] = inc[k];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const u64 own = lane < 16 ? sh[k * kScanSh + lane] : 0;
            u64 w = own;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) { const u64 t = __shfl_up(w, d); if ((int)lane >= d) w += t; }
            if (lane < 16) sh[k * kScanSh + lane] = w - own;
            if (lane == 15) sh[k * kScanSh + 16] = w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) { ex[k] = sh[k * kScanSh + wave] + inc[k] - v[k]; all[k] = sh[k * kScanSh + 16]; }
    __syncthreads();
}

// the middle step of every grid-wide scan here (single workgroup): tile sums -> exclusive tile carries in place, the totals in row nTiles
template <int K> __global__ __launch_bounds__(1024) void tile_carry_kernel(u64* __restrict__ tile, u32 nTiles)
{
    __shared__ u64 sh[K * kScanSh];
    const u32 tid = threadIdx.x;
    u64 carry[K];
#pragma unroll
    for (int k = 0; k < K; ++k) carry[k] = 0;
    for (u32 base = 0; base < nTiles; base += 1024) {
        const u32 t = base + tid;
        u64 v[K], ex[K], all[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = t < nTiles ? tile[(u64)t * K + k] : 0;
        block_scan<K>(v, ex, all, sh);
#pragma unroll
        for (int k = 0; k < K; ++k) { if (t < nTiles) tile[(u64)t * K + k] = carry[k] + ex[k]; carry[k] += all[k]; }
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) tile[(u64)nTiles * K + k] = carry[k];
    }
}

// entry i of the table: (compressed size, content size); a checksum behind the two sizes is skipped.  i == n: the end marker (0, 0)
__device__ __forceinline__ void table_entry(const u8* __restrict__ tab, u32 n, u32 stride, u32 i, u64& c, u64& d)
{
    c = 0; d = 0;
    if (i < n) { const u8* p = tab + 8 + (u64)i * stride; c = readLE32(p); d = readLE32(p + 4); }
}

// ------------------------------------------------------------------------------------------------
// seek_index: tile sums, [tile_carry], tile scans
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void seek_index_sum_kernel(const u8* __restrict__ tab, u32 n, u32 stride, u64* __restrict__ tile)
{
    __shared__ u64 sh[2 * kScanSh];
    u64 v[2], ex[2], all[2];
    table_entry(tab, n, stride, blockIdx.x * kRangesTile + threadIdx.x, v[0], v[1]);
    block_scan<2>(v, ex, all, sh);
    if (threadIdx.x == 0) { tile[(u64)blockIdx.x * 2] = all[0]; tile[(u64)blockIdx.x * 2 + 1] = all[1]; }
}

// `tab` = the table's skippable frame (tableBytes of it; the host has read the footer).  Writes cOff / dOff [0 .. n], clears the
// difference array, and checks what seek_select_kernel checks: the header's magic and size field, and that the compressed sizes add up
// to the bytes in front of the table — so every offset derived from them lies inside the stream.
__global__ __launch_bounds__(1024) void seek_index_kernel(const u8* __restrict__ tab, u64 tableBytes, u32 n, u32 stride, u64 srcSize,
                                                          const u64* __restrict__ tile, u32 nTiles, RangesWs ws)
{
    __shared__ u64 sh[2 * kScanSh];
    const u32 i = blockIdx.x * kRangesTile + threadIdx.x;
    u64 v[2], ex[2], all[2];
    table_entry(tab, n, stride, i, v[0], v[1]);
    block_scan<2>(v, ex, all, sh);
    if (i <= n) {
        ws.cOff[i] = tile[(u64)blockIdx.x * 2] + ex[0]; ws.dOff[i] = tile[(u64)blockIdx.x * 2 + 1] + ex[1];
        ws.diff[i] = 0;
    }
    if (i == 0) {
        u32 err = 0;
        if (readLE32(tab) != 0x184D2A5Eu || (u64)readLE32(tab + 4) != tableBytes - 8) err = kErrPrefixUnknown;
        else if (tile[(u64)nTiles * 2] != srcSize - tableBytes) err = kErrCorruption;
        for (u32 k = 0; k < kRgWords; ++k) ws.sum[k] = 0;
        ws.sum[kRgErr] = err; ws.sum[kRgTotal] = tile[(u64)nTiles * 2 + 1];
    }
}

// first index in a[0 .. count) whose value is above x (a is non-decreasing)
__device__ __forceinline__ u32 upper_bound(const u64* __restrict__ a, u32 count, u64 x)
{
    u32 lo = 0, hi = count;
    while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (a[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}

// ------------------------------------------------------------------------------------------------
// ranges_select: one lane per range
// ------------------------------------------------------------------------------------------------
// The order of the answers is the single call's: more than the capacity, nothing to return, no destination.  A served range
// [offset, offset + ret) has 0 < ret and offset + ret <= total = dOff[n], so the entry that holds a byte of it exists, has content
// (dOff[j] <= x < dOff[j + 1]) and is found by one search; entries without content share their neighbour's offset and are never hit.
__global__ __launch_bounds__(256) void ranges_select_kernel(const RangeIn* __restrict__ in, RangeRec* __restrict__ recs, u32 nRanges,
                                                            const u64* __restrict__ dOff, u32 n, u32* __restrict__ diff)
{
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nRanges) return;
    const RangeIn R = in[r];
    const u64 total = dOff[n];
    const u64 ret = R.offset < total ? (R.length < total - R.offset ? R.length : total - R.offset) : 0;
    RangeRec rec = {};
    if (ret > R.dstCap) rec.result = (u64)0 - (u64)kErrDstSizeTooSmall;
    else if (!ret) rec.result = 0;
    else if (!R.dst) rec.result = (u64)0 - (u64)kErrDstBufferNull;
    else if (ret > kRangesAloneAbove) { rec.result = ret; rec.state = kRangeAlone; }
    else {
        rec.result = ret; rec.state = kRangeServed;
        rec.first = upper_bound(dOff, n + 1, R.offset) - 1;
        rec.last = upper_bound(dOff, n + 1, R.offset + ret - 1) - 1;
        atomicAdd(&diff[rec.first], 1u);
        atomicAdd(&diff[rec.last + 1], 0xFFFFFFFFu);
    }
    recs[r] = rec;
}

// ------------------------------------------------------------------------------------------------
// ranges_plan: cover sums, [tile_carry], touched sums, [tile_carry], emit
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ranges_cover_sum_kernel(const u32* __restrict__ diff, u32 n, u64* __restrict__ tile)
{
    __shared__ u64 sh[kScanSh];
    const u32 i = blockIdx.x * kRangesTile + threadIdx.x;
    u64 v[1], ex[1], all[1];
    v[0] = i < n ? diff[i] : 0;
    block_scan<1>(v, ex, all, sh);
    if (threadIdx.x == 0) tile[blockIdx.x] = all[0];
}

// what the plan knows of entry i = blockIdx.x * kRangesTile + threadIdx.x (both plan kernels compute it the same way)
struct PlanEntry { u64 c, d; u32 touched, start, end; };
__device__ inline PlanEntry plan_entry(const u8* __restrict__ tab, u32 n, u32 stride, const u32* __restrict__ diff,
                                       const u64* __restrict__ tileCover, u64* __restrict__ sh, u32* __restrict__ shTouched)
{
    const u32 tid = threadIdx.x, i = blockIdx.x * kRangesTile + tid;
    PlanEntry e;
    table_entry(tab, n, stride, i, e.c, e.d);
    u64 v[1], ex[1], all[1];
    v[0] = i < n ? diff[i] : 0;
    block_scan<1>(v, ex, all, sh);
    const u64 carry = tileCover[blockIdx.x];
    const u32 cover = (u32)(carry + ex[0] + v[0]);              // ranges over entry i (the +1 / -1 are mod 2^32, and so is this)
    e.touched = (i < n && cover > 0 && e.d > 0) ? 1u : 0u;
    shTouched[tid] = e.touched;
    __syncthreads();
    u32 prev;
    if (tid) prev = shTouched[tid - 1];
    else { u64 pc, pd; table_entry(tab, n, stride, i ? i - 1 : n, pc, pd); prev = (i && (u32)carry > 0 && pd > 0) ? 1u : 0u; }
    u32 next;
    if (tid + 1 < kRangesTile) next = shTouched[tid + 1];
    else { u64 nc, nd; table_entry(tab, n, stride, i + 1, nc, nd); next = (i + 1 < n && (u32)(cover + diff[i + 1]) > 0 && nd > 0) ? 1u : 0u; }
    __syncthreads();
    e.start = e.touched & (prev ^ 1u); e.end = e.touched & (next ^ 1u);
    return e;
}

__global__ __launch_bounds__(1024) void ranges_plan_sum_kernel(const u8* __restrict__ tab, u32 n, u32 stride, const u32* __restrict__ diff,
                                                               const u64* __restrict__ tileCover, u64* __restrict__ tilePlan)
{
    __shared__ u64 sh[4 * kScanSh];
    __shared__ u32 shTouched[kRangesTile];
    const PlanEntry e = plan_entry(tab, n, stride, diff, tileCover, sh, shTouched);
    u64 v[4] = {e.touched, e.touched ? e.d : 0, e.touched ? e.c : 0, e.start}, ex[4], all[4];
    block_scan<4>(v, ex, all, sh);
    if (threadIdx.x == 0) { for (u32 k = 0; k < 4; ++k) tilePlan[(u64)blockIdx.x * 4 + k] = all[k]; }
}

// emit: one BatchEntryIn per touched entry — destination = its arena slot, capacity = the table's content size (the walk refuses
// more), source = its compressed offset in the stream (device source) or in the compacted staging buffer (host source: the touched
// entries' bytes one behind the other) —, every entry's slot and decode index for the gather, and the runs for the host
__global__ __launch_bounds__(1024) void ranges_plan_kernel(const u8* __restrict__ tab, u32 n, u32 stride, u32 nTiles, u32 srcDev,
                                                           RangesWs ws, BatchEntryIn* __restrict__ out)
{
    __shared__ u64 sh[4 * kScanSh];
    __shared__ u32 shTouched[kRangesTile];
    const u32 i = blockIdx.x * kRangesTile + threadIdx.x;
    const PlanEntry e = plan_entry(tab, n, stride, ws.diff, ws.tileCover, sh, shTouched);
    u64 v[4] = {e.touched, e.touched ? e.d : 0, e.touched ? e.c : 0, e.start}, ex[4], all[4];
    block_scan<4>(v, ex, all, sh);
    const u64* carry = ws.tilePlan + (u64)blockIdx.x * 4;
    const u64 k = carry[0] + ex[0], slot = carry[1] + ex[1], packed = carry[2] + ex[2], run = carry[3] + ex[3];
    if (i < n) { ws.slot[i] = slot; ws.decIdx[i] = e.touched ? (u32)k : kNoEntry; }
    if (e.touched) {
        BatchEntryIn b; b.srcOff = srcDev ? ws.cOff[i] : packed; b.srcSize = e.c; b.dstOff = slot; b.dstCap = e.d;
        out[k] = b;
        if (e.start) ws.runs[2 * run] = ws.cOff[i];
        if (e.end) ws.runs[2 * (run + e.start - 1) + 1] = ws.cOff[i] + e.c;
    }
    if (i == 0) {
        const u64* tot = ws.tilePlan + (u64)nTiles * 4;
        ws.sum[kRgTouched] = tot[0]; ws.sum[kRgArena] = tot[1]; ws.sum[kRgCompact] = tot[2]; ws.sum[kRgRuns] = tot[3];
    }
}

// a touched entry that the batch walk left to the single-call path: the host decodes those in front of the gather (a flag, so that
// running it in front of both of decode_entries' read-backs changes nothing)
__global__ __launch_bounds__(256) void ranges_alone_kernel(const BatchEntryOut* __restrict__ out, u32 nEntries, u64* __restrict__ sum)
{
    const u32 e = blockIdx.x * 256 + threadIdx.x;
    if (e < nEntries && out[e].state == kBatchAlone) sum[kRgAloneEntries] = 1;
}

// ------------------------------------------------------------------------------------------------
// ranges_gather: blockIdx.x = the range, blockIdx.y = the 64 KiB slice of its output
// ------------------------------------------------------------------------------------------------
// First the range's entries (every workgroup of the range looks: a failed range writes nothing): one that failed or did not decode to
// the size its table entry names fails the range with the first such entry's code — entries the walk decoded in front of entries the
// single-call path decoded, as the single range call orders them; dstSize_tooSmall from the walk is corruption of the table, as in
// range_check_kernel.  Then the copy, in 16-byte pieces of the DESTINATION's alignment: a piece that lies in one entry is one
// unaligned 16-byte load from that entry's slot and one aligned store; the head, the tail and a piece across a boundary go byte by
// byte.  Every address is dst + q with lo <= q < hi <= ret, and arena + slot[j] + x with x below entry j's content size.
__global__ __launch_bounds__(256) void ranges_gather_kernel(const RangeIn* __restrict__ in, const RangeRec* __restrict__ recs, u64* __restrict__ res,
                                                            const u64* __restrict__ dOff, const u64* __restrict__ slot, const u32* __restrict__ decIdx,
                                                            const BatchEntryOut* __restrict__ out, const u8* __restrict__ arena)
{
    __shared__ unsigned long long key;
    const u32 r = blockIdx.x, tid = threadIdx.x;
    const RangeRec rec = recs[r];
    if (rec.state != kRangeServed) { if (blockIdx.y == 0 && tid == 0) res[r] = rec.result; return; }
    const u64 ret = rec.result, lo = (u64)blockIdx.y * kGatherSlice, hi = ret < lo + kGatherSlice ? ret : lo + kGatherSlice;
    if (lo >= ret) return;                  // (ret > 0: slice 0 always stays)
    if (tid == 0) key = ~0ull;
    __syncthreads();
    for (u64 j = (u64)rec.first + tid; j <= rec.last; j += 256) {
        const u32 k = decIdx[j];
        if (k == kNoEntry) continue;        // (no content)
        const BatchEntryOut o = out[k];
        u32 err = 0;
        if (o.result > (u64)0 - (u64)kErrMaxCode) { err = (u32)((u64)0 - o.result); if (err == kErrDstSizeTooSmall) err = kErrCorruption; }
        else if (o.result != dOff[j + 1] - dOff[j]) err = kErrCorruption;
        if (err) atomicMin(&key, (o.state == kBatchAlone ? 1ull << 63 : 0ull) | (j << 16) | err);
    }
    __syncthreads();
    const unsigned long long bad = key;
    if (blockIdx.y == 0 && tid == 0) res[r] = bad != ~0ull ? (u64)0 - (u64)(bad & 0xFFFFull) : ret;
    if (bad != ~0ull) return;

    const RangeIn R = in[r];
    u8* const dst = reinterpret_cast<u8*>(R.dst);
    const u64* const base = dOff + rec.first;
    const u32 span = rec.last - rec.first + 2;                  // dOff[first .. last + 1]: base[0] <= offset, base[span - 1] >= offset + ret
    const uintptr_t a0 = (uintptr_t)(dst + lo) & ~(uintptr_t)15, aLo = (uintptr_t)(dst + lo), aHi = (uintptr_t)(dst + hi);
    const u64 nPieces = (u64)(aHi - a0 + 15) >> 4;
    for (u64 p = tid; p < nPieces; p += 256) {
        const uintptr_t a = a0 + 16 * p;
        const u64 q0 = (a > aLo ? a : aLo) - (uintptr_t)dst, q1 = (a + 16 < aHi ? a + 16 : aHi) - (uintptr_t)dst;
        const u64 at = R.offset + q0;
        u32 j = rec.first + upper_bound(base, span, at) - 1;
        if (q1 - q0 == 16 && at + 16 <= dOff[j + 1]) {
            const u8* s = arena + slot[j] + (at - dOff[j]);
            uint4 v; v.x = readLE32(s); v.y = readLE32(s + 4); v.z = readLE32(s + 8); v.w = readLE32(s + 12);
            *reinterpret_cast<uint4*>(dst + q0) = v;
        } else {
            for (u64 q = q0; q < q1; ++q) {
                const u64 x = R.offset + q;
                while (x >= dOff[j + 1]) ++j;
                dst[q] = arena[slot[j] + (x - dOff[j])];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// ranges enqueued from the device (ZSTDMI_decompressRangesAsync): the select and the plan's last step over the caller's
// device arrays and a prepared index.  The scans between them, seek_index at the prepare and the gather are the kernels above.
// ------------------------------------------------------------------------------------------------
// select, one lane per range: the caller's four arrays -> RangeIn / RangeRec rows, ranges_select_kernel's answers in its order; where
// that kernel decides "alone", a range that would return more than maxRangeBytes (which sized the gather's grid) answers
// workSpace_tooSmall and marks nothing.  The difference array is zero when this runs: the index persists, the marks are the call's.
__global__ __launch_bounds__(256) void ranges_select_d_kernel(const unsigned long long* __restrict__ offsets, const size_t* __restrict__ lengths,
                                                              void* const* __restrict__ dsts, const size_t* __restrict__ caps, u32 nRanges, u64 maxRangeBytes,
                                                              RangeIn* __restrict__ in, RangeRec* __restrict__ recs, const u64* __restrict__ dOff, u32 n,
                                                              u32* __restrict__ diff)
{
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nRanges) return;
    RangeIn R;
    R.offset = offsets[r]; R.length = (u64)lengths[r]; R.dstCap = (u64)caps[r]; R.dst = (u64)(uintptr_t)dsts[r];
    const u64 total = dOff[n];
    const u64 ret = R.offset < total ? (R.length < total - R.offset ? R.length : total - R.offset) : 0;
    RangeRec rec = {};
    if (ret > R.dstCap) rec.result = (u64)0 - (u64)kErrDstSizeTooSmall;
    else if (!ret) rec.result = 0;
    else if (!R.dst) rec.result = (u64)0 - (u64)kErrDstBufferNull;
    else if (ret > maxRangeBytes) rec.result = (u64)0 - (u64)kErrWorkSpaceTooSmall;
    else {
        rec.result = ret; rec.state = kRangeServed;
        rec.first = upper_bound(dOff, n + 1, R.offset) - 1;
        rec.last = upper_bound(dOff, n + 1, R.offset + ret - 1) - 1;
        atomicAdd(&diff[rec.first], 1u);
        atomicAdd(&diff[rec.last + 1], 0xFFFFFFFFu);
    }
    in[r] = R; recs[r] = rec;
}

// emit (behind ranges_cover_sum, ranges_plan_sum and their carries, as ranges_plan_kernel): the decode core's table has nRows rows, a
// host constant.  Touched entry number k, in table order, is refused iff k + 1 exceeds maxFrames or its arena slot, the exclusive sum
// of the touched entries' table content sizes, would end beyond maxContent: both sums only grow, so the admitted entries are a prefix
// and none of their slots reaches beyond the arena whatever the frames' own headers say.  An admitted entry fills row k — its source
// and its slot as offsets from kAsyncBase, the base the core's kernels get —; every row nothing fills is an empty entry (srcSize 0),
// which walks as batch_plan_d_kernel's and costs no frame, block or byte.  A refused entry, and one of more than aloneAbove
// compressed bytes (there is no single-call path), points the gather at one of two verdict rows behind the table (rows nRows and
// nRows + 1: workSpace_tooSmall, srcSize_wrong), so ranges_gather_kernel fails their ranges as it fails any entry's.
__global__ __launch_bounds__(1024) void ranges_plan_d_kernel(const u8* __restrict__ tab, u32 n, u32 stride, u32 nTiles, RangesWs ws, u64 streamOff, u64 arenaOff,
                                                             u32 maxFrames, u64 maxContent, u64 aloneAbove, u32 nRows, BatchEntryIn* __restrict__ rows,
                                                             BatchEntryOut* __restrict__ verdicts)
{
    __shared__ u64 sh[4 * kScanSh];
    __shared__ u32 shTouched[kRangesTile];
    const u32 i = blockIdx.x * kRangesTile + threadIdx.x;
    const PlanEntry e = plan_entry(tab, n, stride, ws.diff, ws.tileCover, sh, shTouched);
    u64 v[4] = {e.touched, e.touched ? e.d : 0, e.touched ? e.c : 0, e.start}, ex[4], all[4];
    block_scan<4>(v, ex, all, sh);
    const u64* carry = ws.tilePlan + (u64)blockIdx.x * 4;
    const u64 k = carry[0] + ex[0], slot = carry[1] + ex[1];
    const u64* tot = ws.tilePlan + (u64)nTiles * 4;
    u32 idx = kNoEntry;
    if (e.touched) {
        const bool refused = k + 1 > maxFrames || slot + e.d > maxContent;
        idx = refused ? nRows : e.c > aloneAbove ? nRows + 1 : (u32)k;
        if (k < nRows) {
            BatchEntryIn b = {};
            if (idx == (u32)k) { b.srcOff = streamOff + ws.cOff[i]; b.srcSize = e.c; b.dstOff = arenaOff + slot; b.dstCap = e.d; }
            rows[k] = b;
        }
    }
    if (i < n) { ws.slot[i] = slot; ws.decIdx[i] = idx; }
    if ((u64)i >= tot[0] && i < nRows) rows[i] = BatchEntryIn{};
    if (i == 0) {
        BatchEntryOut o = {};
        o.state = kBatchDone;
        o.result = (u64)0 - (u64)kErrWorkSpaceTooSmall; verdicts[0] = o;
        o.result = (u64)0 - (u64)kErrSrcSizeWrong; verdicts[1] = o;
        ws.sum[kRgTouched] = tot[0]; ws.sum[kRgArena] = tot[1]; ws.sum[kRgCompact] = tot[2]; ws.sum[kRgRuns] = tot[3];
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t ranges_ws_bytes(u32 n)
{
    const size_t N = n, T = n / kRangesTile + 1;
    return 2 * up256((N + 1) * 8) + up256(N * 8) + up256((N + 2) * 8) + up256((T + 1) * 16) + up256((T + 1) * 8) + up256((T + 1) * 32) + up256(kRgWords * 8) +
           up256((N + 1) * 4) + up256(N * 4) + 256;
}
RangesWs ranges_ws(u8* p, u32 n)
{
    const size_t N = n, T = n / kRangesTile + 1;
    RangesWs w;
    auto take = [&](size_t bytes) { u8* q = p; p += up256(bytes); return q; };
    w.cOff = (u64*)take((N + 1) * 8); w.dOff = (u64*)take((N + 1) * 8); w.slot = (u64*)take(N * 8); w.runs = (u64*)take((N + 2) * 8);
    w.tileIdx = (u64*)take((T + 1) * 16); w.tileCover = (u64*)take((T + 1) * 8); w.tilePlan = (u64*)take((T + 1) * 32); w.sum = (u64*)take(kRgWords * 8);
    w.diff = (u32*)take((N + 1) * 4); w.decIdx = (u32*)take(N * 4);
    return w;
}

void launch_seek_index(const u8* tab, u64 tableBytes, u32 n, u32 stride, u64 srcSize, const RangesWs& ws, hipStream_t stream)
{
    const u32 T = n / kRangesTile + 1;          // (n + 1 items: the end marker gets the totals)
    hipLaunchKernelGGL(seek_index_sum_kernel, dim3(T), dim3(1024), 0, stream, tab, n, stride, ws.tileIdx);
    hipLaunchKernelGGL(tile_carry_kernel<2>, dim3(1), dim3(1024), 0, stream, ws.tileIdx, T);
    hipLaunchKernelGGL(seek_index_kernel, dim3(T), dim3(1024), 0, stream, tab, tableBytes, n, stride, srcSize, ws.tileIdx, T, ws);
}
void launch_ranges_select(const RangeIn* in, RangeRec* recs, u32 nRanges, u32 n, const RangesWs& ws, hipStream_t stream)
{
    hipLaunchKernelGGL(ranges_select_kernel, dim3((nRanges + 255) / 256), dim3(256), 0, stream, in, recs, nRanges, ws.dOff, n, ws.diff);
}
void launch_ranges_plan(const u8* tab, u32 n, u32 stride, u32 srcDev, const RangesWs& ws, BatchEntryIn* out, hipStream_t stream)
{
    const u32 T = n / kRangesTile + 1;
    hipLaunchKernelGGL(ranges_cover_sum_kernel, dim3(T), dim3(1024), 0, stream, ws.diff, n, ws.tileCover);
    hipLaunchKernelGGL(tile_carry_kernel<1>, dim3(1), dim3(1024), 0, stream, ws.tileCover, T);
    hipLaunchKernelGGL(ranges_plan_sum_kernel, dim3(T), dim3(1024), 0, stream, tab, n, stride, ws.diff, ws.tileCover, ws.tilePlan);
    hipLaunchKernelGGL(tile_carry_kernel<4>, dim3(1), dim3(1024), 0, stream, ws.tilePlan, T);
    hipLaunchKernelGGL(ranges_plan_kernel, dim3(T), dim3(1024), 0, stream, tab, n, stride, T, srcDev, ws, out);
}
void launch_ranges_alone(const BatchEntryOut* out, u32 nEntries, const RangesWs& ws, hipStream_t stream)
{
    hipLaunchKernelGGL(ranges_alone_kernel, dim3((nEntries + 255) / 256), dim3(256), 0, stream, out, nEntries, ws.sum);
}
void launch_ranges_gather(const RangeIn* in, const RangeRec* recs, u64* res, u32 nRanges, u32 nSlices, const RangesWs& ws, const BatchEntryOut* out,
                          const u8* arena, hipStream_t stream)
{
    const u32 most = 1u << 30;          // (a grid's x dimension ends below 2^31)
    for (u32 base = 0; base < nRanges; base += most) {
        const u32 count = nRanges - base < most ? nRanges - base : most;
        hipLaunchKernelGGL(ranges_gather_kernel, dim3(count, nSlices ? nSlices : 1), dim3(256), 0, stream, in + base, recs + base, res + base, ws.dOff, ws.slot,
                           ws.decIdx, out, arena);
    }
}

// an enqueued call (ZSTDMI_decompressRangesAsync): the select over the caller's arrays; the plan's scans as launch_ranges_plan runs them,
// then the emit into the decode core's nRows rows (the two verdict rows lie behind row nRows - 1 of `out`)
void launch_ranges_select_d(const unsigned long long* offsets, const size_t* lengths, void* const* dsts, const size_t* caps, u32 nRanges, u64 maxRangeBytes,
                            RangeIn* in, RangeRec* recs, u32 n, const RangesWs& ws, hipStream_t stream)
{
    hipLaunchKernelGGL(ranges_select_d_kernel, dim3((nRanges + 255) / 256), dim3(256), 0, stream, offsets, lengths, dsts, caps, nRanges, maxRangeBytes, in, recs,
                       ws.dOff, n, ws.diff);
}
void launch_ranges_plan_d(const u8* tab, u32 n, u32 stride, const RangesWs& ws, u64 streamOff, u64 arenaOff, u32 maxFrames, u64 maxContent, u64 aloneAbove,
                          u32 nRows, BatchEntryIn* rows, BatchEntryOut* out, hipStream_t stream)
{
    const u32 T = n / kRangesTile + 1;
    hipLaunchKernelGGL(ranges_cover_sum_kernel, dim3(T), dim3(1024), 0, stream, ws.diff, n, ws.tileCover);
    hipLaunchKernelGGL(tile_carry_kernel<1>, dim3(1), dim3(1024), 0, stream, ws.tileCover, T);
    hipLaunchKernelGGL(ranges_plan_sum_kernel, dim3(T), dim3(1024), 0, stream, tab, n, stride, ws.diff, ws.tileCover, ws.tilePlan);
    hipLaunchKernelGGL(tile_carry_kernel<4>, dim3(1), dim3(1024), 0, stream, ws.tilePlan, T);
    hipLaunchKernelGGL(ranges_plan_d_kernel, dim3(T), dim3(1024), 0, stream, tab, n, stride, T, ws, streamOff, arenaOff, maxFrames, maxContent, aloneAbove, nRows,
                       rows, out + nRows);
}

} // namespace zmi
