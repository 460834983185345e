// content_cuts_async.hip — the cuts and digests of a device buffer enqueued without a host round trip (ZSTDMI_contentCutsAsync; the
// rule: zmi_cuts.h; the selection: zmi_cut_rank.h).
//
// Behind launch_cut_count (content_cuts.hip: the candidates' count per tile, their scan and the total, as the synchronous call runs them):
//   cut_emit_bounded   cut_mark's emit pass with a limit: no store at or beyond maxCand.  The host never learns the total, so the list
//                      has the prepared room and a call with more candidates is refused on the device (every kernel below reads the
//                      total first and leaves when it passes the room; cuts_finish files workSpace_tooSmall)
//   cut_rank_init      one lane per node (the start, every candidate, the end): the candidate its piece would end at and the forced
//                      ends in front of it, by a lower bound in the sorted list and a jump over every bad zone it lands in
//   cut_rank_round     x cut_rank_rounds(most pieces): the nodes the walk from the start reaches, by pointer doubling.  A round is a
//                      launch: the pointers it reads were written by the launch before it, so no lane waits for another inside one
//   cut_rank_sum / _scan / _write   the exclusive scan of the reached nodes' end counts in list order (the path ascends in position, so
//                      that is the order of the ends); every reached node writes its forced run and its real end at its index, in
//                      cut_select's layout: count, then ends — launch_digest's `ends` form reads it as it stands
//   cuts_finish        ends -> sizes, sources, digests (copied from the workspace), *d_nPieces and *d_status, by the capacity rule
// Every grid is a function of the prepared limits and the call's srcSize; every count a kernel acts on is a device word held to the
// room its arrays have.
#include <hip/hip_runtime.h>
#include "zmi_common.h"
#include "zmi_device.h"
#include "zmi_host.h"
#include "zmi_cuts.h"
#include "zmi_cut_rank.h"

namespace zmi {

// ---- the bounded emit: cut_mark_kernel<true> (content_cuts.hip) with `room`.  That kernel and its helpers stay where the synchronous
// calls compile them, text and code object unchanged; the tile image, the roll and the block scan are restated here. ----
constexpr u32 kEmitSegs = kCutTile / 64 + 1;
__device__ __forceinline__ u32 emit_pad_word(u32 w) { return w + (w >> 4); }
__device__ __forceinline__ u32 emit_pad_byte(u32 i) { return i + ((i >> 6) << 2); }

// exclusive scan of the 256 lanes' v (all 256 threads call it, once per kernel: part is not reused)
__device__ __forceinline__ u32 rank_excl_scan256(u32 v, u32* part, u32* tot)
{
    const u32 lane = lane_id(), wave = wave_id();
    const u32 incl = wave_scan_incl(v);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    u32 before = 0;
    for (u32 w = 0; w < wave; ++w) before += part[w];
    *tot = part[0] + part[1] + part[2] + part[3];
    return before + incl - v;
}

template <bool MARK>
__device__ __forceinline__ u64 emit_roll(u64 h, const u32* seg, const u64* gear, u32 cnt, u32 bits, u64& mask)
{
#pragma unroll 4
    for (u32 j = 0; j < 16; ++j) {
        const u32 w = seg[j];
#pragma unroll
        for (u32 b = 0; b < 4; ++b) {
            h = (h << 1) + gear[(w >> (8 * b)) & 255u];
            if (MARK && 4 * j + b < cnt && cut_candidate(h, bits)) mask |= 1ull << (4 * j + b);
        }
    }
    return h;
}

__global__ __launch_bounds__(256) void cut_emit_bounded_kernel(const u8* __restrict__ src, u64 n, u32 bits, const u32* __restrict__ tileBase,
                                                               const u32* __restrict__ total, u32* __restrict__ cand, u32 room)
{
    __shared__ u64 gear[256];
    __shared__ u32 buf[kEmitSegs * 17];
    __shared__ u32 part[4];
    if (*total > room) return;                              // (uniform: the call is refused, the list is never read)
    const u32 tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * kCutTile;
    const u64 tEnd = (t0 + kCutTile) < n ? t0 + kCutTile : n;
    const u32 first = t0 ? 0u : 64u;                        // image bytes [first, last) are the source's [t0 - 64 + first, tEnd)
    const u32 last = 64u + (u32)(tEnd - t0);
    const u8* const at = src + t0;                          // image byte i is at[i - 64]
    gear[tid] = cut_gear(tid);
    if ((((uintptr_t)src) & 3u) == 0) {
        for (u32 w = tid; w < kEmitSegs * 16; w += 256) {
            const u32 i = 4 * w;
            if (i < first || i >= last) continue;
            if (i + 4 <= last) buf[emit_pad_word(w)] = *(const u32*)(at + (s64)i - 64);
            else for (u32 k = i; k < last; ++k) ((u8*)buf)[emit_pad_byte(k)] = at[(s64)k - 64];
        }
    } else {
        for (u32 i = first + tid; i < last; i += 256) ((u8*)buf)[emit_pad_byte(i)] = at[(s64)i - 64];
    }
    __syncthreads();
    const u64 p0 = t0 + (u64)tid * 64;
    u64 mask = 0;
    if (p0 < tEnd) {
        u64 h = 0, none = 0;
        if (p0) h = emit_roll<false>(h, buf + tid * 17, gear, 0, bits, none);
        const u32 cnt = (tEnd - p0) < 64 ? (u32)(tEnd - p0) : 64u;
        (void)emit_roll<true>(h, buf + (tid + 1) * 17, gear, cnt, bits, mask);
    }
    u32 tot;
    const u32 before = rank_excl_scan256(popc64(mask), part, &tot);
    u64 i = (u64)tileBase[blockIdx.x] + before;
    while (mask) { const u32 k = ctz64(mask); mask &= mask - 1; if (i < room) cand[i] = (u32)(p0 + k + 1); ++i; }
}

// ---- the selection ----
constexpr u32 kRankPer = 4, kRankTile = 256 * kRankPer;    // nodes per lane and per workgroup of the sum and write passes

__global__ __launch_bounds__(256) void cut_rank_init_kernel(const u32* __restrict__ cand, const u32* __restrict__ total, u32 room, u64 n, CutRule rule,
                                                            u32* __restrict__ succ, u32* __restrict__ forced, u8* __restrict__ mark)
{
    const u32 m = *total;
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (m > room || j > (u64)m + 1) return;
    u32 steps = 0;
    cut_rank_init(cand, m, n, rule, (u32)j, succ, forced, mark, steps);
}

// (mark is read and written by different lanes of one launch: no __restrict__, no const)
__global__ __launch_bounds__(256) void cut_rank_round_kernel(const u32* __restrict__ total, u32 room, const u32* __restrict__ in, u32* __restrict__ out, u8* mark)
{
    const u32 m = *total;
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (m > room || j > (u64)m + 1) return;
    cut_rank_round((u32)j, in, out, mark);
}

// the ends node j writes (0: none), its position
__device__ __forceinline__ u32 rank_node_weight(const u32* cand, u32 m, u64 n, const u32* forced, const u8* mark, u64 j, u64& pos)
{
    pos = 0;
    if (j > (u64)m + 1 || !mark[j]) return 0;
    pos = cut_node_pos(cand, m, n, (u32)j);
    return cut_rank_weight(true, pos, n, forced[j]);
}

__global__ __launch_bounds__(256) void cut_rank_sum_kernel(const u32* __restrict__ cand, const u32* __restrict__ total, u32 room, u64 n,
                                                           const u32* __restrict__ forced, const u8* __restrict__ mark, u32* __restrict__ blockSum)
{
    __shared__ u32 part[4];
    const u32 m = *total;
    if (m > room) return;                                   // (uniform; cut_rank_scan answers for the call)
    const u64 j0 = ((u64)blockIdx.x * 256 + threadIdx.x) * kRankPer;
    u32 w = 0;
    u64 pos;
#pragma unroll
    for (u32 k = 0; k < kRankPer; ++k) w += rank_node_weight(cand, m, n, forced, mark, j0 + k, pos);
    w = wave_sum(w);
    if (lane_id() == 0) part[wave_id()] = w;
    __syncthreads();
    if (threadIdx.x == 0) blockSum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// One workgroup: blockBase = the exclusive scan of blockSum[0 .. N); state[0] = the pieces, state[1] = the list passed its room;
// ends[0] = the pieces where the ends behind it can be trusted (at most cap of them), else 0
__global__ __launch_bounds__(1024) void cut_rank_scan_kernel(const u32* __restrict__ blockSum, u32* __restrict__ blockBase, u32 N, const u32* __restrict__ total, u32 room,
                                                             u32* __restrict__ state, u32* __restrict__ ends, u32 cap)
{
    __shared__ u32 part[1024];
    const u32 tid = threadIdx.x;
    if (*total > room) { if (tid == 0) { state[0] = 0; state[1] = 1; ends[0] = 0; } return; }
    const u32 per = (N + 1023) / 1024;
    const u64 a = (u64)tid * per, b = (a + per) < N ? a + per : N;
    u32 s = 0;
    for (u64 i = a; i < b; ++i) s += blockSum[i];
    part[tid] = s;
    __syncthreads();
    for (u32 d = 1; d < 1024; d <<= 1) { const u32 t = tid >= d ? part[tid - d] : 0u; __syncthreads(); part[tid] += t; __syncthreads(); }
    u32 run = part[tid] - s;
    for (u64 i = a; i < b; ++i) { const u32 v = blockSum[i]; blockBase[i] = run; run += v; }
    if (tid == 1023) { const u32 np = part[1023]; state[0] = np; state[1] = 0; ends[0] = np <= cap ? np : 0u; }
}

__device__ __forceinline__ u64 rank_read_lane64(u64 v, u32 l) { return (u64)read_lane((u32)v, l) | ((u64)read_lane((u32)(v >> 32), l) << 32); }

constexpr u32 kRankSerial = 4;      // a node with more ends than this hands them to its wave, 64 at a time (a desert's forced run)

__global__ __launch_bounds__(256) void cut_rank_write_kernel(const u32* __restrict__ cand, const u32* __restrict__ total, u32 room, u64 n, CutRule rule,
                                                             const u32* __restrict__ succ, const u32* __restrict__ forced, const u8* __restrict__ mark,
                                                             const u32* __restrict__ blockBase, u32* __restrict__ ends, u32 cap)
{
    __shared__ u32 part[4];
    const u32 m = *total;
    if (m > room) return;
    const u64 j0 = ((u64)blockIdx.x * 256 + threadIdx.x) * kRankPer;
    u32 w[kRankPer], sum = 0;
    u64 pos[kRankPer];
#pragma unroll
    for (u32 k = 0; k < kRankPer; ++k) { w[k] = rank_node_weight(cand, m, n, forced, mark, j0 + k, pos[k]); sum += w[k]; }
    u32 tot;
    u64 at = (u64)blockBase[blockIdx.x] + rank_excl_scan256(sum, part, &tot);
    const u32 lane = lane_id();
#pragma unroll
    for (u32 k = 0; k < kRankPer; ++k) {
        const u64 end = w[k] ? cut_node_pos(cand, m, n, succ[j0 + k]) : 0;
        const bool wide = w[k] > kRankSerial;
        if (w[k] && !wide) for (u32 x = 0; x < w[k]; ++x) if (at + x < cap) ends[1 + at + x] = cut_rank_end(pos[k], x, w[k] - 1, end, rule);
        for (u64 mb = ballot(wide); mb; mb &= mb - 1) {     // (every lane of the wave is here: none left above)
            const u32 l = ctz64(mb);
            const u64 bPos = rank_read_lane64(pos[k], l), bEnd = rank_read_lane64(end, l), bAt = rank_read_lane64(at, l);
            const u32 bW = read_lane(w[k], l);
            for (u32 x = lane; x < bW; x += 64) if (bAt + x < cap) ends[1 + bAt + x] = cut_rank_end(bPos, x, bW - 1, bEnd, rule);
        }
        at += w[k];
    }
}

// ---- what the caller gets ----
struct CutsFinish {
    const u32* ends; const u32* state; u32 endsCap; const u8* src; u64 n;
    size_t* sizes; const void** srcs; u64 capacity;
    const u8* digestsWs; u8* digests; u64 digestsCapacity; u32 digestSize;
    size_t* nPieces; size_t* status;
};
__global__ __launch_bounds__(256) void cuts_finish_kernel(const CutsFinish f)
{
    const u32 np = f.state[0];
    const bool over = f.state[1] != 0;
    // (np <= endsCap by the rule, cut_max_pieces; a count beyond it names ends that were never written)
    const u32 code = over ? (u32)kErrWorkSpaceTooSmall : np > f.endsCap ? (u32)kErrGeneric : ((u64)np > f.capacity || (u64)np * f.digestSize > f.digestsCapacity) ? (u32)kErrDstSizeTooSmall : 0u;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { *f.nPieces = np; *f.status = code ? (size_t)0 - (size_t)code : (size_t)0; }
    if (code || i >= np) return;
    const u32 s = i ? f.ends[i] : 0u, e = f.ends[i + 1];
    f.sizes[i] = (size_t)(e - s);
    if (f.srcs) f.srcs[i] = f.src + s;
    if (f.digestSize) {
        const u8* const from = f.digestsWs + i * f.digestSize;       // (the workspace's digests lie at multiples of 8)
        u8* const to = f.digests + i * f.digestSize;
        if (((uintptr_t)f.digests & 7u) == 0) for (u32 k = 0; k < f.digestSize; k += 8) *(u64*)(to + k) = *(const u64*)(from + k);
        else for (u32 k = 0; k < f.digestSize; ++k) to[k] = from[k];
    }
}
// an empty source: no piece, no array touched
__global__ void cuts_finish_empty_kernel(size_t* nPieces, size_t* status) { *nPieces = 0; *status = 0; }

// ---- host side ----
static u32 emit_tiles(u64 n) { return (u32)((n + kCutTile - 1) / kCutTile); }
static u32 blocks_of(u64 items, u32 per) { return (u32)((items + per - 1) / per); }

CutsAsyncLayout cuts_async_layout(u64 bound, u64 maxCand, u64 maxPieces, u32 digestSize)
{
    auto r = [](u64 x) { return (size_t)((x + 255) & ~(u64)255); };
    CutsAsyncLayout L;
    size_t at = 0;
    const u64 nodes = maxCand + 2, blocks = (nodes + kRankTile - 1) / kRankTile;
    L.atSmall = at; at += r(cut_small_bytes(bound));
    L.atList = at; at += r(4 * maxCand + 64);
    L.atSucc = at; at += r(4 * nodes);
    L.atJumpA = at; at += r(4 * nodes);
    L.atJumpB = at; at += r(4 * nodes);
    L.atForced = at; at += r(4 * nodes);
    L.atMark = at; at += r(nodes);
    L.atSum = at; at += r(4 * (blocks + 16));
    L.atBase = at; at += r(4 * (blocks + 16));
    L.atState = at; at += 256;
    L.atEnds = at; at += r(4 * (maxPieces + 1));
    L.atDigests = at; at += r(maxPieces * digestSize);
    L.bytes = at;
    return L;
}

void launch_cut_emit_bounded(const u8* src, u64 n, u32 bits, u8* small, u32* cand, u32 room, hipStream_t stream)
{
    const u32 nTiles = emit_tiles(n);
    const u32* tileBase = (const u32*)small + nTiles + 16;
    hipLaunchKernelGGL(cut_emit_bounded_kernel, dim3(nTiles), dim3(256), 0, stream, src, n, bits, tileBase, cut_total_word(small, n), cand, room);
}

// the selection over a list of *total candidates (a device word; more than room: nothing is read, state says so) of a source of n bytes:
// ends[0] = the pieces, ends[1 ..] their ends (at most cap).  Grids: the nodes room and n allow; rounds: the pieces n allows.
void launch_cut_rank(const u32* cand, const u32* total, u32 room, u64 n, const CutRule& rule, const CutRankWs& ws, u32* ends, u32 cap, hipStream_t stream)
{
    const u64 nodes = ((u64)room < n ? (u64)room : n) + 2;
    const u32 gNode = blocks_of(nodes, 256), gTile = blocks_of(nodes, kRankTile);
    hipLaunchKernelGGL(cut_rank_init_kernel, dim3(gNode), dim3(256), 0, stream, cand, total, room, n, rule, ws.succ, ws.forced, ws.mark);
    const u32 rounds = cut_rank_rounds(cut_max_pieces(n, rule));
    const u32* in = ws.succ; u32* out = ws.jumpA;
    for (u32 k = 0; k < rounds; ++k) {
        hipLaunchKernelGGL(cut_rank_round_kernel, dim3(gNode), dim3(256), 0, stream, total, room, in, out, ws.mark);
        in = out; out = out == ws.jumpA ? ws.jumpB : ws.jumpA;
    }
    hipLaunchKernelGGL(cut_rank_sum_kernel, dim3(gTile), dim3(256), 0, stream, cand, total, room, n, ws.forced, ws.mark, ws.blockSum);
    hipLaunchKernelGGL(cut_rank_scan_kernel, dim3(1), dim3(1024), 0, stream, ws.blockSum, ws.blockBase, gTile, total, room, ws.state, ends, cap);
    hipLaunchKernelGGL(cut_rank_write_kernel, dim3(gTile), dim3(256), 0, stream, cand, total, room, n, rule, ws.succ, ws.forced, ws.mark, ws.blockBase, ends, cap);
}

void launch_cuts_finish(const CutsFinishArgs& a, hipStream_t stream)
{
    if (!a.n) { hipLaunchKernelGGL(cuts_finish_empty_kernel, dim3(1), dim3(1), 0, stream, a.nPieces, a.status); return; }
    const CutsFinish f = { a.ends, a.state, a.endsCap, a.src, a.n, a.sizes, a.srcs, a.capacity, a.digestsWs, a.digests, a.digestsCapacity, a.digestSize, a.nPieces, a.status };
    hipLaunchKernelGGL(cuts_finish_kernel, dim3(blocks_of(a.maxPieces, 256)), dim3(256), 0, stream, f);
}

} // namespace zmi
