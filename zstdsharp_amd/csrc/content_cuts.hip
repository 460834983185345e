// content_cuts.hip — where a call's pieces end, from the content alone (ZSTDMI_CCtx_setContentCuts; the rule: zmi_cuts.h).
//
// Runs once per call in front of the pack's rounds (compress_cut, zstd_mi355x.hip):
//   cut_mark (count)   one workgroup per 16 KiB tile: the tile and the 64 bytes in front of it in LDS, the gear table in LDS; every lane
//                      rolls the hash over its 64 positions behind a warm-up over the 64 bytes in front of them and keeps the candidate
//                      ends among them as one 64-bit mask; one count per tile
//   cut_scan           the tiles' first candidate index (the host reads the total back and sizes the list)
//   cut_mark (emit)    the same pass again; the candidate ends go out in position order, one u32 each
//   cut_select         one wave walks the list by the rule (cut_walk) and writes the piece ends and their count
// Unlike ldm_split there is no cap on candidates per lane and no second hash of a window: a mark pass reads the source once.
// Every step is a function of the source's bytes and avgLog alone.
#include <hip/hip_runtime.h>
#include "zmi_common.h"
#include "zmi_device.h"
#include "zmi_host.h"
#include "zmi_cuts.h"

namespace zmi {

// LDS image of a tile: segment g = 64 bytes = 16 words at word 17 g (one word of padding: the lanes' segments start in different
// banks); segment 0 is the 64 bytes in front of the tile, segment 1 + l lane l's positions
constexpr u32 kCutSegs = kCutTile / 64 + 1;
__device__ __forceinline__ u32 cut_pad_word(u32 w) { return w + (w >> 4); }
__device__ __forceinline__ u32 cut_pad_byte(u32 i) { return i + ((i >> 6) << 2); }

// exclusive scan of the 256 lanes' v (all 256 threads call it); the total in *tot
__device__ __forceinline__ u32 cut_excl_scan256(u32 v, u32* part, u32* tot)
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

// h over one segment's words: 64 steps of h = (h << 1) + gear[byte], the candidates among the first cnt of them into mask
template <bool MARK>
__device__ __forceinline__ u64 cut_roll(u64 h, const u32* seg, const u64* gear, u32 cnt, u32 bits, u64& mask)
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

template <bool EMIT>
__global__ __launch_bounds__(256) void cut_mark_kernel(const u8* __restrict__ src, u64 n, u32 bits, u32* __restrict__ tileCount,
                                                       const u32* __restrict__ tileBase, u32* __restrict__ cand)
{
    __shared__ u64 gear[256];
    __shared__ u32 buf[kCutSegs * 17];
    __shared__ u32 part[4];
    const u32 tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * kCutTile;
    const u64 tEnd = (t0 + kCutTile) < n ? t0 + kCutTile : n;
    const u32 first = t0 ? 0u : 64u;                        // image bytes [first, last) are the source's [t0 - 64 + first, tEnd)
    const u32 last = 64u + (u32)(tEnd - t0);
    const u8* const at = src + t0;                          // image byte i is at[i - 64]
    gear[tid] = cut_gear(tid);
    if ((((uintptr_t)src) & 3u) == 0) {
        // whole words where all four bytes are the source's, bytes at the source's end
        for (u32 w = tid; w < kCutSegs * 16; w += 256) {
            const u32 i = 4 * w;
            if (i < first || i >= last) continue;
            if (i + 4 <= last) buf[cut_pad_word(w)] = *(const u32*)(at + (s64)i - 64);
            else for (u32 k = i; k < last; ++k) ((u8*)buf)[cut_pad_byte(k)] = at[(s64)k - 64];
        }
    } else {
        for (u32 i = first + tid; i < last; i += 256) ((u8*)buf)[cut_pad_byte(i)] = at[(s64)i - 64];
    }
    __syncthreads();
    const u64 p0 = t0 + (u64)tid * 64;
    u64 mask = 0;
    if (p0 < tEnd) {
        u64 h = 0, none = 0;
        if (p0) h = cut_roll<false>(h, buf + tid * 17, gear, 0, bits, none);        // warm-up: the 64 bytes in front of p0
        const u32 cnt = (tEnd - p0) < 64 ? (u32)(tEnd - p0) : 64u;
        (void)cut_roll<true>(h, buf + (tid + 1) * 17, gear, cnt, bits, mask);       // (bytes behind cnt are not the source's: never marked)
    }
    u32 tot;
    const u32 before = cut_excl_scan256(popc64(mask), part, &tot);
    if (!EMIT) { if (tid == 0) tileCount[blockIdx.x] = tot; return; }
    u32 i = tileBase[blockIdx.x] + before;
    while (mask) { const u32 k = ctz64(mask); mask &= mask - 1; cand[i++] = (u32)(p0 + k + 1); }
}

// exclusive scan of in[0 .. N) into out, total -> *total; one workgroup.  (ldm_scan_kernel's form, and cut_excl_scan256 above is
// ldm.hip's block scan: a kernel of another translation unit cannot be launched from here without relocatable device code, and
// ldm.hip stays as it is.)
__global__ __launch_bounds__(1024) void cut_scan_kernel(const u32* __restrict__ in, u32* __restrict__ out, u32 N, u32* __restrict__ total)
{
    __shared__ u32 part[1024];
    const u32 tid = threadIdx.x, per = (N + 1023) / 1024;
    const u64 a = (u64)tid * per, b = (a + per) < N ? a + per : N;
    u32 s = 0;
    for (u64 i = a; i < b; ++i) s += in[i];
    part[tid] = s;
    __syncthreads();
    for (u32 d = 1; d < 1024; d <<= 1) { const u32 t = tid >= d ? part[tid - d] : 0u; __syncthreads(); part[tid] += t; __syncthreads(); }
    u32 run = part[tid] - s;
    for (u64 i = a; i < b; ++i) { const u32 v = in[i]; out[i] = run; run += v; }
    if (tid == 1023) *total = part[1023];
}

// One wave.  The list goes through LDS in blocks of kCutListBlock candidates (coalesced loads: a piece costs LDS latency, not a
// dependent global load); the next candidate at or behind s + min is found by a ballot over 64 list entries at a time; the forced cuts
// of a stretch without a usable candidate are written by the lanes side by side.  Every value of the walk is uniform across the wave.
// out[0] = the pieces, out[1 ..] their ends (at most cap of them are written).
__global__ __launch_bounds__(64) void cut_select_kernel(const u32* __restrict__ cand, u32 nCand, u64 n, CutRule rule, u32* __restrict__ out, u32 cap)
{
    __shared__ u32 blk[kCutListBlock];
    const u32 lane = lane_id();
    u32 idx = 0, base = 0, lim = 0;         // the list's entries [base, lim) are in blk; idx: the first entry not yet passed
    u32 win = 0, winEnd = 0, v = 0;         // a window of the block in registers: lane l holds entry win + l, 0 at or behind winEnd
    u32 np = 0;
    // Entries in front of idx lie below every later target, and a lane without an entry holds 0, below every target: one compare and
    // one ballot over the window find the next candidate, and a piece costs no LDS read while its candidate lies in the window.
    auto next = [&](u32 target, u32& c) -> bool {
        while (idx < nCand) {
            if (idx >= winEnd) {
                if (idx >= lim) {           // (idx == lim, a multiple of the block)
                    wave_lds_sync();
                    base = idx; lim = (nCand - base) < kCutListBlock ? nCand : base + kCutListBlock;
                    u32 t[kCutListBlock / 64];  // (all loads in flight before the first LDS write: one global latency per block)
#pragma unroll
                    for (u32 k = 0; k < kCutListBlock / 64; ++k) { const u32 i = k * 64 + lane; t[k] = i < lim - base ? cand[base + i] : 0u; }
#pragma unroll
                    for (u32 k = 0; k < kCutListBlock / 64; ++k) blk[k * 64 + lane] = t[k];
                    wave_lds_sync();
                }
                win = idx; winEnd = (lim - win) < 64 ? lim : win + 64;
                v = win + lane < winEnd ? blk[win + lane - base] : 0u;
            }
            const u64 m = ballot(v >= target);
            if (m) { const u32 l = ctz64(m); idx = win + l; c = read_lane(v, l); return true; }
            idx = winEnd;
        }
        return false;
    };
    // (np + count <= cap by the rule: cut_max_pieces; the compare keeps a wrong list from writing past the buffer)
    auto run = [&](u32 first, u32 step, u32 count) {
        if (count == 1) { if (lane == 0 && np < cap) out[1 + np] = first; }
        else for (u32 j = lane; j < count; j += 64) if (np + j < cap) out[1 + np + j] = first + j * step;
        np += count;
    };
    const u32 pieces = cut_walk<u32>((u32)n, rule, next, run);      // (n <= kCutMaxSrc: the host's check)
    if (lane == 0) out[0] = pieces;
}

// ---- host side ----
// tileCount[nTiles + 16] | tileBase[nTiles + 16] | total
static u32 cut_tiles(u64 n) { return (u32)((n + kCutTile - 1) / kCutTile); }
size_t cut_small_bytes(u64 n) { return ((size_t)cut_tiles(n) + 16) * sizeof(u32) * 2 + 256; }
u32* cut_total_word(u8* small, u64 n) { return (u32*)small + 2 * ((size_t)cut_tiles(n) + 16); }
// count the candidates of [src, src + n), 0 < n <= kCutMaxSrc: -> the device word cut_total_word
void launch_cut_count(const u8* src, u64 n, u32 bits, u8* small, hipStream_t stream)
{
    const u32 nTiles = cut_tiles(n);
    u32* tileCount = (u32*)small; u32* tileBase = tileCount + nTiles + 16;
    hipLaunchKernelGGL(cut_mark_kernel<false>, dim3(nTiles), dim3(256), 0, stream, src, n, bits, tileCount, nullptr, nullptr);
    hipLaunchKernelGGL(cut_scan_kernel, dim3(1), dim3(1024), 0, stream, tileCount, tileBase, nTiles, cut_total_word(small, n));
}
// the candidates in position order into cand (room for the total the count gave)
void launch_cut_emit(const u8* src, u64 n, u32 bits, u8* small, u32* cand, hipStream_t stream)
{
    const u32 nTiles = cut_tiles(n);
    const u32* tileBase = (const u32*)small + nTiles + 16;
    hipLaunchKernelGGL(cut_mark_kernel<true>, dim3(nTiles), dim3(256), 0, stream, src, n, bits, nullptr, tileBase, cand);
}
// out: 1 + cap words
void launch_cut_select(const u32* cand, u32 nCand, u64 n, const CutRule& rule, u32* out, u32 cap, hipStream_t stream)
{
    hipLaunchKernelGGL(cut_select_kernel, dim3(1), dim3(64), 0, stream, cand, nCand, n, rule, out, cap);
}

} // namespace zmi
