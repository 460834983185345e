// ldm.hip — long-distance matching (ZSTD_c_enableLongDistanceMatching; the reference's ZSTD_ldm_generateSequences, U/ZstdLdm.cs).
//
// Runs once per pass between the block match finder (launch_lz) and the entropy stages, over the whole pass at once:
//   ldm_split  (count)  a gear rolling hash marks the split points of every 16 KiB tile; one count per tile
//   ldm_scan            the tiles' first split index (the host reads the total back and sizes the workspace)
//   ldm_split  (emit)   the splits in position order: window start, 32-bit checksum, sort key (frame, bucket)
//   ldm_radix_*         a stable LSD radix sort of the splits by key: a bucket's splits end up side by side in position order
//   ldm_inv             split -> its place in the sorted order
//   ldm_match           one wave per block: each split's candidates are the (1 << bucketSizeLog) splits in front of it in its
//                       bucket (what the reference's round-robin bucket holds when it looks); verified by bytes, the longest kept,
//                       then walked greedily with an anchor as the reference's loop does
//   ldm_merge           one wave per block that has LDM matches: the finder's sequences are trimmed around them and the block's
//                       sequence store (seqs / lits / ChunkMeta) is rewritten in place
// Every step is a function of the pass's bytes alone (no insert-order-dependent table): the output does not depend on scheduling.
//
// A referenced prefix (ZSTD_CCtx_refPrefix; the PFX instances of ldm_split and ldm_match): prefix and source lie in different buffers
// and are ONE window.  Positions are virtual: the source's byte i is at base + i with base = the prefix length rounded up to a split
// tile, the prefix's byte i at vlo + i with vlo = base - prefixLen, and nothing lies below vlo.  The prefix so ends exactly where
// block 0 of the source begins: position - candidate is the zstd offset, the source's tiles and blocks keep their alignment, and no
// tile straddles the seam.  Splits are taken over [vlo, end) — the rolling hash and a split's window run across the seam —, the
// prefix's sort in front of the source's, and only the source's blocks are matched: the prefix's splits are candidates only.
// A window that slides with ONE frame (ZSTDMI_CCtx_setSlidingLdm; the WIN instance of ldm_match): the same coordinate, with the frame's
// own content in front of the pass — up to 2^windowLog bytes of it, in the same buffer — in the prefix's place, and a distance bound,
// because such a pass may be longer than its window.
#include <hip/hip_runtime.h>
#include "zmi_common.h"
#include "zmi_device.h"
#include "zmi_host.h"

namespace zmi {

constexpr u32 kLdmTile = 16384;         // bytes per workgroup of the split kernels (256 lanes x 64 positions); a frame may start inside one
constexpr u32 kLdmSegCap = 4;           // splits kept per 64 positions (the first four): the workspace holds at most one per 16 bytes
constexpr u32 kSortTile = 4096;         // elements per workgroup of the radix sort (16 rounds of 256)
static_assert(kLdmPrefixAlign == kLdmTile, "a referenced prefix ends on a tile boundary of the virtual coordinate");

// The gear table: splitmix64 of 0 .. 255 (the reference's table is another set of random constants; any fixed one serves)
__device__ __forceinline__ u64 splitmix64(u64 i)
{
    u64 z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// 64-bit hash of a split's window (its first min(minMatch, 64) bytes; a match is verified by bytes anyway): FNV-1a + fmix64.
// Bytes from the workgroup's LDS copy of the tile (i -> index of byte i), or from global memory for a window that starts in front of it.
template <class At>
__device__ __forceinline__ u64 window_hash(At at, u32 len)
{
    u64 x = 0xCBF29CE484222325ull ^ len;
    for (u32 i = 0; i < len; ++i) x = (x ^ at(i)) * 0x100000001B3ull;
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}

__device__ __forceinline__ u32 ldm_pad(u32 i) { return i + ((i >> 6) << 2); }

// exclusive scan of the 256 lanes' v (all 256 threads call it); returns the total in *tot
__device__ __forceinline__ u32 block_excl_scan256(u32 v, u32* part, u32* tot)
{
    const u32 lane = lane_id(), wave = wave_id();
    const u32 incl = wave_scan_incl(v);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    u32 before = 0;
    for (u32 w = 0; w < wave; ++w) before += part[w];
    *tot = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
    return before + incl - v;
}

// Split points (ZSTD_ldm_gear_feed): after byte p, h = (h << 1) + gear[byte]; a split ends at p + 1 when (h & stopMask) == 0.  Bit k
// of h depends on the last k + 1 bytes only and stopMask lies below bit 64, so every lane starts 64 bytes ahead of its 64 positions
// (never before its frame's start, where h is 0).  A split's window [p + 1 - minMatch, p + 1) must lie in the frame.  The default
// blocks (64, 48, 32 KiB) make a frame span a multiple of the tile; ZSTDMI_CCtx_setHistory can make it any multiple of 4 KiB, so the
// frame is taken per lane and per position, not per tile.  Only the first kLdmSegCap splits of a lane's 64 positions are kept.
// PFX: n, the tiles and every position are virtual (see the head of the file); the one frame starts at pfx.vlo.
template <bool EMIT, bool PFX>
__global__ __launch_bounds__(256) void ldm_split_kernel(const u8* __restrict__ src, u64 n, u64 frameSpan, u32 minMatch, u64 stopMask, u32 hb, const LdmPrefix pfx,
                                                        u32* __restrict__ tileCount, const u32* __restrict__ tileBase,
                                                        u32* __restrict__ splitPos, u32* __restrict__ splitCheck, u64* __restrict__ key, u32* __restrict__ val)
{
    __shared__ u64 gear[256];
    __shared__ u8 buf[(kLdmTile + 64) / 64 * 68];     // 4 bytes of padding behind every 64: the lanes' segments fall in different banks
    __shared__ u32 part[4];
    const u32 tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * kLdmTile;
    const u64 tEnd = (t0 + kLdmTile) < n ? t0 + kLdmTile : n;
    auto byteAt = [&](u64 v) -> u32 { if (PFX) return v < pfx.base ? pfx.pre[v - pfx.vlo] : src[v - pfx.base]; return src[v]; };
    const u64 fStart = PFX ? (u64)pfx.vlo : t0 / frameSpan * frameSpan;
    const u64 lo = t0 >= fStart + 64 ? t0 - 64 : fStart;
    gear[tid] = splitmix64(tid);
    const u32 pre = (u32)(t0 - lo), len = pre + (u32)(tEnd - t0);      // (PFX, the first tile: lo = vlo lies behind t0, pre wraps, the sums hold)
    for (u32 i = tid; i < len; i += 256) buf[ldm_pad(64 - pre + i)] = (u8)byteAt(lo + i);
    __syncthreads();
    const u64 p0 = t0 + (u64)tid * 64;
    const u32 mm = minMatch < 64 ? minMatch : 64;
    u32 found = 0, base = 0;
    for (int pass = 0; pass < (EMIT ? 2 : 1); ++pass) {
        if (pass == 1) {
            u32 tot;
            base = tileBase[blockIdx.x] + block_excl_scan256(found, part, &tot);
            found = 0;
        }
        if (p0 < tEnd) {
            u64 h = 0;
            // the frame of this lane's positions: a frame span need not be a multiple of the tile (nor of 64), so it is the lane's
            // own, and it moves on where a frame starts among the lane's 64 positions (the hash starts from 0 there)
            u64 fS = PFX ? fStart : p0 / frameSpan * frameSpan;
            const u64 wlo = p0 >= fS + 64 ? p0 - 64 : fS;
            for (u64 q = wlo; q < p0; ++q) h = (h << 1) + gear[buf[ldm_pad((u32)(64 + (s64)(q - t0)))]];
            const u32 cnt = (tEnd - p0) < 64 ? (u32)(tEnd - p0) : 64u;
            const u32 k0 = (PFX && p0 < fStart) ? ((fStart - p0) < 64 ? (u32)(fStart - p0) : 64u) : 0u;      // (nothing lies in front of the prefix)
            for (u32 k = k0; k < cnt && found < kLdmSegCap; ++k) {
                const u64 p = p0 + k;
                if (!PFX && p == fS + frameSpan) { fS = p; h = 0; }
                h = (h << 1) + gear[buf[ldm_pad(64 + tid * 64 + k)]];
                if ((h & stopMask) == 0 && p + 1 >= fS + minMatch) {
                    if (pass == 1) {
                        const u32 w = (u32)(p + 1 - minMatch), i = base + found;
                        const u64 x = w >= lo ? window_hash([&](u32 j) { return (u32)buf[ldm_pad((u32)(64 + (s64)(w + j - t0)))]; }, mm)
                                              : window_hash([&](u32 j) { return byteAt((u64)w + j); }, mm);
                        splitPos[i] = w; splitCheck[i] = (u32)(x >> 32);
                        key[i] = ((u64)(PFX ? 0u : w / frameSpan) << hb) | (x & ((1ull << hb) - 1)); val[i] = i;
                    }
                    found++;
                }
            }
        }
    }
    if (!EMIT) { u32 tot; block_excl_scan256(found, part, &tot); if (tid == 0) tileCount[blockIdx.x] = tot; }
}

// exclusive scan of in[0 .. N) into out (may be in), total -> *total; one workgroup (tile counts, radix histograms)
__global__ __launch_bounds__(1024) void ldm_scan_kernel(const u32* in, u32* out, u32 N, u32* total)
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
    if (tid == 1023 && total) *total = part[1023];
}

// radix sort, 8 bits a pass: per-tile digit histograms (LDS, one global write per digit and tile) -> scan (digit-major) -> scatter
__global__ __launch_bounds__(256) void ldm_radix_hist_kernel(const u64* __restrict__ key, u32 n, u32 shift, u32* __restrict__ hist, u32 nTiles)
{
    __shared__ u32 h[256];
    const u32 tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const u32 base = blockIdx.x * kSortTile;
    for (u32 i = tid; i < kSortTile; i += 256) { const u32 e = base + i; if (e < n) atomicAdd(&h[(u32)(key[e] >> shift) & 255u], 1u); }
    __syncthreads();
    hist[tid * nTiles + blockIdx.x] = h[tid];
}
// stable: a tile's elements are taken 256 at a time in order; inside a round, rank = same-digit lanes in front (8 ballots per wave)
__global__ __launch_bounds__(256) void ldm_radix_scatter_kernel(const u64* __restrict__ keyIn, const u32* __restrict__ valIn, u64* __restrict__ keyOut,
                                                                u32* __restrict__ valOut, u32 n, u32 shift, const u32* __restrict__ histScan, u32 nTiles)
{
    __shared__ u32 run[256];
    __shared__ u32 wcnt[4][256];
    const u32 tid = threadIdx.x, wave = wave_id();
    run[tid] = histScan[tid * nTiles + blockIdx.x];
    const u32 base = blockIdx.x * kSortTile;
    for (u32 r = 0; r < kSortTile && base + r < n; r += 256) {
        for (u32 w = 0; w < 4; ++w) wcnt[w][tid] = 0;
        __syncthreads();
        const u32 e = base + r + tid;
        const bool valid = e < n;
        const u64 k = valid ? keyIn[e] : 0;
        const u32 v = valid ? valIn[e] : 0;
        const u32 d = (u32)(k >> shift) & 255u;
        u64 m = __ballot(valid);
        for (u32 b = 0; b < 8; ++b) { const bool bit = (d >> b) & 1u; const u64 bb = __ballot(bit); m &= bit ? bb : ~bb; }
        const u32 rank = (u32)__popcll(m & lanemask_lt());
        if (valid && rank == 0) wcnt[wave][d] = (u32)__popcll(m);
        __syncthreads();
        if (valid) {
            u32 pos = run[d] + rank;
            for (u32 w = 0; w < wave; ++w) pos += wcnt[w][d];
            keyOut[pos] = k; valOut[pos] = v;
        }
        __syncthreads();
        run[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void ldm_inv_kernel(const u32* __restrict__ sortedVal, u32* __restrict__ inv, u32 n)
{
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) inv[sortedVal[j]] = j;
}

// first index i in [0, n) with a[i] >= x (uniform)
__device__ __forceinline__ u32 lower_bound_u32(const u32* a, u32 n, u32 x)
{
    u32 lo = 0, hi = n;
    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
// bytes a[i] == b[i] from i = 0 on, at most limit (whole wave, uniform result)
__device__ __forceinline__ u32 wave_match_fwd(const u8* a, const u8* b, u32 limit)
{
    const u32 lane = lane_id();
    for (u32 len = 0; len < limit; len += 256) {
        const u32 i = len + lane * 4;
        u32 mm = 4;
        for (u32 k = 0; k < 4; ++k) if (i + k >= limit || a[i + k] != b[i + k]) { mm = k; break; }
        const u64 bad = __ballot(mm < 4);
        if (bad) { const u32 l = (u32)__ffsll((long long)bad) - 1; const u32 r = len + l * 4 + read_lane(mm, l); return r < limit ? r : limit; }
    }
    return limit;
}
// bytes a[-1 - i] == b[-1 - i] from i = 0 on, at most limit
__device__ __forceinline__ u32 wave_match_back(const u8* a, const u8* b, u32 limit)
{
    const u32 lane = lane_id();
    for (u32 len = 0; len < limit; len += 256) {
        const u32 i = len + lane * 4;
        u32 mm = 4;
        for (u32 k = 0; k < 4; ++k) if (i + k >= limit || a[-1 - (s64)(i + k)] != b[-1 - (s64)(i + k)]) { mm = k; break; }
        const u64 bad = __ballot(mm < 4);
        if (bad) { const u32 l = (u32)__ffsll((long long)bad) - 1; const u32 r = len + l * 4 + read_lane(mm, l); return r < limit ? r : limit; }
    }
    return limit;
}

// One wave per block.  For every split whose window lies in the block: its candidates (bucket neighbours in front of it with the
// same checksum) are looked up by the lanes side by side; the splits that have any are then taken one after the other by the whole
// wave, left to right, as ZSTD_ldm_generateSequences_internal does: a split in front of the anchor is skipped, every candidate is
// extended forward (to the block's end) and backward (to the anchor, and not before its frame), the longest total whose forward part
// reaches minMatch wins, and the anchor moves behind it.  Result per split: mLen (0 = none), mStart (pass offset), mOff.
// PFX: positions are virtual and the blocks are the source's (block c starts at pfx.base + c * chunkBytes).  The split's own side of
// a compare always lies in the source; the candidate's side is read in two segments: a forward compare that starts in the prefix
// runs on into the source, a backward one that starts in the source runs back into the prefix and stops at the prefix's first byte.
// Either is cut at the seam into two wave compares of 256 bytes a step, the second only when the first matched to its end.
// WIN (a window that slides with its frame, ZSTDMI_CCtx_setSlidingLdm; with PFX): what lies in front of the source is the frame's own
// content, up to pfx.maxDist = 2^windowLog bytes of it, and the source may be longer than that, so the index holds splits further back
// than a position may reach: a candidate more than pfx.maxDist behind its split is passed over (a match keeps its candidate's
// distance when it is extended, so no offset exceeds the window).
template <bool PFX, bool WIN = false>
__global__ __launch_bounds__(256) void ldm_match_kernel(const u8* __restrict__ src, u64 n, u32 nChunks, u32 chunkBytes, u64 frameSpan, u32 minMatch, u32 bucketLog, const LdmPrefix pfx,
                                                        const u32* __restrict__ splitPos, const u32* __restrict__ splitCheck, const u64* __restrict__ sortedKey,
                                                        const u32* __restrict__ sortedVal, const u32* __restrict__ inv, u32 nSplits,
                                                        u32* __restrict__ mStart, u32* __restrict__ mLen, u32* __restrict__ mOff)
{
    const u32 lane = lane_id();
    const u32 c = blockIdx.x * 4 + wave_id();
    if (c >= nChunks) return;
    const u64 bStart = (PFX ? (u64)pfx.base : 0u) + (u64)c * chunkBytes, bEnd = (bStart + chunkBytes) < n ? bStart + chunkBytes : n;
    const u64 fStart = PFX ? (u64)pfx.vlo : bStart / frameSpan * frameSpan;
    const u32 s0 = lower_bound_u32(splitPos, nSplits, (u32)bStart), s1 = lower_bound_u32(splitPos, nSplits, (u32)bEnd);
    const u32 ents = 1u << bucketLog;
    const u8* const vsrc = PFX ? src - pfx.base : src;      // virtual position -> source byte (positions >= base only)
    u32 anchor = (u32)bStart;
    for (u32 sb = s0; sb < s1; sb += 64) {
        const u32 s = sb + lane;
        bool has = false;
        u32 myStart = 0, myLen = 0, myOff = 0;      // this lane's split's result (each lane writes its own)
        if (s < s1) {
            const u32 w = splitPos[s];
            if ((u64)w + minMatch <= bEnd) {
                const u32 j = inv[s]; const u64 k = sortedKey[j]; const u32 cs = splitCheck[s];
                for (u32 i = 1; i <= ents && i <= j; ++i) {
                    if (sortedKey[j - i] != k) break;
                    if (WIN && w - splitPos[sortedVal[j - i]] > pfx.maxDist) break;      // (a bucket's splits lie in position order: the rest is further back)
                    if (splitCheck[sortedVal[j - i]] == cs) { has = true; break; }
                }
            }
        }
        u64 todo = __ballot(has);
        while (todo) {
            const u32 l = (u32)__ffsll((long long)todo) - 1; todo &= todo - 1;
            const u32 sl = sb + l, w = splitPos[sl];
            if (w < anchor) continue;
            const u32 j = inv[sl]; const u64 k = sortedKey[j]; const u32 cs = splitCheck[sl];
            u32 bestLen = 0, bestBack = 0, bestFwd = 0, bestOff = 0;
            for (u32 i = 1; i <= ents && i <= j; ++i) {
                if (sortedKey[j - i] != k) break;
                const u32 t = sortedVal[j - i];
                if (splitCheck[t] != cs) continue;
                const u32 cw = splitPos[t];
                if (WIN && w - cw > pfx.maxDist) break;
                const u32 fwdLim = (u32)(bEnd - w);
                u32 fwd;
                if (PFX && cw < pfx.base) {
                    const u32 seg = pfx.base - cw;      // the candidate's bytes in front of the seam
                    fwd = wave_match_fwd(vsrc + w, pfx.pre + (cw - pfx.vlo), fwdLim < seg ? fwdLim : seg);
                    if (fwd == seg && fwdLim > seg) fwd += wave_match_fwd(vsrc + w + seg, src, fwdLim - seg);
                } else fwd = wave_match_fwd(vsrc + w, vsrc + cw, fwdLim);
                if (fwd < minMatch) continue;
                const u32 backLim = (w - anchor) < (u32)(cw - fStart) ? (w - anchor) : (u32)(cw - fStart);
                u32 back;
                if (PFX && cw < pfx.base) back = wave_match_back(vsrc + w, pfx.pre + (cw - pfx.vlo), backLim);
                else if (PFX && backLim > cw - pfx.base) {
                    const u32 seg = cw - pfx.base;      // the candidate's bytes behind the seam
                    back = wave_match_back(vsrc + w, vsrc + cw, seg);
                    if (back == seg) back += wave_match_back(vsrc + w - seg, pfx.pre + (pfx.base - pfx.vlo), backLim - seg);
                } else back = wave_match_back(vsrc + w, vsrc + cw, backLim);
                if (fwd + back > bestLen) { bestLen = fwd + back; bestBack = back; bestFwd = fwd; bestOff = w - cw; }
            }
            if (bestLen) {
                if (lane == l) { myStart = w - bestBack; myLen = bestLen; myOff = bestOff; }
                anchor = w + bestFwd;
            }
        }
        if (s < s1) { mStart[s] = myStart; mLen[s] = myLen; mOff[s] = myOff; }
    }
}

// One wave per block (persistent: wave g takes blocks g, g + nWaves, ...), blocks without LDM matches untouched.  The finder's
// matches and the block's LDM matches are merged left to right with every value uniform across the wave (64 of each are loaded at a
// time, one per lane, and read with readlane): an LDM match is taken whole; a finder match that overlaps one keeps its uncovered
// pieces with its own offset, and a piece shorter than 4 bytes becomes literals (every sequence still consumes >= 4 bytes: kMaxSeq
// holds).  The sequences go 64 at a time through LDS to the wave's scratch, each lane copying its sequence's literals from src;
// then the scratch replaces the block's sequences.  Offsets stay raw (distance + 3): seq_encode resolves repcodes.
struct StagedSeq { u32 litSrc, litDst; Seq q; };
__global__ __launch_bounds__(256) void ldm_merge_kernel(const u8* __restrict__ src, u64 n, u32 nChunks, u32 chunkBytes, u32 base, const u32* __restrict__ splitPos, u32 nSplits,
                                                        const u32* __restrict__ mStart, const u32* __restrict__ mLen, const u32* __restrict__ mOff,
                                                        Seq* __restrict__ seqs, u8* __restrict__ lits, ChunkMeta* __restrict__ meta, Seq* __restrict__ scratch, u32 nWaves)
{
    __shared__ StagedSeq stageAll[4][64];
    const u32 lane = lane_id(), wave = wave_id();
    StagedSeq* const stage = stageAll[wave];
    const u32 g = blockIdx.x * 4 + wave;
    Seq* const tmp = scratch + (u64)g * kMaxSeq;
    for (u32 c = g; c < nChunks; c += nWaves) {
        const u64 bStart = (u64)c * chunkBytes, bEnd = (bStart + chunkBytes) < n ? bStart + chunkBytes : n;
        const u32 blockLen = (u32)(bEnd - bStart);
        const u32 vStart = base + (u32)bStart;      // splits and matches are filed by virtual position (base = 0 without a prefix)
        const u32 s0 = lower_bound_u32(splitPos, nSplits, vStart), s1 = lower_bound_u32(splitPos, nSplits, vStart + blockLen);
        bool any = false;
        for (u32 s = s0 + lane; s < s1; s += 64) any |= mLen[s] != 0;
        if (!__ballot(any)) continue;
        const u8* const in = src + bStart;
        u8* const litOut = lits + (u64)c * kLitStride;
        Seq* const sq = seqs + (u64)c * kMaxSeq;
        const ChunkMeta m = meta[c];
        const u32 nF = m.litFromSrc ? 0u : m.nbSeq;
        // finder reader: batch [fBase, fBase + 64) in the lanes' fS / fE / fOff (block offsets); fPos = block offset behind the batch
        u32 fi = 0, fBase = 0, fPos = 0, fS = 0, fE = 0, fOff = 0;
        auto loadF = [&](u32 b) {
            const u32 i = b + lane;
            u32 ll = 0, ml = 0, off = 0;
            if (i < nF) { const Seq q = sq[i]; ll = q.litLength; ml = (u32)q.mlBase + 3; off = q.offBase - 3; }
            const u32 adv = ll + ml, incl = wave_scan_incl(adv);
            fS = fPos + incl - adv + ll; fE = fS + ml; fOff = off;
            fPos += read_lane(incl, 63); fBase = b;
        };
        // LDM reader: batch of splits [lBase, lBase + 64), lMask = lanes still to take
        u32 lBase = s0, lS = 0, lE = 0, lO = 0; u64 lMask = 0;
        auto loadL = [&](u32 b) {
            const u32 s = b + lane;
            const u32 len = s < s1 ? mLen[s] : 0u;
            lS = len ? mStart[s] - vStart : 0u; lE = lS + len; lO = len ? mOff[s] : 0u;
            lMask = __ballot(len != 0); lBase = b;
        };
        if (nF) loadF(0);
        loadL(s0);
        while (!lMask && lBase + 64 < s1) loadL(lBase + 64);
        u32 nOut = 0, nStaged = 0, litStart = 0, litPos = 0, pos = 0;
        auto flush = [&]() {
            wave_lds_sync();
            if (lane < nStaged) {
                const StagedSeq e = stage[lane];
                tmp[nOut - nStaged + lane] = e.q;
                if (e.q.litLength < 256) for (u32 k = 0; k < e.q.litLength; ++k) litOut[e.litDst + k] = in[e.litSrc + k];
            }
            u64 longs = __ballot(lane < nStaged && stage[lane].q.litLength >= 256);
            while (longs) {
                const u32 l = (u32)__ffsll((long long)longs) - 1; longs &= longs - 1;
                const StagedSeq e = stage[l];
                for (u32 k = lane; k < e.q.litLength; k += 64) litOut[e.litDst + k] = in[e.litSrc + k];
            }
            wave_lds_sync();
            nStaged = 0;
        };
        auto emit = [&](u32 s, u32 len, u32 off) {
            if (lane == 0) {
                StagedSeq& e = stage[nStaged];
                e.litSrc = litStart; e.litDst = litPos; e.q.offBase = off + 3; e.q.litLength = (u16)(s - litStart); e.q.mlBase = (u16)(len - 3);
            }
            litPos += s - litStart; litStart = s + len; nOut++; nStaged++;
            if (nStaged == 64) flush();
        };
        for (;;) {
            const bool haveL = lMask != 0;
            u32 Ls = 0, Le = 0, Lo = 0;
            if (haveL) { const u32 l = (u32)__ffsll((long long)lMask) - 1; Ls = read_lane(lS, l); Le = read_lane(lE, l); Lo = read_lane(lO, l); }
            const bool haveF = fi < nF;
            u32 Fs = 0, Fe = 0, Fo = 0;
            if (haveF) { if (fi >= fBase + 64) loadF(fBase + 64); const u32 l = fi - fBase; Fs = read_lane(fS, l); Fe = read_lane(fE, l); Fo = read_lane(fOff, l); }
            const u32 ps = Fs > pos ? Fs : pos;
            if (haveL && (!haveF || Ls <= ps)) {
                emit(Ls, Le - Ls, Lo); pos = Le;
                lMask &= lMask - 1;
                while (!lMask && lBase + 64 < s1) loadL(lBase + 64);
                continue;
            }
            if (!haveF) break;
            if (Fe <= ps) { fi++; continue; }
            const u32 pe = (haveL && Ls < Fe) ? Ls : Fe;
            if (pe - ps >= 4) emit(ps, pe - ps, Fo);
            pos = pe;
            if (pe == Fe) fi++;
        }
        if (nStaged) flush();
        // trailing literals, then the merged sequences in place of the finder's (each lane copies what it wrote to the scratch)
        for (u32 k = lane; k < blockLen - litStart; k += 64) litOut[litPos + k] = in[litStart + k];
        for (u32 i = lane; i < nOut; i += 64) sq[i] = tmp[i];
        if (lane == 0) { ChunkMeta& mo = meta[c]; mo.nbSeq = nOut; mo.litSize = litPos + (blockLen - litStart); mo.litFromSrc = 0; }
    }
}

// ---- host side ----
size_t ldm_small_bytes(u64 n) { return ((n + kLdmTile - 1) / kLdmTile + 64) * sizeof(u32) * 2 + 256; }
constexpr u32 kMergeWaves = 2048;
// bytes of the big workspace for nSplits splits over nChunks blocks
size_t ldm_big_bytes(u64 nSplits)
{
    const u64 S = nSplits + 64, sortTiles = (nSplits + kSortTile - 1) / kSortTile + 1;
    return (size_t)(S * (4 + 4 + 8 + 8 + 4 + 4 + 4 + 12) + 256 * sortTiles * 4 + (u64)kMergeWaves * kMaxSeq * sizeof(Seq) + 4096);
}

// Count the splits of [src, src + n): -> the device word *total (the host reads it back and sizes the big workspace)
// With a prefix (pfx.pre != nullptr) n is the virtual end, pfx.base + the source's length, and frameSpan is not used.
void launch_ldm_count(const u8* src, u64 n, u64 frameSpan, const LdmLaunch& p, u8* small, hipStream_t stream, const LdmPrefix& pfx)
{
    const u32 nTiles = (u32)((n + kLdmTile - 1) / kLdmTile);
    u32* tileCount = (u32*)small; u32* tileBase = tileCount + nTiles + 16; u32* total = tileBase + nTiles + 16;
    const u32 m = p.minMatch < 64 ? p.minMatch : 64;
    const u64 stopMask = (p.hashRateLog > 0 && p.hashRateLog <= m) ? (((1ull << p.hashRateLog) - 1) << (m - p.hashRateLog)) : ((1ull << p.hashRateLog) - 1);
    if (pfx.pre) hipLaunchKernelGGL((ldm_split_kernel<false, true>), dim3(nTiles), dim3(256), 0, stream, src, n, frameSpan, p.minMatch, stopMask, 0u, pfx, tileCount, nullptr,
                                    nullptr, nullptr, nullptr, nullptr);
    else hipLaunchKernelGGL((ldm_split_kernel<false, false>), dim3(nTiles), dim3(256), 0, stream, src, n, frameSpan, p.minMatch, stopMask, 0u, pfx, tileCount, nullptr,
                            nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(ldm_scan_kernel, dim3(1), dim3(1024), 0, stream, tileCount, tileBase, nTiles, total);
}
u32* ldm_total_word(u8* small, u64 n) { const u32 nTiles = (u32)((n + kLdmTile - 1) / kLdmTile); return (u32*)small + 2 * (nTiles + 16); }

// everything after the count: emit, sort, match, merge (nSplits > 0).  nChunks: the source's blocks.
LdmRecord launch_ldm_rest(const u8* src, u64 n, u32 nChunks, u32 chunkBytes, u64 frameSpan, const LdmLaunch& p, u32 nSplits, u8* small, u8* big,
                          Seq* seqs, u8* lits, ChunkMeta* meta, hipStream_t stream, StageHook hook, const LdmPrefix& pfx, bool merge)
{
    const u32 nTiles = (u32)((n + kLdmTile - 1) / kLdmTile);
    const u32* tileBase = (const u32*)small + nTiles + 16;
    const u64 S = (u64)nSplits + 64;
    u8* q = big;
    auto carve = [&](u64 bytes) { u8* r = q; q += (bytes + 255) & ~(u64)255; return r; };
    u32* splitPos = (u32*)carve(S * 4); u32* splitCheck = (u32*)carve(S * 4);
    u64* keyA = (u64*)carve(S * 8); u64* keyB = (u64*)carve(S * 8);
    u32* valA = (u32*)carve(S * 4); u32* valB = (u32*)carve(S * 4); u32* inv = (u32*)carve(S * 4);
    u32* mStart = (u32*)carve(S * 4); u32* mLen = (u32*)carve(S * 4); u32* mOff = (u32*)carve(S * 4);
    const u32 sortTiles = (nSplits + kSortTile - 1) / kSortTile;
    u32* hist = (u32*)carve((u64)256 * (sortTiles + 1) * 4);
    Seq* scratch = (Seq*)carve((u64)kMergeWaves * kMaxSeq * sizeof(Seq));
    const u32 m = p.minMatch < 64 ? p.minMatch : 64;
    const u64 stopMask = (p.hashRateLog > 0 && p.hashRateLog <= m) ? (((1ull << p.hashRateLog) - 1) << (m - p.hashRateLog)) : ((1ull << p.hashRateLog) - 1);
    const u32 hb = p.hashLog - p.bucketLog;
    if (pfx.pre) hipLaunchKernelGGL((ldm_split_kernel<true, true>), dim3(nTiles), dim3(256), 0, stream, src, n, frameSpan, p.minMatch, stopMask, hb, pfx, nullptr, tileBase,
                                    splitPos, splitCheck, keyA, valA);
    else hipLaunchKernelGGL((ldm_split_kernel<true, false>), dim3(nTiles), dim3(256), 0, stream, src, n, frameSpan, p.minMatch, stopMask, hb, pfx, nullptr, tileBase,
                            splitPos, splitCheck, keyA, valA);
    hook("ldm_split");
    // key bits: the frame's index in the pass above the bucket's hb bits
    const u64 nFrames = pfx.pre ? 1u : (n + frameSpan - 1) / frameSpan;
    u32 fBits = 0; while (((u64)1 << fBits) < nFrames) ++fBits;
    const u32 keyBits = fBits + hb;
    for (u32 shift = 0; shift < keyBits; shift += 8) {
        hipLaunchKernelGGL(ldm_radix_hist_kernel, dim3(sortTiles), dim3(256), 0, stream, keyA, nSplits, shift, hist, sortTiles);
        hipLaunchKernelGGL(ldm_scan_kernel, dim3(1), dim3(1024), 0, stream, hist, hist, 256u * sortTiles, nullptr);
        hipLaunchKernelGGL(ldm_radix_scatter_kernel, dim3(sortTiles), dim3(256), 0, stream, keyA, valA, keyB, valB, nSplits, shift, hist, sortTiles);
        u64* tk = keyA; keyA = keyB; keyB = tk; u32* tv = valA; valA = valB; valB = tv;
    }
    hipLaunchKernelGGL(ldm_inv_kernel, dim3((nSplits + 255) / 256), dim3(256), 0, stream, valA, inv, nSplits);
    hook("ldm_sort");
    if (pfx.pre && pfx.maxDist) hipLaunchKernelGGL((ldm_match_kernel<true, true>), dim3((nChunks + 3) / 4), dim3(256), 0, stream, src, n, nChunks, chunkBytes, frameSpan, p.minMatch, p.bucketLog, pfx,
                                                   splitPos, splitCheck, keyA, valA, inv, nSplits, mStart, mLen, mOff);
    else if (pfx.pre) hipLaunchKernelGGL(ldm_match_kernel<true>, dim3((nChunks + 3) / 4), dim3(256), 0, stream, src, n, nChunks, chunkBytes, frameSpan, p.minMatch, p.bucketLog, pfx,
                                    splitPos, splitCheck, keyA, valA, inv, nSplits, mStart, mLen, mOff);
    else hipLaunchKernelGGL(ldm_match_kernel<false>, dim3((nChunks + 3) / 4), dim3(256), 0, stream, src, n, nChunks, chunkBytes, frameSpan, p.minMatch, p.bucketLog, pfx,
                            splitPos, splitCheck, keyA, valA, inv, nSplits, mStart, mLen, mOff);
    hook("ldm_match");
    LdmRecord rec; rec.splitPos = splitPos; rec.mStart = mStart; rec.mLen = mLen; rec.mOff = mOff; rec.nSplits = nSplits;
    if (!merge) return rec;
    const u32 waves = nChunks < kMergeWaves ? ((nChunks + 3) & ~3u) : kMergeWaves;
    hipLaunchKernelGGL(ldm_merge_kernel, dim3(waves / 4), dim3(256), 0, stream, src, pfx.pre ? n - pfx.base : n, nChunks, chunkBytes, pfx.pre ? pfx.base : 0u, splitPos, nSplits, mStart, mLen, mOff,
                       seqs, lits, meta, scratch, waves);
    hook("ldm_merge");
    return rec;
}

} // namespace zmi
