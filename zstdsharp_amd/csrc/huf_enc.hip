// huf_enc.hip — literals section of a block on gfx950.
//
//   huf_hist_kernel   : the counting phase alone, one wave per stream of a chunk (HIST_count, U/Hist.cs:67-166).  A wave
//                       owns 16 KiB of LDS: 256 symbols x 64 BYTE counters, one per lane, so no two lanes ever add to
//                       the same counter — skew costs nothing and nothing is lost; one ds_add_u32 without return per
//                       input byte.  A byte counter holds 255, so the table is summed (v_sad_u8) into 32-bit
//                       registers and zeroed again after at most 8 x 16 bytes per lane.  Hands the four per-stream
//                       histograms and the two sample maxima of HUF_compress_internal's pre-check to the next kernel
//                       through the chunk's output slot.
//   huf_tree_kernel   : one wave per chunk (5.4 KiB of LDS, ~29 chunks per CU), four symbols per lane.  First the
//                       compressible / RLE / raw verdict of HUF_compress_internal (U/HufCompress.cs:1360-1543) and
//                       HUF_sort (:520-680: parallel bucket placement, the log2 buckets quick-sorted on separate lanes
//                       exactly as the reference does), then the serial constructions, exactly as
//                       the reference: HUF_buildTree / HUF_setMaxHeight / HUF_buildCTableFromTree (:377-823), the tree
//                       description (HUF_writeCTable_wksp + HUF_compressWeights, :40-235) and every raw / RLE /
//                       compressed decision of ZSTD_compressLiterals (U/ZstdCompressLiterals.cs:86-185).  Because
//                       stream sizes follow from histogram x code length, the whole literals section is sized before
//                       a byte is encoded.
//   huf_encode_kernel : one 256-thread workgroup per chunk, wave w encodes stream w
//                       (HUF_compress4X_usingCTable_internal, U/HufCompress.cs:1221-1321): symbols are taken last
//                       to first, 16 per lane, their codes concatenated in registers, bit offsets come from a wave
//                       prefix scan, and the lanes OR their bits into an LDS tile that is flushed with coalesced
//                       dword stores.
// Given the same literals and sequence count, the bytes produced equal the oracle's
// (tests/test_gpu_parity.py::test_entropy_stage_is_byte_identical_to_oracle).
#include "zmi_device.h"
#include "zmi_fse.h"
#include "zmi_host.h"

namespace zmi {

#ifdef ZMI_LZ_STAMPS
__device__ unsigned long long g_hufStamps[16];
#define ZMI_HSTAMP(i) do { if (tid == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); stampAcc[i] += now_ - stampLast; stampLast = now_; } } while (0)
#else
#define ZMI_HSTAMP(i) do { } while (0)
#endif

struct Node { u32 count; u16 parent; u8 byte; u8 nbBits; };

struct alignas(16) HufTreeLds {
    Node nodes[513];
    u8  nbBits[256];
    u8  weights[256];
    u32 wcount[13]; s16 wnorm[13]; u16 wstate[64]; SymTT wtt[13]; u16 wcumul[15]; u8 wsym[64];
    u32 valPerRank[13];
    u32 rankLast[14];
    u32 sh[8];
    u32 sortPad[90];            // makes room for HufSortLds, which otherwise lies over members that are dead while HUF_sort runs
};
// HUF_sort's scratch: lives from nodes[258] to the end of HufTreeLds (the node queue, the code lengths and the weight tables
// are written only after the sort).  The placement keys are dead before the first quicksort pushes.
struct HufSortLds {
    union {
        u32 keys[256];          // huf_get_index(count) << 8 | 255 - symbol (0 above maxSymbolValue)
        s16 qsStack[26][64];    // one explicit quicksort stack per log2 bucket (buckets are sorted by separate lanes); values -1..256
    };
    u16 rankGe[32];             // [t] = symbols whose index is >= 164 + t: bucket 165 + b spans [rankGe[b + 1], rankGe[b])
};
constexpr u32 kSortScratchNode = 258;
static_assert(kSortScratchNode * sizeof(Node) % 16 == 0, "keys are read 16 bytes at a time");
static_assert(kSortScratchNode * sizeof(Node) + sizeof(HufSortLds) <= sizeof(HufTreeLds), "HUF_sort's scratch fits the tree's storage");

enum { kShHuffLog = 4, kShNonNull, kShRoot, kShHSize };

// ---- HUF_sort (U/HufCompress.cs:520-680): bucket sort by count, quicksort inside the log2 buckets ----
__device__ __forceinline__ u32 huf_get_index(u32 count) { return count < 165 ? count : highbit32(count) + 158; }

__device__ inline void huf_insertion_sort(Node* a, int low, int high)
{
    const int size = high - low + 1; a += low;
    for (int i = 1; i < size; i++) {
        const Node key = a[i]; int j = i - 1;
        while (j >= 0 && a[j].count < key.count) { a[j + 1] = a[j]; j--; }
        a[j + 1] = key;
    }
}
__device__ inline int huf_partition(Node* a, int low, int high)
{
    const u32 pivot = a[high].count; int i = low - 1;
    for (int j = low; j < high; j++) if (a[j].count > pivot) { i++; const Node t = a[i]; a[i] = a[j]; a[j] = t; }
    { const Node t = a[i + 1]; a[i + 1] = a[high]; a[high] = t; }
    return i + 1;
}
// HUF_simpleQuickSort: a call checks the insertion-sort threshold once, then partitions in a loop, recursing
// (threshold checked again) into the smaller side and continuing the loop (threshold NOT checked) on the larger.
// Sub-ranges are disjoint, so an explicit stack of {low, high, isCall} reproduces the result exactly.
__device__ inline void huf_quick_sort(Node* a, int low0, int high0, s16* stack)
{
    int sp = 0;
    stack[sp++] = (s16)low0; stack[sp++] = (s16)high0; stack[sp++] = 1;
    while (sp) {
        const int isCall = stack[--sp]; const int high = stack[--sp]; const int low = stack[--sp];
        if (isCall && high - low < 8) { huf_insertion_sort(a, low, high); continue; }
        if (!(low < high)) continue;
        const int idx = huf_partition(a, low, high);
        if (idx - low < high - idx) {
            stack[sp++] = (s16)(idx + 1); stack[sp++] = (s16)high;      stack[sp++] = 0;
            stack[sp++] = (s16)low;       stack[sp++] = (s16)(idx - 1); stack[sp++] = 1;
        } else {
            stack[sp++] = (s16)low;       stack[sp++] = (s16)(idx - 1); stack[sp++] = 0;
            stack[sp++] = (s16)(idx + 1); stack[sp++] = (s16)high;      stack[sp++] = 1;
        }
    }
}

// the log2 buckets (extents computed by the kernel's parallel placement) are sorted on separate lanes
__device__ inline void huf_sort_bucket(Node* nodes, HufSortLds& S, u32 b /* 0..25 */)
{
    const u32 bucketStart = S.rankGe[b + 1], bucketSize = S.rankGe[b] - bucketStart;
    if (bucketSize > 1) huf_quick_sort(nodes + 1 + bucketStart, 0, (int)bucketSize - 1, S.qsStack[b]);
}

// ---- HUF_buildTree (U/HufCompress.cs:689-738) ----
__device__ inline int huf_build_tree(Node* huffNode, u32 maxSV, int* rootOut)
{
    Node* const huffNode0 = huffNode - 1;
    int nonNullRank = (int)maxSV, lowS, lowN, nodeNb = 256, nodeRoot;
    while (huffNode[nonNullRank].count == 0) nonNullRank--;
    lowS = nonNullRank; nodeRoot = nodeNb + lowS - 1; lowN = nodeNb;
    huffNode[nodeNb].count = huffNode[lowS].count + huffNode[lowS - 1].count;
    huffNode[lowS].parent = huffNode[lowS - 1].parent = (u16)nodeNb;
    nodeNb++; lowS -= 2;
    for (int n = nodeNb; n <= nodeRoot; n++) huffNode[n].count = 1u << 30;
    huffNode0[0].count = 1u << 31;
    // two-queue merge; the heads of both queues are kept in registers so that each pick costs one LDS read
    u32 cS = huffNode[lowS].count, cN = huffNode[lowN].count;
    while (nodeNb <= nodeRoot) {
        int n1, n2; u32 c1, c2;
        // (a head equal to nodeNb reads the 1<<30 placeholder, exactly as the reference's second comparison does)
        if (cS < cN) { n1 = lowS--; c1 = cS; cS = huffNode[lowS].count; } else { n1 = lowN++; c1 = cN; cN = huffNode[lowN].count; }
        if (cS < cN) { n2 = lowS--; c2 = cS; cS = huffNode[lowS].count; } else { n2 = lowN++; c2 = cN; cN = huffNode[lowN].count; }
        huffNode[nodeNb].count = c1 + c2;
        if (lowN == nodeNb) cN = c1 + c2;          // the node just created is the next head of the node queue
        huffNode[n1].parent = huffNode[n2].parent = (u16)nodeNb;
        nodeNb++;
    }
    // code lengths (the reference's two top-down loops) are computed by the caller, one leaf per lane
    *rootOut = nodeRoot;
    return nonNullRank;
}

// ---- HUF_setMaxHeight (U/HufCompress.cs:377-514), called by all 64 lanes of the chunk's wave ----
// The three scans of the reference (clamp the over-long tail and total its cost; skip the run already at maxNbBits; find
// the last symbol of every shorter length) are evaluated with ballots over the four positions each lane holds; only the
// repayment loops, whose steps depend on each other, run on lane 0.  rankLast lives in LDS (it is indexed dynamically).
template <class LDS>
__device__ inline u32 huf_set_max_height_wave(LDS& L, Node* huffNode, u32 lastNonNull, u32 maxNbBits)
{
    const u32 lane = lane_id();
    const u32 largestBits = huffNode[lastNonNull].nbBits;
    if (largestBits <= maxNbBits) return largestBits;
    const u32 noSymbol = 0xF0F0F0F0u;
    u32 nb[4];
    for (u32 k = 0; k < 4; ++k) { const u32 pos = k * 64 + lane; nb[k] = pos <= lastNonNull ? huffNode[pos].nbBits : 0xFFu; }
    auto highest = [&](bool p0, bool p1, bool p2, bool p3) -> int {       // highest position whose predicate holds, -1 if none
        const u64 b3 = ballot(p3), b2 = ballot(p2), b1 = ballot(p1), b0 = ballot(p0);
        if (b3) return 192 + 63 - __builtin_clzll(b3);
        if (b2) return 128 + 63 - __builtin_clzll(b2);
        if (b1) return 64 + 63 - __builtin_clzll(b1);
        if (b0) return 63 - __builtin_clzll(b0);
        return -1;
    };
    // loop 1: the tail of positions above n1 is longer than allowed
    const int n1 = highest(nb[0] <= maxNbBits, nb[1] <= maxNbBits, nb[2] <= maxNbBits, nb[3] <= maxNbBits);
    const u32 baseCost = 1u << (largestBits - maxNbBits);
    int cost = 0;
    for (u32 k = 0; k < 4; ++k) {
        const int pos = (int)(k * 64 + lane);
        if (pos > n1 && pos <= (int)lastNonNull) { cost += (int)(baseCost - (1u << (largestBits - nb[k]))); huffNode[pos].nbBits = (u8)maxNbBits; }
    }
    int totalCost = (int)wave_sum((u32)cost);
    totalCost >>= (largestBits - maxNbBits);
    // loop 2: n = last position (<= n1) not already at maxNbBits
    auto upTo = [&](u32 k, int lim) { return (int)(k * 64 + lane) <= lim; };
    const int n = highest(upTo(0, n1) && nb[0] != maxNbBits, upTo(1, n1) && nb[1] != maxNbBits, upTo(2, n1) && nb[2] != maxNbBits, upTo(3, n1) && nb[3] != maxNbBits);
    // loop 3: rankLast[maxNbBits - b] = last position of length b, if nothing shorter or equal sits above it
    if (lane < 14) L.rankLast[lane] = noSymbol;
    wave_lds_sync();
    {
        int above = -1;        // highest position (<= n) of any length smaller than b
        for (u32 b = 1; b < maxNbBits; ++b) {
            const int hi = highest(upTo(0, n) && nb[0] == b, upTo(1, n) && nb[1] == b, upTo(2, n) && nb[2] == b, upTo(3, n) && nb[3] == b);
            if (hi >= 0 && hi > above && lane == 0) L.rankLast[maxNbBits - b] = (u32)hi;
            if (hi > above) above = hi;
        }
    }
    wave_lds_sync();
    if (lane == 0) {
        u32* rankLast = L.rankLast; int nn = n;
        while (totalCost > 0) {
            u32 nBitsToDecrease = highbit32((u32)totalCost) + 1;
            for (; nBitsToDecrease > 1; nBitsToDecrease--) {
                const u32 highPos = rankLast[nBitsToDecrease], lowPos = rankLast[nBitsToDecrease - 1];
                if (highPos == noSymbol) continue;
                if (lowPos == noSymbol) break;
                const u32 highTotal = huffNode[highPos].count, lowTotal = 2 * huffNode[lowPos].count;
                if (highTotal <= lowTotal) break;
            }
            while (nBitsToDecrease <= 12 && rankLast[nBitsToDecrease] == noSymbol) nBitsToDecrease++;
            totalCost -= 1 << (nBitsToDecrease - 1);
            huffNode[rankLast[nBitsToDecrease]].nbBits++;
            if (rankLast[nBitsToDecrease - 1] == noSymbol) rankLast[nBitsToDecrease - 1] = rankLast[nBitsToDecrease];
            if (rankLast[nBitsToDecrease] == 0) rankLast[nBitsToDecrease] = noSymbol;
            else {
                rankLast[nBitsToDecrease]--;
                if (huffNode[rankLast[nBitsToDecrease]].nbBits != maxNbBits - nBitsToDecrease) rankLast[nBitsToDecrease] = noSymbol;
            }
        }
        while (totalCost < 0) {
            if (rankLast[1] == noSymbol) {
                while (huffNode[nn].nbBits == maxNbBits) nn--;
                huffNode[nn + 1].nbBits--;
                rankLast[1] = (u32)(nn + 1);
                totalCost++;
                continue;
            }
            huffNode[rankLast[1] + 1].nbBits--;
            rankLast[1]++;
            totalCost++;
        }
    }
    wave_lds_sync();
    return maxNbBits;
}

// ---- HUF_compressWeights (U/HufCompress.cs:40-125); returns bytes written, 0 = not compressible, 1 = single symbol ----
// Called by all 64 lanes of the chunk's wave (the result is uniform).  Lane 0 takes the decisions, FSE_normalizeCount and
// FSE_writeNCount (13 symbols); the table is built by the wave; then FSE_compress_usingCTable_generic (U/FseCompress.cs:722-820):
// symbol i uses state (i & 1), last symbol first — two independent chains, so lane p walks the symbols of parity p (each lane
// first fetches the transforms of its four symbols, so a chain step is one dependent LDS read) and leaves (bits, count) per
// symbol; the fields are placed by a prefix sum over the emission order and OR-ed into an LDS bit buffer, the two final states
// and the end mark behind them (BIT_closeCStream), and the bytes copied out.  (On one lane with a serial bit writer this was
// 300 000 cycles per chunk — the longest stretch of huf_tree_kernel; byte-identical by tests/test_gpu_parity.py.)
// Scratch: the tree's node array, dead by now.
__device__ inline u32 huf_compress_weights_wave(HufTreeLds& L, u8* dst, u32 wtSize, u32 lane)
{
    u32* const fields = reinterpret_cast<u32*>(L.nodes);            // [256] value | nbBits << 16, by symbol index
    SymTT* const tts = reinterpret_cast<SymTT*>(fields + 256);      // [256] the symbols' transforms
    u32* const bitbuf = reinterpret_cast<u32*>(tts + 256);          // [64]
    u16* const cumR = reinterpret_cast<u16*>(bitbuf + 64);          // [64] scratch of the table build
    static_assert(256 * 4 + 256 * sizeof(SymTT) + 64 * 4 + 64 * 2 <= sizeof(L.nodes), "scratch fits the node array");
    u32 res = 0xFFFFFFFFu, maxSV = 12, tableLog = 0, hs = 0;
    if (lane == 0) {
        do {
            if (wtSize <= 1) { res = 0; break; }
            while (!L.wcount[maxSV]) maxSV--;
            u32 maxCount = 0;
            for (u32 s = 0; s <= maxSV; s++) if (L.wcount[s] > maxCount) maxCount = L.wcount[s];
            if (maxCount == wtSize) { res = 1; break; }
            if (maxCount == 1) { res = 0; break; }
            tableLog = fse_optimal_table_log(6, wtSize, maxSV, 2);
            if (!fse_normalize_count(L.wnorm, tableLog, L.wcount, wtSize, maxSV, 0)) { res = 0; break; }
            hs = fse_write_ncount(dst, L.wnorm, maxSV, tableLog);
            if (!hs) { res = 0; break; }
            if (wtSize <= 2) { res = 0; break; }
        } while (false);
    }
    res = uniform(res); maxSV = uniform(maxSV); tableLog = uniform(tableLog); hs = uniform(hs);
    if (res != 0xFFFFFFFFu) return res;
    wave_lds_sync();                                                // (wnorm)
    fse_build_ctable_wave(L.wstate, L.wtt, L.wnorm, maxSV, tableLog, cumR, L.wsym, lane);
#pragma unroll
    for (u32 k = 0; k < 4; ++k) { const u32 i = k * 64 + lane; if (i < wtSize) tts[i] = L.wtt[L.weights[i]]; }
    if (lane < 64) bitbuf[lane] = 0;
    wave_lds_sync();
    if (lane < 2) {                                                 // the chain of parity `lane`
        const int top = (int)(wtSize - 1) - ((((wtSize - 1) & 1u) != lane) ? 1 : 0);
        u32 v = fse_init_state2(L.wstate, L.wtt, L.weights[top]);
        for (int i = top - 2; i >= 0; i -= 2) {
            const SymTT t = tts[i];
            const u32 nb = (v + t.deltaNbBits) >> 16;
            fields[i] = (v & ((1u << nb) - 1u)) | (nb << 16);
            v = L.wstate[(s32)(v >> nb) + t.deltaFindState];
        }
        L.sh[6 + lane] = v;                                         // (kShRoot and kShHSize: free by now)
    }
    wave_lds_sync();
    // emission order: symbol wtSize - 3 first, symbol 0 last; rank r = wtSize - 3 - i
    const u32 nEmit = wtSize - 2;
    u32 carry = 0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const u32 r = k * 64 + lane;
        const bool have = r < nEmit;
        const u32 f = have ? fields[nEmit - 1 - r] : 0u;
        const u32 nb = f >> 16, val = f & 0xFFFFu;
        const u32 incl = wave_scan_incl(nb);
        const u32 at = carry + incl - nb;
        if (nb) {
            const u64 sh = (u64)val << (at & 31u);
            atomicOr(&bitbuf[at >> 5], (u32)sh);
            if ((u32)(sh >> 32)) atomicOr(&bitbuf[(at >> 5) + 1], (u32)(sh >> 32));
        }
        carry += read_lane(incl, 63);
    }
    wave_lds_sync();
    if (lane == 0) {                                                // FSE_flushCState x2 (state 2 first) + the end mark
        const u32 st0 = L.sh[6], st1 = L.sh[7], mask = (1u << tableLog) - 1u;
        const u64 tail = (u64)(st1 & mask) | ((u64)(st0 & mask) << tableLog) | (1ull << (2 * tableLog));
        const u32 at = carry;
        const u64 lo = tail << (at & 31u);                          // (2 * 6 + 1 bits shifted by at most 31: fits 64)
        bitbuf[at >> 5] |= (u32)lo;
        if ((u32)(lo >> 32)) bitbuf[(at >> 5) + 1] |= (u32)(lo >> 32);
    }
    wave_lds_sync();
    const u32 nBytes = (carry + 2 * tableLog + 1 + 7) >> 3;
    const u8* const bytes = reinterpret_cast<const u8*>(bitbuf);
#pragma unroll
    for (u32 k = 0; k < 4; ++k) { const u32 i = k * 64 + lane; if (i < nBytes) dst[hs + i] = bytes[i]; }
    return hs + nBytes;
}

__device__ __forceinline__ u32 min_gain(u32 srcSize) { return (srcSize >> 6) + 2; }   // ZSTD_minGain, strategies < btultra

// ---- counting phase: lane-private byte counters ----
// The wave's table holds 256 symbols x 16 dwords; lane l counts in byte (l >> 4) of dword sym * 16 + (l & 15).  A counter byte
// has one writer, so an add never meets another lane's on its address, and by banks (dword mod 32, inside a 32-lane half)
// only lanes l and l + 16 can meet: 2-way at most, whatever the data.
constexpr u32 kHistBatch = 8;            // 16-byte loads in flight per lane, and per lane between two flushes (4: 0.357 ms per GiB of Zipf bytes against 0.331)
static_assert(kHistBatch * 16 + 2 <= 255, "a byte counter takes a batch plus one head and one tail byte");
constexpr u32 kHistItemsPerWave = 8;     // (chunk, stream) items per wave of a large call (1 GiB of Zipf bytes: 1 item 0.320 ms, 4 0.320, 8 0.331, 32 0.341; text 0.149 / 0.137 / 0.139 / 0.136)
constexpr u32 kHistMinGrid = 2 * 9 * 256;   // a small call gets a wave per item: two rounds of 9 waves (16 KiB each) on 256 CUs

struct HufHistLds { u32 ctr[256 * 16]; };

__device__ __forceinline__ void hist_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
__device__ __forceinline__ void hist_add(u32* slot0 /* &ctr[lane & 15] */, u32 sym, u32 inc)
{
    (void)__hip_atomic_fetch_add(slot0 + sym * 16, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);     // ds_add_u32, no return
}
// adds the table to acc[k] (symbol k * 64 + lane) and leaves it zeroed
__device__ __forceinline__ void hist_flush(HufHistLds& L, u32 lane, u32 (&acc)[4])
{
    hist_wave_sync();
    const uint4* t4 = reinterpret_cast<const uint4*>(L.ctr);
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            // ds_read_b128 serves 16 lanes at a time over 64 banks; symbols are 16 dwords apart, so lanes that agree in
            // (lane & 3) start at different quarters of their symbols
            const uint4 x = t4[(k * 64 + lane) * 4 + ((j + (lane >> 2)) & 3u)];
            acc[k] = __builtin_amdgcn_sad_u8(x.x, 0u, acc[k]); acc[k] = __builtin_amdgcn_sad_u8(x.y, 0u, acc[k]);
            acc[k] = __builtin_amdgcn_sad_u8(x.z, 0u, acc[k]); acc[k] = __builtin_amdgcn_sad_u8(x.w, 0u, acc[k]);
        }
    }
    hist_wave_sync();
    uint4* z4 = reinterpret_cast<uint4*>(L.ctr);
#pragma unroll
    for (u32 i = 0; i < 16; ++i) z4[i * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
    hist_wave_sync();
}
// counts lit[r0, r1) into acc; the table is zero before and after
__device__ __forceinline__ void hist_count_range(HufHistLds& L, const u8* __restrict__ lit, u32 r0, u32 r1, u32 lane, u32 (&acc)[4])
{
    u32* const slot0 = L.ctr + (lane & 15u);
    const u32 inc = 1u << (8u * (lane >> 4));
    // 16 bytes per lane per load (aligned: the literal buffer is, a caller's source need not be); the pieces in front of and
    // behind the aligned part are shorter than 16 bytes: one byte per lane
    u32 a0 = r0 + ((0u - (u32)(uintptr_t)(lit + r0)) & 15u); if (a0 > r1) a0 = r1;
    if (r0 + lane < a0) hist_add(slot0, lit[r0 + lane], inc);
    const u32 nVec = (r1 - a0) >> 4;
    const u32 t0 = a0 + (nVec << 4);
    if (t0 + lane < r1) hist_add(slot0, lit[t0 + lane], inc);
    const uint4* v4 = reinterpret_cast<const uint4*>(lit + a0);
    auto count16 = [&](const uint4 v) {
        const u32 d[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
#pragma unroll
            for (u32 b = 0; b < 4; ++b) hist_add(slot0, (d[k] >> (8 * b)) & 0xFFu, inc);
        }
    };
    // (the loads are unconditional — past the end they re-read the range's first piece —: behind a branch the compiler
    //  waits for every load in flight instead of the oldest; the next batch is on its way while this one is counted and flushed)
    uint4 q[kHistBatch];
    if (nVec) {
#pragma unroll
        for (u32 k = 0; k < kHistBatch; ++k) { const u32 ix = lane + 64 * k; q[k] = v4[ix < nVec ? ix : 0u]; }
    }
    for (u32 i = lane; i < nVec + lane; i += 64 * kHistBatch) {       // (uniform trip count)
#pragma unroll
        for (u32 k = 0; k < kHistBatch; ++k) {
            const uint4 v = q[k];
            const u32 nx = i + 64 * k + 64 * kHistBatch;
            q[k] = v4[nx < nVec ? nx : 0u];
            if (i + 64 * k < nVec) count16(v);
        }
        hist_flush(L, lane, acc);
    }
    if (!nVec) hist_flush(L, lane, acc);
}

// Front half: the four per-stream histograms (they also size the four streams) and the sample maxima.  One wave per workgroup;
// a wave takes (chunk, stream) items blockIdx.x, blockIdx.x + gridDim.x, ...
// MINLIT: literals up to this many are stored raw whatever they hold — 63, or 6 where a dictionary's Huffman table may be reused
// (huf_tree_kernel<true> decides per chunk; a histogram it does not need costs a few bytes of reading).
template <u32 MINLIT>
__global__ __launch_bounds__(64) void huf_hist_kernel(const u8* __restrict__ lits, const ChunkMeta* __restrict__ meta,
                                                      u8* __restrict__ slots, const u32 rawLiterals, const u8* __restrict__ src, const u32 chunkBytes,
                                                      const u32 nItems)
{
    __shared__ HufHistLds L;
    const u32 lane = threadIdx.x;
#ifdef ZMI_LZ_STAMPS
    const u32 tid = lane; unsigned long long stampAcc[10] = {0,0,0,0,0,0,0,0,0,0}; unsigned long long stampLast = __builtin_amdgcn_s_memtime();
#endif
    {
        uint4* z4 = reinterpret_cast<uint4*>(L.ctr);
#pragma unroll
        for (u32 i = 0; i < 16; ++i) z4[i * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
    }
    hist_wave_sync();
    for (u32 item = blockIdx.x; item < nItems; item += gridDim.x) {
        const u32 c = item >> 2, w = item & 3u;
        const ChunkMeta m0 = meta_checked(meta[c]);
        const u32 litSize = m0.litSize, nbSeqIn = m0.nbSeq;
        // ZSTD_compressLiterals: <= 63 literals are stored raw (no previous table in a one-block frame)
        // (rawLiterals: literal compression is off — the fast strategy with a step, i.e. negative levels; U/ZstdCompressInternal.cs:146-173)
        if (litSize <= MINLIT || rawLiterals) continue;   // huf_tree_kernel stores them raw
        HufWork* __restrict__ W = reinterpret_cast<HufWork*>(slots + (u64)c * kSlotStride);
        // (a chunk without sequences never copied its literals: they are its source bytes, lz_fast.hip)
        const u8* __restrict__ lit = m0.litFromSrc ? src + (u64)c * chunkBytes : lits + (u64)c * kLitStride;
        const u32 seg = (litSize + 3) / 4;
        u32 s0 = w * seg; if (s0 > litSize) s0 = litSize;
        const u32 s1 = (s0 + seg < litSize) ? s0 + seg : litSize;
        // HUF_compress_internal's 2 x 4 KiB pre-check (U/HufCompress.cs:1412-1446) looks at the first 4 KiB of stream 0 and the
        // last 4 KiB of stream 3 (a stream is >= 10 KiB here): those are counted as a range of their own and read off at the flush
        const u32 suspect = (nbSeqIn == 0) || (litSize / nbSeqIn >= 20);
        const bool doSample = suspect && litSize >= 4096 * 10;
        u32 mid = s1;
        if (doSample && w == 0) mid = s0 + 4096;
        if (doSample && w == 3) mid = s1 - 4096;
        u32 acc[4] = { 0, 0, 0, 0 }, part[4] = { 0, 0, 0, 0 };
        if (s0 < mid) hist_count_range(L, lit, s0, mid, lane, acc);
#pragma unroll
        for (u32 k = 0; k < 4; ++k) part[k] = acc[k];
        if (mid < s1) hist_count_range(L, lit, mid, s1, lane, acc);
#pragma unroll
        for (u32 k = 0; k < 4; ++k) W->hist[w][k * 64 + lane] = (u16)acc[k];
        if (doSample && (w == 0 || w == 3)) {
            u32 mx = 0;
#pragma unroll
            for (u32 k = 0; k < 4; ++k) { const u32 v = w == 0 ? part[k] : acc[k] - part[k]; mx = v > mx ? v : mx; }
            mx = wave_max(mx);
            if (lane == 0) W->sampleMax[w ? 1 : 0] = mx;
        }
    }
    ZMI_HSTAMP(0);
#ifdef ZMI_LZ_STAMPS
    if (tid == 0) atomicAdd(&g_hufStamps[0], stampAcc[0]);
#endif
}

// Back half: the verdict and HUF_sort (parallel over the 256 symbols, four per lane), then the serial constructions
// (HUF_buildTree, HUF_setMaxHeight, HUF_compressWeights) and the decisions.  One wave per chunk and 5.4 KiB of LDS, so
// that ~29 chunks per CU hide each other's LDS latency.
// DICT (ZSTDMI_CCtx_setDictEntropy with a formatted dictionary): the first block of a frame has the dictionary's Huffman table as its
// previous table, and ZSTD_compressLiterals / HUF_compress_internal decide with it (U/ZstdCompressLiterals.cs:86-185,
// U/HufCompress.cs:1360-1543): raw up to 6 literals instead of 63 and a single stream up to 1023 when the table is `valid`; the
// table as it is for <= 1024 literals (preferRepeat: every strategy here is below lazy) once it is known to cover them; else the
// block's own tree unless the old table costs no more than the new one with its description.  What the old table costs follows
// from the histograms in registers.  A block coded with it gets kLitTreeless and a copy of the dictionary's codes as its table.
// The instance without DICT is the code from before the switch existed.
// SET (ZSTDMI_compressBatchCDicts, zmi_cdictset.h; on the DICT instance): the chunk's tables come from dictSlots[chunkSlot[c]].dct, one
// scalar load per workgroup; null there means "this chunk has no dictionary tables", and it comes out as the instance without DICT
// writes it (dMode stays kDictHufNone, which switches every DICT step off).
// (The kernel is a template on SET itself, which costs the other instances a `false` in their mangled names: as an inlined body behind
// two kernels, huf_tree_kernel<true> / <false> came out with 52 / 45 SGPR spills for the 56 / 46 they have.  dictSlots and chunkSlot
// are arguments of every instance; the instances without SET never load them.)
template <bool DICT, bool SET = false>
__global__ __launch_bounds__(64) void huf_tree_kernel(ChunkMeta* __restrict__ meta, HufTable* __restrict__ tables, const u8* __restrict__ slots,
                                                      const u32 rawLiterals, const DictCTables* __restrict__ dctArg, const u32 frameBlocks,
                                                      const CDictSlot* __restrict__ dictSlots, const u32* __restrict__ chunkSlot)
{
    static_assert(!SET || DICT, "the set form stands on the DICT instance");
    __shared__ HufTreeLds L;
    const u32 c = blockIdx.x, lane = threadIdx.x, tid = lane;
    const DictCTables* __restrict__ const dct = SET ? dictSlots[chunkSlot[c]].dct : dctArg;
    // (the record is written back field by field: a whole-struct copy kept across the kernel went through scratch memory)
    const ChunkMeta m = meta_checked(meta[c]);
    ChunkMeta* const mOut = meta + c;
    const u32 litSize = m.litSize;
    auto store_section = [&](u32 litMode, u32 lhSz, u32 sectionSize) {      // + what meta_checked settled
        mOut->srcSize = m.srcSize; mOut->nbSeq = m.nbSeq; mOut->litSize = m.litSize; mOut->fhSize = m.fhSize;
        mOut->litMode = litMode; mOut->lhSize = lhSz; mOut->litSectionSize = sectionSize;
    };
    const u32 lhSizeRaw = 1 + (litSize > 31) + (litSize > 4095);
    const HufWork* __restrict__ W = reinterpret_cast<const HufWork*>(slots + (u64)c * kSlotStride);
#ifdef ZMI_LZ_STAMPS
    unsigned long long stampAcc[10] = {0,0,0,0,0,0,0,0,0,0}; unsigned long long stampLast = __builtin_amdgcn_s_memtime();
#endif
    // the dictionary's table stands behind a frame's first block only (a later block never writes a treeless section)
    u32 dMode = kDictHufNone;
    if (DICT && (!SET || dct)) { if (!frameBlocks || block_index(c, frameBlocks) == 0) dMode = dct->hufMode; }
    // ZSTD_compressLiterals: <= 63 literals are stored raw (no previous table in a one-block frame)
    if (litSize <= ((DICT && dMode == kDictHufValid) ? 6u : 63u) || rawLiterals) {        // (or ZSTD_noCompressLiterals because literal compression is disabled, U/ZstdCompressLiterals.cs:99-101)
        if (tid == 0) store_section(kLitRaw, lhSizeRaw, lhSizeRaw + litSize);
        return;
    }
    const u32 lhSize = 3 + (litSize >= 1024) + (litSize >= 16384);
    const u32 single = litSize < 256 || (DICT && dMode == kDictHufValid && lhSize == 3);
    HufTable* T = tables + c;
    u32 hst[4][4], cnt[4];          // [stream][k]: symbol k * 64 + lane
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        cnt[k] = 0;
#pragma unroll
        for (u32 w = 0; w < 4; ++w) { hst[w][k] = W->hist[w][k * 64 + lane]; cnt[k] += hst[w][k]; }
    }
    // what the dictionary's table makes of the four streams, and whether it has a code for every literal that occurs
    u32 dictBits[4] = { 0, 0, 0, 0 };
    bool useOld = false, oldUsable = false;
    if (DICT && dMode != kDictHufNone) {
        u32 dnb[4]; bool covered = true;
#pragma unroll
        for (u32 k = 0; k < 4; ++k) { dnb[k] = dct->hufNbBits[k * 64 + lane]; covered &= ballot(cnt[k] != 0 && dnb[k] == 0) == 0; }
#pragma unroll
        for (u32 w = 0; w < 4; ++w) {
            u32 bits = 0;
#pragma unroll
            for (u32 k = 0; k < 4; ++k) bits += hst[w][k] * dnb[k];
            dictBits[w] = wave_sum(bits);
        }
        oldUsable = covered;                                        // (a `valid` table covers every byte: HUF_validateCTable for `check`)
        useOld = dMode == kDictHufValid && covered && litSize <= 1024;      // preferRepeat with a valid table: no look at the literals
    }
    u32 shCompressed = 1, maxSV = 0, shRle = 0, shRleByte = 0;
    if (DICT && useOld) shCompressed = 0;
    else {   // compressible at all?  (HUF_compress_internal, U/HufCompress.cs:1412-1462) — uniform
        u32 largest = cnt[0];
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            const u64 nz = ballot(cnt[k] != 0);
            if (nz) maxSV = k * 64 + 63 - (u32)__builtin_clzll(nz);
            largest = cnt[k] > largest ? cnt[k] : largest;
        }
        largest = wave_max(largest);
        const u32 suspect = (m.nbSeq == 0) || (litSize / m.nbSeq >= 20);
        const bool doSample = suspect && litSize >= 4096 * 10;
        if (doSample && W->sampleMax[0] + W->sampleMax[1] <= ((2 * 4096) >> 7) + 4) { shCompressed = 0; maxSV = 255; }
        else if (largest == litSize) {             // one symbol: it is the RLE byte
            shRle = 1; shCompressed = 0;
#pragma unroll
            for (u32 k = 0; k < 4; ++k) { const u64 b = ballot(cnt[k] == litSize); if (b) shRleByte = k * 64 + ctz64(b); }
        }
        else if (largest <= (litSize >> 7) + 4) shCompressed = 0;
        if (DICT && shCompressed && oldUsable && litSize <= 1024) { useOld = true; shCompressed = 0; }      // preferRepeat after the check
    }
    u32 huffLog = 0;
    u32 streamBits[4] = { 0, 0, 0, 0 };
    if (shCompressed) {
        HufSortLds& S = *reinterpret_cast<HufSortLds*>(&L.nodes[kSortScratchNode]);
        // HUF_sort's bucket placement (U/HufCompress.cs:635-680) without the serial counters: a symbol lands behind
        // every symbol of a higher bucket and behind the lower-numbered symbols of its own bucket — behind every symbol
        // with a larger key
        u32 idx[4], key[4], pos[4];
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            const u32 sIdx = k * 64 + lane;
            idx[k] = huf_get_index(cnt[k]);
            key[k] = sIdx <= maxSV ? (idx[k] << 8) | (255u - sIdx) : 0u;
            S.keys[sIdx] = key[k];
            pos[k] = 0;
        }
        for (u32 i = lane; i < kSortScratchNode; i += 64) { Node z; z.count = 0; z.parent = 0; z.byte = 0; z.nbBits = 0; L.nodes[i] = z; }
        // extents of the log2 buckets, for huf_sort_bucket: lane t keeps the number of symbols whose index is >= 164 + t
        u32 ge = 0;
#pragma unroll
        for (u32 t = 0; t < 27; ++t) {
            const u32 n = popc64(ballot(idx[0] >= 164 + t)) + popc64(ballot(idx[1] >= 164 + t)) + popc64(ballot(idx[2] >= 164 + t)) + popc64(ballot(idx[3] >= 164 + t));
            if (lane == t) ge = n;
        }
        wave_lds_sync();
        {
            const uint4* k4 = reinterpret_cast<const uint4*>(S.keys);
            const u32 nQuad = (maxSV >> 2) + 1;
            for (u32 i = 0; i < nQuad; ++i) {          // (every lane reads the same four keys)
                const uint4 o = k4[i];
#pragma unroll
                for (u32 k = 0; k < 4; ++k) pos[k] += (u32)(o.x > key[k]) + (u32)(o.y > key[k]) + (u32)(o.z > key[k]) + (u32)(o.w > key[k]);
            }
        }
        wave_lds_sync();                               // (the keys are read: their storage becomes the quicksort stacks)
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            const u32 sIdx = k * 64 + lane;
            if (sIdx <= maxSV) { Node nd; nd.count = cnt[k]; nd.parent = 0; nd.byte = (u8)sIdx; nd.nbBits = 0; L.nodes[1 + pos[k]] = nd; }
        }
        if (lane < 27) S.rankGe[lane] = (u16)ge;
        wave_lds_sync();
        ZMI_HSTAMP(1);
        if (lane < 26) huf_sort_bucket(L.nodes, S, lane);      // HUF_sort's per-bucket quicksorts, one bucket per lane
        wave_lds_sync();
        ZMI_HSTAMP(2);
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            const u32 pos = k * 64 + lane;
            Node z; z.count = 0; z.parent = 0; z.byte = 0; z.nbBits = 0;
            L.nodes[257 + pos] = z;
            L.nbBits[pos] = 0;
        }
        if (lane < 13) L.wcount[lane] = 0;
        wave_lds_sync();
        Node* huffNode = L.nodes + 1;
        if (lane == 0) { int root = 0; L.sh[kShNonNull] = (u32)huf_build_tree(huffNode, maxSV, &root); L.sh[kShRoot] = (u32)root; }
        wave_lds_sync();
        ZMI_HSTAMP(3);
        const u32 nonNull = L.sh[kShNonNull], root = L.sh[kShRoot];
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {   // depth of every leaf = number of parent links up to the root (HUF_buildTree's nbBits loops)
            const u32 pos = k * 64 + lane;
            if (pos <= nonNull) { u32 node = pos, d = 0; while (node != root) { node = huffNode[node].parent; d++; } huffNode[pos].nbBits = (u8)d; }
        }
        wave_lds_sync();
        ZMI_HSTAMP(4);
        {
            u32 hl = fse_optimal_table_log(11, litSize, maxSV, 1);
            hl = huf_set_max_height_wave(L, huffNode, nonNull, hl);
            // HUF_buildCTableFromTree: symbols per length, then the first code value of every length
            u32 nbPerRank[13];
            {
                u32 nbk[4];
#pragma unroll
                for (u32 k = 0; k < 4; ++k) { const u32 pos = k * 64 + lane; nbk[k] = pos <= nonNull ? huffNode[pos].nbBits : 0xFFu; }
#pragma unroll
                for (u32 r = 0; r < 13; ++r) nbPerRank[r] = popc64(ballot(nbk[0] == r)) + popc64(ballot(nbk[1] == r)) + popc64(ballot(nbk[2] == r)) + popc64(ballot(nbk[3] == r));
            }
            if (lane == 0) {
                u32 mn = 0;
#pragma unroll
                for (int r = 12; r > 0; r--) { if (r <= (int)hl) { L.valPerRank[r] = mn; mn += nbPerRank[r]; mn >>= 1; } }
                L.valPerRank[0] = 0;
                L.sh[kShHuffLog] = hl;
            }
        }
        wave_lds_sync();
        ZMI_HSTAMP(5);
        huffLog = L.sh[kShHuffLog];
#pragma unroll
        for (u32 k = 0; k < 4; ++k) { const u32 pos = k * 64 + lane; if (pos <= maxSV) L.nbBits[huffNode[pos].byte] = huffNode[pos].nbBits; }   // HUF_buildCTableFromTree
        wave_lds_sync();
        {   // canonical codes: symbols of one length get consecutive values in symbol order (U/HufCompress.cs:766-785)
            u32 nb[4], pre[4];
#pragma unroll
            for (u32 k = 0; k < 4; ++k) { const u32 sIdx = k * 64 + lane; nb[k] = sIdx <= maxSV ? L.nbBits[sIdx] : 0; pre[k] = 0; }
            for (u32 r = 1; r <= 12; r++) {
                u32 acc = 0;
#pragma unroll
                for (u32 k = 0; k < 4; ++k) {
                    const u64 b = ballot(nb[k] == r);
                    if (nb[k] == r) pre[k] = acc + popc64(b & lanemask_lt());
                    acc += popc64(b);
                }
            }
#pragma unroll
            for (u32 k = 0; k < 4; ++k) {
                const u32 sIdx = k * 64 + lane;
                const u32 code = nb[k] ? L.valPerRank[nb[k]] + pre[k] : 0;
                T->nbBits[sIdx] = (u8)nb[k]; T->code[sIdx] = (u16)code;
                if (sIdx < maxSV) { const u32 wt = nb[k] ? huffLog + 1 - nb[k] : 0; L.weights[sIdx] = (u8)wt; atomicAdd(&L.wcount[wt], 1u); }   // HUF_writeCTable_wksp's bitsToWeight + the weights' histogram
            }
            // stream sizes = sum(count x nbBits) per segment (HUF_compress1X_usingCTable_internal + HUF_closeCStream)
#pragma unroll
            for (u32 w = 0; w < 4; ++w) {
                u32 bits = 0;
#pragma unroll
                for (u32 k = 0; k < 4; ++k) bits += hst[w][k] * nb[k];
                streamBits[w] = wave_sum(bits);
            }
        }
        wave_lds_sync();
        ZMI_HSTAMP(6);
    }
    u32 wsWave = 0;
    if (shCompressed) wsWave = huf_compress_weights_wave(L, T->hdr + 1, maxSV, lane);      // (uniform branch, uniform result)
    if (!DICT && tid != 0) return;      // (DICT: every lane takes the same decisions, lane 0 stores them, the wave copies the table)
    const bool lead = !DICT || tid == 0;

    // ---------------- remaining serial section: tree description + decisions ----------------
    bool compressed = shCompressed != 0;
    const bool rle = shRle != 0;
    u32 hSize = 0, cLitSize = 0;
    u32 streamSize[4] = { 0, 0, 0, 0 };
    if (compressed) {
        if (lead) { T->maxSV = maxSV; T->tableLog = huffLog; }
        const u32 ws = wsWave;
        if (ws > 1 && ws < maxSV / 2) { if (lead) T->hdr[0] = (u8)ws; hSize = ws + 1; }
        else if (maxSV > 128) { compressed = false; }     // HUF_writeCTable_wksp fails -> ZSTD_compressLiterals stores raw
        else {
            if (lead) {
                T->hdr[0] = (u8)(128 + (maxSV - 1));
                L.weights[maxSV] = 0;
                for (u32 n = 0; n < maxSV; n += 2) T->hdr[(n / 2) + 1] = (u8)((L.weights[n] << 4) + L.weights[n + 1]);
            }
            hSize = ((maxSV + 1) / 2) + 1;
        }
        if (DICT && compressed && oldUsable) {      // the old table unless the new one pays for its description (HUF_estimateCompressedSize: bits >> 3)
            const u32 oldSize = (dictBits[0] + dictBits[1] + dictBits[2] + dictBits[3]) >> 3;
            const u32 newSize = (streamBits[0] + streamBits[1] + streamBits[2] + streamBits[3]) >> 3;
            if (oldSize <= hSize + newSize || hSize + 12 >= litSize) useOld = true;
        }
        if (compressed && !(DICT && useOld) && hSize + 12 >= litSize) compressed = false;
    }
    if (DICT && useOld) {
        compressed = true; hSize = 0;
#pragma unroll
        for (u32 w = 0; w < 4; w++) streamBits[w] = dictBits[w];
    }
    if (compressed) {
        if (single) {
            const u32 bits = streamBits[0] + streamBits[1] + streamBits[2] + streamBits[3];
            streamSize[0] = (bits >> 3) + 1;
            cLitSize = hSize + streamSize[0];
        } else {
            if (litSize < 12) compressed = false;
            cLitSize = hSize + 6;
#pragma unroll
            for (u32 w = 0; w < 4; w++) {
                streamSize[w] = (streamBits[w] >> 3) + 1;
                if (streamSize[w] > 65535) compressed = false;    // (a zero-length stream cannot occur: the end mark is a byte)
                cLitSize += streamSize[w];
            }
        }
        if (compressed && cLitSize >= litSize - 1) compressed = false;                     // HUF_compressCTable_internal
        if (compressed && cLitSize >= litSize - min_gain(litSize)) compressed = false;     // ZSTD_compressLiterals
    }
    if (lead) {
        if (compressed) {
            store_section((DICT && useOld) ? kLitTreeless : kLitCompressed, lhSize, lhSize + cLitSize);
            mOut->litSingle = single; mOut->hufHdrSize = hSize;
            mOut->streamSize[0] = streamSize[0]; mOut->streamSize[1] = streamSize[1]; mOut->streamSize[2] = streamSize[2]; mOut->streamSize[3] = streamSize[3];
        } else if (rle) {
            store_section(kLitRle, lhSizeRaw, lhSizeRaw + 1); mOut->rleByte = shRleByte;
        } else {
            store_section(kLitRaw, lhSizeRaw, lhSizeRaw + litSize);
        }
    }
    if (DICT && useOld && compressed) {     // huf_encode_kernel reads the chunk's table as ever
#pragma unroll
        for (u32 k = 0; k < 4; ++k) { const u32 sIdx = k * 64 + lane; T->nbBits[sIdx] = dct->hufNbBits[sIdx]; T->code[sIdx] = dct->hufCode[sIdx]; }
    }
    ZMI_HSTAMP(7);
#ifdef ZMI_LZ_STAMPS
    if (tid == 0) for (int i = 1; i < 10; i++) atomicAdd(&g_hufStamps[i], stampAcc[i]);
#endif
}

#ifdef ZMI_LZ_STAMPS
extern "C" void ZSTDMI_debugReadHufStamps(unsigned long long* out16, int reset)
{
    (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_hufStamps), 16 * sizeof(unsigned long long));
    if (reset) { unsigned long long z[16] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_hufStamps), z, sizeof z); }
}
#endif

// ------------------------------------------------------------------------------------------------
constexpr u32 kSymPerLane = 16;
constexpr u32 kTileSyms   = 64 * kSymPerLane;             // 1024 symbols per wave step, <= 11264 bits
// 11264 bits behind at most 31 carried ones end in dword 352; a lane ORs four dwords per half whatever they hold, the last of
// them at most three dwords further: 356, a whole number of 16-byte pieces (the tile is zeroed in those)
constexpr u32 kTileWords  = 356;
static_assert((31 + kTileSyms * 11) / 32 + 3 < kTileWords && kTileWords % 4 == 0 && kTileWords <= 128 * 4, "tile holds every OR; zeroed in two 16-byte stores per lane");
static_assert((31 + kTileSyms * 11) / 32 <= 6 * 64, "a tile is flushed in at most six stores per lane");

struct alignas(16) HufEncLds {
    u32 ct[256];                       // nbBits | code << 8: a sum of entries keeps the sum of the lengths in its low byte (16 x 11 = 176),
                                       // and a shift takes its count from the low bits of an entry or of such a sum as it is
    u32 tile[4][kTileWords];
};
typedef u32 u32x4u __attribute__((ext_vector_type(4), aligned(1)));     // one unaligned global_load_dwordx4

// inclusive prefix sum across the wave without LDS: four steps inside the rows of 16 lanes (row_shr 1, 2, 4, 8: a lane without a
// source keeps the 0), then the total of row 0 / 2 into row 1 / 3 (row_bcast:15) and that of rows 0-1 into rows 2-3 (row_bcast:31)
__device__ __forceinline__ u32 wave_scan_incl_dpp(u32 v)
{
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
    return v;
}

// One tile of a stream: the lane's 16 symbols are the reversed indices kb .. kb + 15, i.e. the source bytes len - 1 - kb downwards,
// which `pack` holds in descending order (byte 15 first) when all 16 are in range.  FULL: every lane's are (k0 + kTileSyms <= len):
// no test per symbol.  Otherwise a lane whose 16 straddle the stream's start reads them byte by byte, and lanes behind it add nothing.
template <bool FULL>
__device__ __forceinline__ void huf_encode_tile(const u32* __restrict__ ct, u32* __restrict__ tile, const u8* __restrict__ sym, const u32 len,
                                                const u32 kb, const uint4 pack, uint4& packNext, const u32 lane, u8* __restrict__ out,
                                                u32& carry, u32& carryBits, u32& outWords)
{
    {
        uint4* z4 = reinterpret_cast<uint4*>(tile);
        z4[lane] = make_uint4(0u, 0u, 0u, 0u);
        if (lane < kTileWords / 4 - 64) z4[64 + lane] = make_uint4(0u, 0u, 0u, 0u);
    }
    const u32 d[4] = { pack.x, pack.y, pack.z, pack.w };
    const bool full16 = FULL || kb + kSymPerLane <= len;
    u32 e[kSymPerLane];
#pragma unroll
    for (u32 j = 0; j < kSymPerLane; j++) {
        u32 s8 = (d[3 - (j >> 2)] >> (8 * (3 - (j & 3)))) & 0xFFu;
        if (FULL) e[j] = ct[s8];
        else {
            const u32 k = kb + j;
            if (!full16) s8 = k < len ? (u32)sym[len - 1 - k] : 0u;
            e[j] = k < len ? ct[s8] : 0u;
        }
    }
    // codes are at most 11 bits: two fit 32 bits (one shift-or), four fit 64, eight need 88.  The two halves of the lane go to the
    // tile separately: joining them would cost more shifts than the OR it saves.
    u32 p[8], ps[8];
#pragma unroll
    for (u32 i = 0; i < 8; i++) { const u32 a = e[2 * i], b = e[2 * i + 1]; p[i] = ((b >> 8) << (a & 31u)) | (a >> 8); ps[i] = a + b; }
    u64 q[4]; u32 qs[4];
#pragma unroll
    for (u32 i = 0; i < 4; i++) { q[i] = (u64)p[2 * i] | ((u64)p[2 * i + 1] << (ps[2 * i] & 63u)); qs[i] = ps[2 * i] + ps[2 * i + 1]; }
    u64 lo[2]; u32 hi[2], hs[2];
#pragma unroll
    for (u32 h = 0; h < 2; h++) {
        const u32 t = qs[2 * h];                                       // <= 44 in its low byte
        lo[h] = q[2 * h] | (q[2 * h + 1] << (t & 63u));
        hi[h] = (u32)((q[2 * h + 1] >> 1) >> (~t & 63u));              // >> (64 - t), also right for t = 0
        hs[h] = qs[2 * h] + qs[2 * h + 1];
    }
    const u32 nb0 = hs[0] & 0xFFu, nb = (hs[0] + hs[1]) & 0xFFu;
    const u32 incl = wave_scan_incl_dpp(nb);
    const u32 tileBits = read_lane(incl, 63);
    const u32 bitOff = carryBits + incl - nb;
#pragma unroll
    for (u32 h = 0; h < 2; h++) {
        // up to 88 bits shifted by < 32: four dwords; a zero ORs nothing, so none of them is tested
        const u32 at = h ? bitOff + nb0 : bitOff;
        const u32 w0 = at >> 5, sh = at & 31u;
        const u64 a0 = lo[h] << sh;
        const u64 a1 = (((u64)hi[h] << 32) | (lo[h] >> 32)) << sh;
        const u64 a2 = (u64)hi[h] << sh;
        atomicOr(&tile[w0], (u32)a0);
        atomicOr(&tile[w0 + 1], (u32)(a0 >> 32));
        atomicOr(&tile[w0 + 2], (u32)(a1 >> 32));
        atomicOr(&tile[w0 + 3], (u32)(a2 >> 32));
    }
    if (lane == 0 && carryBits) atomicOr(&tile[0], carry);
    const u32 total = carryBits + tileBits;
    const u32 fullWords = total >> 5;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // The next tile's symbols, on their way since the top of this tile, are waited for HERE: loads and stores share one in-order
    // counter, so waiting for them at the top of the next tile would also wait until the stores below have reached L2.
    if (FULL) asm volatile("" : "+v"(packNext.x), "+v"(packNext.y), "+v"(packNext.z), "+v"(packNext.w));
#pragma unroll
    for (u32 r = 0; r < 6; ++r) { const u32 i = lane + 64 * r; if (i < fullWords) *(u32u*)(out + 4 * (outWords + i)) = tile[i]; }
    carry = tile[fullWords]; carryBits = total & 31;       // every lane reads the same LDS word
    outWords += fullWords;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// `dst` != nullptr: the literals section goes straight to its final place in the output (offsets[] from the scan; the
// sequences section and the headers follow through gather_kernel); nullptr: into the chunk's slot (test hook).
// DICT: a kLitTreeless chunk is coded like a compressed one — its table is the dictionary's, copied by huf_tree_kernel<true> — under
// literals type 3 and without a tree description; its single stream may hold up to 1023 symbols (less than one tile).  Without
// DICT such a record is not expected and stored raw, as any unknown mode.
template <bool DICT>
__global__ __launch_bounds__(256) void huf_encode_kernel(const u8* __restrict__ lits, const ChunkMeta* __restrict__ meta,
                                                         const HufTable* __restrict__ tables, u8* __restrict__ slots,
                                                         u8* __restrict__ dst, const u64* __restrict__ offsets, u64 dstCapacity,
                                                         const u8* __restrict__ src, const u32 chunkBytes)
{
    __shared__ HufEncLds L;
    const u32 c = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = uniform(wave_id());
    // (the table entry is fetched beside the chunk's record, not behind it: the chunk's table exists whatever the literals' mode)
    const HufTable* __restrict__ T = tables + c;
    const u32 ctEntry = (u32)T->nbBits[tid] | ((u32)T->code[tid] << 8);
    const ChunkMeta m = meta_checked(meta[c]);
    const u32 litSize = m.litSize;
    const u8* __restrict__ lit = m.litFromSrc ? src + (u64)c * chunkBytes : lits + (u64)c * kLitStride;
    u8* __restrict__ body = slots + (u64)c * kSlotStride + m.fhSize + 3;      // block body starts after frame + block header
    if (dst) {
        if (m.blockType != 2) return;                                        // stored raw: gather copies the source bytes
        const u64 off = offsets[c];
        if (off + m.outSize > dstCapacity) return;                           // host reports dstSize_tooSmall from the scanned total
        body = dst + off + m.fhSize + 3;
    }

    const bool treeless = DICT && m.litMode == kLitTreeless;
    if (m.litMode != kLitCompressed && !treeless) {
        // ZSTD_noCompressLiterals / ZSTD_compressRleLiteralsBlock (U/ZstdCompressLiterals.cs:8-83)
        const u32 type = m.litMode == kLitRle ? 1u : 0u;
        if (tid == 0) {
            switch (m.lhSize) {
            case 1: body[0] = (u8)(type + (litSize << 3)); break;
            case 2: writeLE16(body, type + (1u << 2) + (litSize << 4)); break;
            default: writeLE24(body, type + (3u << 2) + (litSize << 4)); break;
            }
            if (type == 1) body[m.lhSize] = (u8)m.rleByte;
        }
        if (type == 0) for (u32 i = tid; i < litSize; i += 256) body[m.lhSize + i] = lit[i];
        return;
    }
    L.ct[tid] = ctEntry;
    // the stream of this wave; its first symbols are on their way while the headers are written
    const u32 nStreams = m.litSingle ? 1 : 4;
    const u32 seg = m.litSingle ? litSize : (litSize + 3) / 4;
    const u32 s0 = wave * seg;
    const u32 len = uniform(wave >= nStreams ? 0u : (wave == nStreams - 1) ? litSize - s0 : seg);
    const u8* __restrict__ sym = lit + s0;
    auto load_pack = [&](u32 k0) -> uint4 {
        const u32 kb = k0 + lane * kSymPerLane;
        if (kb + kSymPerLane > len) return make_uint4(0u, 0u, 0u, 0u);
        const u32x4u v = *reinterpret_cast<const u32x4u*>(sym + (len - kSymPerLane - kb));
        return make_uint4(v.x, v.y, v.z, v.w);
    };
    uint4 packNext = load_pack(0);
    if (tid == 0) {
        const u32 cLitSize = m.litSectionSize - m.lhSize;
        const u32 hType = treeless ? 3u : 2u;
        switch (m.lhSize) {       // ZSTD_compressLiterals header (U/ZstdCompressLiterals.cs:150-182)
        case 3: writeLE24(body, hType + ((m.litSingle ? 0u : 1u) << 2) + (litSize << 4) + (cLitSize << 14)); break;
        case 4: writeLE32(body, hType + (2u << 2) + (litSize << 4) + (cLitSize << 18)); break;
        default: writeLE32(body, hType + (3u << 2) + (litSize << 4) + (cLitSize << 22)); body[4] = (u8)(cLitSize >> 10); break;
        }
    }
    const u32 hufHdrSize = treeless ? 0u : m.hufHdrSize;
    for (u32 i = tid; i < hufHdrSize; i += 256) body[m.lhSize + i] = T->hdr[i];
    u8* payload = body + m.lhSize + hufHdrSize;
    if (!m.litSingle && tid < 3) writeLE16(payload + 2 * tid, meta[c].streamSize[tid]);       // jump table
    __syncthreads();

    if (wave >= nStreams) return;
    u8* out = payload + (m.litSingle ? 0 : 6);
    for (u32 w = 0; w < wave; w++) out += meta[c].streamSize[w];
    u32* tile = L.tile[wave];

    u32 carry = 0, carryBits = 0;        // bits of a partially filled dword carried into the next tile
    u32 outWords = 0;                    // dwords already flushed to `out`
    // The lane's 16 symbols of a tile sit in 16 consecutive bytes (descending): one unaligned 16-byte load when all are in range —
    // issued a tile AHEAD (its way from HBM was the longest part of a tile's time); the tile belongs to this wave alone, so its LDS
    // traffic needs program order only (a wavefront fence: the workgroup fences that stood here waited for every store to reach
    // L2, twice per tile).  Whole tiles run the body without a test per symbol; what is left of the stream — or all of a stream
    // shorter than a tile — runs the general body once.
    asm volatile("" : "+v"(packNext.x), "+v"(packNext.y), "+v"(packNext.z), "+v"(packNext.w));     // (so that the loop never waits at its top: see the flush)
    u32 k0 = 0;
    for (; k0 + kTileSyms <= len; k0 += kTileSyms) {
        const uint4 pack = packNext;
        {   // (no branch around the load: a lane whose next 16 are not all there reads the stream's first 16 and never uses them)
            const u32 kn = k0 + kTileSyms + lane * kSymPerLane;
            const u32x4u v = *reinterpret_cast<const u32x4u*>(sym + (kn + kSymPerLane <= len ? len - kSymPerLane - kn : 0u));
            packNext = make_uint4(v.x, v.y, v.z, v.w);
        }
        huf_encode_tile<true>(L.ct, tile, sym, len, k0 + lane * kSymPerLane, pack, packNext, lane, out, carry, carryBits, outWords);
    }
    if (k0 < len) huf_encode_tile<false>(L.ct, tile, sym, len, k0 + lane * kSymPerLane, packNext, packNext, lane, out, carry, carryBits, outWords);
    if (lane == 0) {       // end mark + tail bytes (HUF_closeCStream, U/HufCompress.cs:964-979)
        u32 v = carry | (1u << carryBits);
        const u32 nbytes = (carryBits + 1 + 7) >> 3;
        u8* p = out + 4 * outWords;
        for (u32 i = 0; i < nbytes; i++) { p[i] = (u8)v; v >>= 8; }
    }
}

// dct != nullptr: the first block of every frame (frames as in seq_encode) may reuse the dictionary's table; a dictionary's framing
// counts the blocks of a frame by the chunk's index
void launch_huf_build(const u8* lits, ChunkMeta* meta, HufTable* tables, u8* slots, u32 nChunks, u32 rawLiterals, const u8* src, const FrameLayout& frames,
                      hipStream_t stream, StageHook hook, const DictCTables* dct, const CDictSlot* dictSlots, const u32* chunkSlot)
{
    assert((!dct && !dictSlots) || frames.form == kArith);
    assert(!dictSlots == !chunkSlot);
    // (a set pass: dct != null says that one of its slots has tables — the short-literal histograms are wanted — and is not read)
    const u32 chunkBytes = frames.chunkBytes, frameBlocks = frames.frameBlocks;
    // a throughput kernel: a wave per (chunk, stream) item while that keeps every CU's share short, several items per wave beyond
    const u32 nItems = 4 * nChunks, perWave = (nItems + kHistItemsPerWave - 1) / kHistItemsPerWave;
    const u32 grid = nItems <= kHistMinGrid ? nItems : (perWave > kHistMinGrid ? perWave : kHistMinGrid);
    if (dct) hipLaunchKernelGGL(huf_hist_kernel<6>, dim3(grid), dim3(64), 0, stream, lits, meta, slots, rawLiterals, src, chunkBytes, nItems);
    else hipLaunchKernelGGL(huf_hist_kernel<63>, dim3(grid), dim3(64), 0, stream, lits, meta, slots, rawLiterals, src, chunkBytes, nItems);
    hook("huf_hist");
    if (dictSlots && dct) hipLaunchKernelGGL((huf_tree_kernel<true, true>), dim3(nChunks), dim3(64), 0, stream, meta, tables, slots, rawLiterals, dct, frameBlocks, dictSlots, chunkSlot);
    else if (dct) hipLaunchKernelGGL((huf_tree_kernel<true>), dim3(nChunks), dim3(64), 0, stream, meta, tables, slots, rawLiterals, dct, frameBlocks, dictSlots, chunkSlot);
    else hipLaunchKernelGGL((huf_tree_kernel<false>), dim3(nChunks), dim3(64), 0, stream, meta, tables, slots, rawLiterals, dct, frameBlocks, dictSlots, chunkSlot);
    hook("huf_tree");
}
void launch_huf_encode(const u8* lits, const ChunkMeta* meta, const HufTable* tables, u8* slots, u8* dst, const u64* offsets, u64 dstCapacity,
                       u32 nChunks, const u8* src, u32 chunkBytes, hipStream_t stream, bool dictEntropy)
{
    if (dictEntropy) hipLaunchKernelGGL(huf_encode_kernel<true>, dim3(nChunks), dim3(256), 0, stream, lits, meta, tables, slots, dst, offsets, dstCapacity, src, chunkBytes);
    else hipLaunchKernelGGL(huf_encode_kernel<false>, dim3(nChunks), dim3(256), 0, stream, lits, meta, tables, slots, dst, offsets, dstCapacity, src, chunkBytes);
}

// ---- the entropy tables of a trained dictionary (ZDICT_analyzeEntropy, U/Zdict.cs:174-408), one wave ----
// In: the statistics (every count >= 1): [0, 256) literals, [256, 292) LL codes, [292, 345) ML codes, [345, 345 + offcodeMax]
// offset codes.  Out: Huffman table description (maxNbBits 11, the ZDICT_flatLit retry when the build returns 8), the offset /
// match-length / literal-length FSE descriptions (logs 8 / 9 / 9, low-probability counts, the offset one written with
// maxSymbolValue 30), and the repcodes {1, 4, 8}.  *outSize = bytes written,
// 0 when the literal table cannot be described (HUF_writeCTable fails), 0xFFFFFFFF when the tables exceed `cap`.
__global__ __launch_bounds__(64) void dict_entropy_kernel(const u32* __restrict__ stats, u32 offcodeMax, u8* __restrict__ out, u32 cap,
                                                          u32* __restrict__ outSize)
{
    __shared__ HufTreeLds L;
    __shared__ u32 cnt[256];
    __shared__ u8 hdr[512];
    const u32 lane = threadIdx.x;
    for (u32 k = 0; k < 4; ++k) cnt[k * 64 + lane] = stats[k * 64 + lane];
    wave_lds_sync();
    u32 huffLog = 0, ws = 0;
    for (u32 attempt = 0; attempt < 2; ++attempt) {
        if (lane == 0) {                                    // HUF_sort: counts in descending order (ties in symbol order)
            Node z; z.count = 0; z.parent = 0; z.byte = 0; z.nbBits = 0;
            for (u32 i = 0; i < 513; i++) L.nodes[i] = z;
            for (u32 s = 0; s < 256; s++) {
                Node nd; nd.count = cnt[s]; nd.parent = 0; nd.byte = (u8)s; nd.nbBits = 0;
                int j = (int)s;
                while (j > 0 && L.nodes[j].count < nd.count) { L.nodes[j + 1] = L.nodes[j]; j--; }
                L.nodes[j + 1] = nd;
            }
        }
        if (lane < 13) L.wcount[lane] = 0;
        wave_lds_sync();
        Node* huffNode = L.nodes + 1;
        if (lane == 0) { int root = 0; L.sh[kShNonNull] = (u32)huf_build_tree(huffNode, 255, &root); L.sh[kShRoot] = (u32)root; }
        wave_lds_sync();
        const u32 nonNull = L.sh[kShNonNull], root = L.sh[kShRoot];
        for (u32 k = 0; k < 4; ++k) {
            const u32 pos = k * 64 + lane;
            if (pos <= nonNull) { u32 node = pos, d = 0; while (node != root) { node = huffNode[node].parent; d++; } huffNode[pos].nbBits = (u8)d; }
        }
        wave_lds_sync();
        const u32 hl = uniform(huf_set_max_height_wave(L, huffNode, nonNull, 11));
        wave_lds_sync();
        if (hl == 8 && attempt == 0) {                      // ZDICT_flatLit: a flat distribution HUF_writeCTable can describe
            for (u32 k = 0; k < 4; ++k) { const u32 s = k * 64 + lane; cnt[s] = s == 0 ? 4u : (s == 253 || s == 254) ? 1u : 2u; }
            wave_lds_sync();
            continue;
        }
        for (u32 k = 0; k < 4; ++k) { const u32 pos = k * 64 + lane; L.nbBits[huffNode[pos].byte] = huffNode[pos].nbBits; }
        wave_lds_sync();
        for (u32 k = 0; k < 4; ++k) {
            const u32 s = k * 64 + lane;
            if (s < 255) { const u32 nb = L.nbBits[s]; const u32 wt = nb ? hl + 1 - nb : 0; L.weights[s] = (u8)wt; atomicAdd(&L.wcount[wt], 1u); }
        }
        wave_lds_sync();
        ws = huf_compress_weights_wave(L, hdr + 1, 255, lane);
        huffLog = hl;
        break;
    }
    if (lane != 0) return;
    if (!huffLog || !(ws > 1 && ws < 255 / 2)) { *outSize = 0; return; }
    hdr[0] = (u8)ws;
    u32 pos = ws + 1;
    u32 count[53]; s16 norm[53]; u32 total = 0;
    // offset codes 0..offcodeMax, written up to maxSymbolValue 30
    for (u32 s = 0; s < 53; s++) { count[s] = s <= offcodeMax ? stats[345 + s] : 0u; norm[s] = 0; total += count[s]; }
    fse_normalize_count(norm, 8, count, total, offcodeMax, 1);
    pos += fse_write_ncount(hdr + pos, norm, 30, 8);
    total = 0; for (u32 s = 0; s < 53; s++) { count[s] = stats[292 + s]; total += count[s]; }
    fse_normalize_count(norm, 9, count, total, 52, 1);
    pos += fse_write_ncount(hdr + pos, norm, 52, 9);
    total = 0; for (u32 s = 0; s < 36; s++) { count[s] = stats[256 + s]; total += count[s]; }
    fse_normalize_count(norm, 9, count, total, 35, 1);
    pos += fse_write_ncount(hdr + pos, norm, 35, 9);
    if (pos + 12 > cap) { *outSize = 0xFFFFFFFFu; return; }
    writeLE32(hdr + pos, 1); writeLE32(hdr + pos + 4, 4); writeLE32(hdr + pos + 8, 8);
    pos += 12;
    for (u32 i = 0; i < pos; i++) out[i] = hdr[i];
    *outSize = pos;
}

void launch_dict_entropy(const u32* stats, u32 offcodeMax, u8* out, u32 cap, u32* outSize, hipStream_t stream)
{
    hipLaunchKernelGGL(dict_entropy_kernel, dim3(1), dim3(64), 0, stream, stats, offcodeMax, out, cap, outSize);
}

} // namespace zmi
