// dict_train.hip — dictionary training (ZDICT_trainFromBuffer and the fastCover trainer behind it, U/Fastcover.cs, U/Cover.cs,
// U/Zdict.cs) on gfx950.
//
//   dt_hash       the f-bit hash (ZSTD_hash8Ptr / ZSTD_hash6Ptr) of every dmer position of the training samples
//   dt_freq       FASTCOVER_computeFrequency: the positions a sample's dmers start at (accel's skip), atomically counted
//   dt_occ        for every position, the distance to the previous and to the next position with the same hash (capped at the
//                 largest window of the call).  Within one epoch the frequencies are constant, so the reference's sliding window
//                 (FASTCOVER_selectSegment) becomes a scan: the dmer entering at p adds its frequency iff its hash does not occur
//                 in the W positions before it (inside the epoch), the dmer leaving at b = p - W removes it iff its hash does not
//                 occur in (b, p].  Both tests are these distances.
//   dt_select     one persistent workgroup per k candidate runs FASTCOVER_buildDictionary's whole epoch loop on its own copy
//                 of the frequencies: a block-wide u32 prefix scan of the terms per epoch, the first step that reaches the
//                 epoch's maximum (the reference's strict >), the segment's hashes zeroed, its bytes copied to the tail.
// Finalize (ZDICT_analyzeEntropy) compresses every finalize sample on its own against the content as a raw dictionary with this
// library's compressor, in one batch (compress_samples, zstd_mi355x.hip), and seq_stats_kernel histograms the literals and the
// LL / ML / offset codes of the blocks that came out compressed; dict_entropy_kernel (huf_enc.hip) writes the tables.  Scoring a k
// (COVER_checkTotalCompressedSize) compresses the test samples with the finalized dictionary in one batch the same way.
// The dictionary content for given (k, d, f, accel, splitPoint) is byte-identical to the reference's; the entropy tables and the k
// choice follow this library's compressor, not the reference's parser.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include <new>
#include "zmi_common.h"
#include "zmi_device.h"
#include "../../include/zstd_mi355x.h"
#include "zmi_host.h"

namespace zmi {

void launch_dict_entropy(const u32* litCount, u32 offcodeMax, u8* out, u32 cap, u32* outSize, hipStream_t stream);

constexpr u32 kNoOcc = 0xFFFFFFFFu;
constexpr u32 kOccTile = 1024;          // positions per workgroup of dt_occ (256 lanes x 4)
constexpr u32 kOccChunk = 4096;         // hashes staged in LDS per step of dt_occ
constexpr u32 kSelThreads = 1024;
constexpr u32 kSelItems = 4;            // consecutive positions per lane of dt_select
constexpr u32 kMaxCandidates = 64;

__device__ __forceinline__ u64 load_le64_bytes(const u8* p)
{
    u64 v = 0;
#pragma unroll
    for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
    return v;
}

__global__ __launch_bounds__(256) void dt_hash_kernel(const u8* __restrict__ samples, u32 nbDmers, u32 f, u32 d, u32* __restrict__ hashes)
{
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nbDmers) return;
    const u64 w = load_le64_bytes(samples + p);                              // p + 8 <= trainingSize
    hashes[p] = d == 6 ? (u32)(((w << 16) * 227718039650203ull) >> (64 - f))       // ZSTD_hash6Ptr
                       : (u32)((w * 0xCF1BBCDCB7A56463ull) >> (64 - f));          // ZSTD_hash8Ptr
}

// offsets[0..nbTrain] are the training samples' starts; a position counts if it is a dmer start of its sample
__global__ __launch_bounds__(256) void dt_freq_kernel(const u32* __restrict__ hashes, const u64* __restrict__ offsets, u32 nbTrain,
                                                      u32 nbDmers, u32 step, u32* __restrict__ freqs)
{
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nbDmers) return;
    u32 lo = 0, hi = nbTrain;                                                // largest s with offsets[s] <= p
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (offsets[mid] <= p) lo = mid; else hi = mid; }
    if (((u64)p - offsets[lo]) % step == 0 && (u64)p + 8 <= offsets[lo + 1]) atomicAdd(&freqs[hashes[p]], 1u);
}

// prevDist[p] = p - (last q < p with hashes[q] == hashes[p]) if that is <= wmax, else kNoOcc; nextDist likewise forwards
__global__ __launch_bounds__(256) void dt_occ_kernel(const u32* __restrict__ hashes, u32 n, u32 wmax, u32* __restrict__ prevDist,
                                                     u32* __restrict__ nextDist)
{
    __shared__ u32 buf[kOccChunk];
    const u32 t0 = blockIdx.x * kOccTile, tid = threadIdx.x;
    u32 h[4], prev[4], next[4];
#pragma unroll
    for (u32 j = 0; j < 4; ++j) { const u32 p = t0 + j * 256 + tid; h[j] = p < n ? hashes[p] : 0; prev[j] = kNoOcc; next[j] = kNoOcc; }
    const u32 tEnd = t0 + kOccTile < n ? t0 + kOccTile : n;
    // backwards: chunks of [lo, t0 + tile) from the nearest to the farthest
    const u32 lo = t0 > wmax ? t0 - wmax : 0;
    for (u32 cEnd = tEnd; cEnd > lo;) {
        const u32 cBeg = cEnd - lo > kOccChunk ? cEnd - kOccChunk : lo;
        __syncthreads();
        for (u32 i = tid; i < cEnd - cBeg; i += 256) buf[i] = hashes[cBeg + i];
        __syncthreads();
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const u32 p = t0 + j * 256 + tid;
            if (p >= n || prev[j] != kNoOcc || p <= cBeg) continue;
            const u32 qLo = p - cBeg > wmax ? p - wmax : cBeg, qHi = (p < cEnd ? p : cEnd) - 1;
            if (qHi < qLo) continue;                                          // the chunk lies beyond the window
            for (u32 q = qHi;; --q) {
                if (buf[q - cBeg] == h[j]) { prev[j] = p - q; break; }
                if (q == qLo) break;
            }
        }
        cEnd = cBeg;
    }
    // forwards: chunks of [t0, hi) from the nearest to the farthest
    const u32 hi = (u64)tEnd + wmax < n ? tEnd + wmax : n;
    for (u32 cBeg = t0; cBeg < hi;) {
        const u32 cEnd = hi - cBeg > kOccChunk ? cBeg + kOccChunk : hi;
        __syncthreads();
        for (u32 i = tid; i < cEnd - cBeg; i += 256) buf[i] = hashes[cBeg + i];
        __syncthreads();
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const u32 p = t0 + j * 256 + tid;
            if (p >= n || next[j] != kNoOcc || p + 1 >= cEnd) continue;
            const u32 qHi = (u64)p + wmax < cEnd - 1 ? p + wmax : cEnd - 1;
            for (u32 q = p + 1 > cBeg ? p + 1 : cBeg; q <= qHi; ++q)
                if (buf[q - cBeg] == h[j]) { next[j] = q - p; break; }
        }
        cBeg = cEnd;
    }
#pragma unroll
    for (u32 j = 0; j < 4; ++j) { const u32 p = t0 + j * 256 + tid; if (p < n) { prevDist[p] = prev[j]; nextDist[p] = next[j]; } }
}

struct SelCand {
    u32 k, epochNum, epochSize;
    u32 tail;                 // out: FASTCOVER_buildDictionary's return value (content = dict[tail, capacity))
};

__device__ __forceinline__ u64 wave_max64(u64 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}

// FASTCOVER_buildDictionary for candidate blockIdx.x; freqs = its own copy (2^f entries), dict = its `capacity` bytes
__global__ __launch_bounds__(kSelThreads) void dt_select_kernel(const u8* __restrict__ samples, const u32* __restrict__ hashes,
                                                                const u32* __restrict__ prevDist, const u32* __restrict__ nextDist,
                                                                u32* __restrict__ freqAll, u64 freqEntries, u8* __restrict__ dictAll,
                                                                u32 capacity, u32 d, SelCand* __restrict__ cands)
{
    __shared__ u32 waveTot[kSelThreads / 64];
    __shared__ u64 waveBest[kSelThreads / 64];
    SelCand* const C = cands + blockIdx.x;
    u32* const freqs = freqAll + freqEntries * blockIdx.x;
    u8* const dict = dictAll + (u64)capacity * blockIdx.x;
    const u32 k = C->k, num = C->epochNum, size = C->epochSize, W = k - d + 1;
    const u32 tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    u32 tail = capacity, zeroRun = 0, epoch = 0;
    while (tail > 0) {
        const u32 begin = epoch * size, end = begin + size;
        u32 carry = 0, bestScore = 0, bestPos = 0;
        for (u32 t0 = begin; t0 < end; t0 += kSelThreads * kSelItems) {
            u32 term[kSelItems], local = 0;
#pragma unroll
            for (u32 j = 0; j < kSelItems; ++j) {
                const u32 p = t0 + tid * kSelItems + j;
                u32 v = 0;
                if (p < end) {
                    const u32 lim = p - begin < W ? p - begin : W;
                    if (prevDist[p] > lim) v += freqs[hashes[p]];             // entering dmer: first of its hash in the window
                    if (p - begin >= W) {
                        const u32 b = p - W;
                        if (nextDist[b] > W) v -= freqs[hashes[b]];           // leaving dmer: last of its hash in the window
                    }
                }
                local += v; term[j] = local;
            }
            // block-wide exclusive prefix of the lanes' totals
            const u32 incl = wave_scan_incl(local);
            if (lane == 63) waveTot[wave] = incl;
            __syncthreads();
            u32 waveBase = 0, blockTot = 0;
            for (u32 w = 0; w < kSelThreads / 64; ++w) { const u32 t = waveTot[w]; if (w < wave) waveBase += t; blockTot += t; }
            const u32 base = carry + waveBase + incl - local;
            // the first position of this tile that reaches the tile's maximum: key = score << 32 | ~position
            u64 key = 0;
#pragma unroll
            for (u32 j = 0; j < kSelItems; ++j) {
                const u32 p = t0 + tid * kSelItems + j;
                if (p < end) { const u64 kk = ((u64)(base + term[j]) << 32) | (u32)~p; key = kk > key ? kk : key; }
            }
            key = wave_max64(key);
            if (lane == 0) waveBest[wave] = key;
            __syncthreads();
            u64 tileBest = 0;
            for (u32 w = 0; w < kSelThreads / 64; ++w) tileBest = waveBest[w] > tileBest ? waveBest[w] : tileBest;
            const u32 tileScore = (u32)(tileBest >> 32);
            if (tileScore > bestScore) { bestScore = tileScore; bestPos = ~(u32)tileBest; }
            carry += blockTot;
            __syncthreads();                                                  // waveTot / waveBest are reused
        }
        epoch = (epoch + 1) % num;
        if (bestScore == 0) {
            if (++zeroRun >= 10) break;
            continue;
        }
        zeroRun = 0;
        const u32 segEnd = bestPos + 1, segBegin = bestPos + 1 - begin > W ? bestPos + 1 - W : begin;
        // FASTCOVER_selectSegment: zero the frequencies of the segment's dmers
        for (u32 q = segBegin + tid; q < segEnd; q += kSelThreads) freqs[hashes[q]] = 0;
        const u32 want = segEnd - segBegin + d - 1, segSize = want < tail ? want : tail;
        if (segSize < d) break;
        tail -= segSize;
        for (u32 i = tid; i < segSize; i += kSelThreads) dict[tail + i] = samples[segBegin + i];
        __threadfence_block();
        __syncthreads();
    }
    if (tid == 0) C->tail = tail;
}

} // namespace zmi

using namespace zmi;

namespace {

// FASTCOVER_accel_t table (U/Fastcover.cs:24-80): finalize percentage, skip
const u32 kAccelFinalize[11] = { 100, 100, 50, 34, 25, 20, 17, 14, 13, 11, 10 };
const u32 kAccelSkip[11]     = { 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9 };
constexpr u32 kMaxF = 24;               // 2^f u32 frequencies per candidate: 64 MiB each at f = 24

struct DBuf {
    void* p = nullptr;
    ~DBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc(&p, n ? n : 1) == hipSuccess || (p = nullptr, false); }
};

// FASTCOVER_checkParameters (U/Fastcover.cs:175-215)
bool check_parameters(u32 k, u32 d, size_t maxDictSize, u32 f, u32 accel, double splitPoint)
{
    if (d == 0 || k == 0) return false;
    if (d != 6 && d != 8) return false;
    if (k > maxDictSize) return false;
    if (d > k) return false;
    if (f > 31 || f == 0) return false;
    if (splitPoint <= 0 || splitPoint > 1) return false;
    if (accel > 10 || accel == 0) return false;
    return true;
}

// COVER_computeEpochs (U/Cover.cs:58-76)
void compute_epochs(u32 maxDictSize, u32 nbDmers, u32 k, u32* num, u32* size)
{
    const u32 minEpochSize = k * 10;
    *num = maxDictSize / k > 1 ? maxDictSize / k : 1;
    *size = nbDmers / *num;
    if (*size >= minEpochSize) return;
    *size = minEpochSize < nbDmers ? minEpochSize : nbDmers;
    *num = nbDmers / *size;
}

u64 xxh64(const u8* p, size_t len, u64 seed)
{
    const u64 P1 = 11400714785074694791ull, P2 = 14029467366897019727ull, P3 = 1609587929392839161ull, P4 = 9650029242287828579ull,
              P5 = 2870177450012600261ull;
    auto rotl = [](u64 x, int r) { return (x << r) | (x >> (64 - r)); };
    auto rd64 = [](const u8* q) { u64 v; memcpy(&v, q, 8); return v; };
    auto rd32 = [](const u8* q) { uint32_t v; memcpy(&v, q, 4); return (u64)v; };
    auto round = [&](u64 acc, u64 in) { acc += in * P2; acc = rotl(acc, 31); return acc * P1; };
    auto merge = [&](u64 acc, u64 v) { v = round(0, v); acc ^= v; return acc * P1 + P4; };
    const u8* const end = p + len;
    u64 h;
    if (len >= 32) {
        u64 v1 = seed + P1 + P2, v2 = seed + P2, v3 = seed, v4 = seed - P1;
        const u8* const limit = end - 32;
        do { v1 = round(v1, rd64(p)); v2 = round(v2, rd64(p + 8)); v3 = round(v3, rd64(p + 16)); v4 = round(v4, rd64(p + 24)); p += 32; } while (p <= limit);
        h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
        h = merge(h, v1); h = merge(h, v2); h = merge(h, v3); h = merge(h, v4);
    } else h = seed + P5;
    h += (u64)len;
    while (p + 8 <= end) { h ^= round(0, rd64(p)); h = rotl(h, 27) * P1 + P4; p += 8; }
    if (p + 4 <= end) { h ^= rd32(p) * P1; h = rotl(h, 23) * P2 + P3; p += 4; }
    while (p < end) { h ^= (*p) * P5; h = rotl(h, 11) * P1; p++; }
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}

// a device and a stream of the trainer's own (the device a fresh ZSTD_CCtx binds to)
struct Device {
    hipStream_t s = nullptr;
    size_t open()
    {
        if (ZSTDMI_deviceCount() <= 0) return ZERR(kErrInitMissing);
        if (hipSetDevice(0) != hipSuccess) return ZERR(kErrInitMissing);
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { s = nullptr; return ZERR(kErrMemoryAllocation); }
        return 0;
    }
    ~Device() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};

// ZDICT_finalizeDictionary (U/Zdict.cs:458-533) with the statistics of ZDICT_analyzeEntropy taken on the device
size_t finalize(Device& dev, void* dictBuffer, size_t capacity, const void* content, size_t contentSize, const void* samples,
                const size_t* sizes, unsigned nbSamples, unsigned dictIDParam, int level)
{
    if (capacity < contentSize) return ZERR(kErrDstSizeTooSmall);
    if (capacity < 256) return ZERR(kErrDstSizeTooSmall);
    u8 header[256];
    const u32 magic = 0xEC30A437u;
    memcpy(header, &magic, 4);
    const u64 randomID = xxh64((const u8*)content, contentSize, 0);
    const u32 compliantID = (u32)((randomID % ((1u << 31) - 32768)) + 32768);
    const u32 dictID = dictIDParam ? dictIDParam : compliantID;
    memcpy(header + 4, &dictID, 4);
    size_t hSize = 8;
    // ZDICT_analyzeEntropy: offcodeMax from the content size; literal counts start at 1
    const u64 offArg = (u64)contentSize + (128u << 10);
    u32 offcodeMax = 0; for (u64 v = (u32)offArg; v > 1; v >>= 1) offcodeMax++;
    if (offcodeMax > 30) return ZERR(kErrDictionaryCreationFailed);
    // ZDICT_countEStats: every finalize sample (its first 128 KiB) compressed alone against the content as a raw dictionary
    std::vector<u32> stats(377, 0);
    {
        std::vector<u64> offs(nbSamples); std::vector<size_t> cut(nbSamples), out(nbSamples);
        u64 o = 0;
        for (unsigned i = 0; i < nbSamples; i++) { offs[i] = o; cut[i] = sizes[i] < (128u << 10) ? sizes[i] : (128u << 10); o += sizes[i]; }
        ZSTD_CCtx* c = ZSTD_createCCtx();
        if (!c) return ZERR(kErrMemoryAllocation);
        size_t r = ZSTD_CCtx_setParameter(c, ZSTD_c_compressionLevel, level);
        if (!isErr(r)) r = ZSTD_CCtx_loadDictionary(c, content, contentSize);
        if (!isErr(r)) r = compress_samples(c, (const u8*)samples, offs.data(), cut.data(), nbSamples, out.data(), stats.data());
        ZSTD_freeCCtx(c);
        if (isErr(r)) return r;
    }
    for (u32 i = 0; i < 256; i++) stats[i] += 1;                                   // every count starts at 1
    for (u32 i = 0; i < 36; i++) stats[256 + i] += 1;
    for (u32 i = 0; i < 53; i++) stats[292 + i] += 1;
    for (u32 i = 0; i <= offcodeMax; i++) stats[345 + i] += 1;
    DBuf dCount, dOut;
    if (!dCount.alloc(377 * 4 + 4) || !dOut.alloc(256)) return ZERR(kErrMemoryAllocation);
    if (hipMemcpyAsync(dCount.p, stats.data(), 377 * 4, hipMemcpyHostToDevice, dev.s) != hipSuccess) return ZERR(kErrGeneric);
    u32* const dSize = (u32*)dCount.p + 377;
    launch_dict_entropy((const u32*)dCount.p, offcodeMax, (u8*)dOut.p, 256 - 8, dSize, dev.s);
    u32 eSize = 0;
    if (isErr(dev_read(&eSize, dSize, 4, dev.s))) return ZERR(kErrGeneric);
    if (eSize == 0) return ZERR(kErrGeneric);
    if (eSize == 0xFFFFFFFFu) return ZERR(kErrDstSizeTooSmall);
    if (hipMemcpy(header + hSize, dOut.p, eSize, hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric);
    hSize += eSize;
    if (hSize + contentSize > capacity) contentSize = capacity - hSize;
    const size_t minContentSize = 8;                                         // ZDICT_maxRep(repStartValue)
    size_t padding = 0;
    if (contentSize < minContentSize) {
        if (hSize + minContentSize > capacity) return ZERR(kErrDstSizeTooSmall);
        padding = minContentSize - contentSize;
    }
    u8* const out = (u8*)dictBuffer;
    memmove(out + hSize + padding, content, contentSize);
    memcpy(out, header, hSize);
    memset(out + hSize, 0, padding);
    return hSize + padding + contentSize;
}

// COVER_checkTotalCompressedSize (U/Cover.cs:80-137) with this library's compressor at the dictionary's level, every test sample
// compressed alone in one batch
size_t check_total(const u8* dict, size_t dictSize, const u8* samples, const size_t* sizes, const u64* offsets, unsigned first,
                   unsigned nbSamples, int level)
{
    ZSTD_CCtx* c = ZSTD_createCCtx();
    if (!c) return ZERR(kErrMemoryAllocation);
    std::vector<size_t> out(nbSamples - first);
    size_t total = dictSize, r = ZSTD_CCtx_setParameter(c, ZSTD_c_compressionLevel, level);
    if (!isErr(r)) r = ZSTD_CCtx_loadDictionary(c, dict, dictSize);
    if (!isErr(r)) r = compress_samples(c, samples, offsets + first, sizes + first, nbSamples - first, out.data(), nullptr);
    ZSTD_freeCCtx(c);
    if (isErr(r)) return r;
    for (size_t v : out) { if (isErr(v)) return v; total += v; }
    return total;
}

struct Best { size_t compressed = ZERR(kErrGeneric); std::vector<u8> dict; u32 k = 0, d = 0; };

// FASTCOVER_ctx_init + FASTCOVER_buildDictionary for every k of `ks` at one d, then COVER_selectDict + COVER_best_finish per k
// (in k order: the first of equal totals wins).  fixed = ZDICT_trainFromBuffer_fastCover (no check, the content finalized as is).
size_t train_d(Device& dev, u8* dictOut, size_t capacity, const u8* samples, const size_t* sizes, unsigned nbSamples, const u32* ks,
               u32 nK, u32 d, u32 f, u32 accel, double splitPoint, int level, unsigned dictID, bool fixed, Best* best)
{
    u64 total = 0; for (unsigned i = 0; i < nbSamples; i++) total += sizes[i];
    const unsigned nbTrain = splitPoint < 1.0 ? (unsigned)((double)nbSamples * splitPoint) : nbSamples;
    const unsigned nbTest = splitPoint < 1.0 ? nbSamples - nbTrain : nbSamples;
    u64 trainSize = 0; for (unsigned i = 0; i < nbTrain; i++) trainSize += sizes[i];
    // FASTCOVER_ctx_init's checks, in its order
    if (total < 8 || total >= 0xFFFFFFFFull) return ZERR(kErrSrcSizeWrong);
    if (nbTrain < 5) return ZERR(kErrSrcSizeWrong);
    if (nbTest < 1) return ZERR(kErrSrcSizeWrong);
    if (trainSize < 8) return ZERR(kErrSrcSizeWrong);
    if (trainSize > 0xFFFFFFFFull - 8192) return ZERR(kErrParameterUnsupported);     // positions are u32: a tile of headroom
    const u32 nbDmers = (u32)(trainSize - 8 + 1);
    std::vector<u64> offsets(nbSamples + 1, 0);
    for (unsigned i = 1; i <= nbSamples; i++) offsets[i] = offsets[i - 1] + sizes[i - 1];
    u32 wmax = 0;
    std::vector<SelCand> cands(nK);
    for (u32 i = 0; i < nK; i++) {
        cands[i].k = ks[i]; cands[i].tail = 0;
        compute_epochs((u32)capacity, nbDmers, ks[i], &cands[i].epochNum, &cands[i].epochSize);
        wmax = ks[i] - d + 1 > wmax ? ks[i] - d + 1 : wmax;
    }
    const u64 fEntries = 1ull << f;
    DBuf dSamples, dOffsets, dHashes, dPrev, dNext, dFreq, dDict, dCands;
    if (!dSamples.alloc(trainSize + 8) || !dOffsets.alloc((nbTrain + 1) * 8) || !dHashes.alloc((u64)nbDmers * 4) ||
        !dPrev.alloc((u64)nbDmers * 4) || !dNext.alloc((u64)nbDmers * 4) || !dFreq.alloc(fEntries * 4 * (nK + 1)) ||
        !dDict.alloc((u64)capacity * nK) || !dCands.alloc(sizeof(SelCand) * nK))
        return ZERR(kErrMemoryAllocation);
    hipStream_t s = dev.s;
    u32* const freq0 = (u32*)dFreq.p;
    u32* const freqCand = freq0 + fEntries;
    if (hipMemcpyAsync(dSamples.p, samples, trainSize, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(dOffsets.p, offsets.data(), (nbTrain + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(dCands.p, cands.data(), sizeof(SelCand) * nK, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(freq0, 0, fEntries * 4, s) != hipSuccess || hipMemsetAsync(dDict.p, 0, (u64)capacity * nK, s) != hipSuccess)
        return ZERR(kErrGeneric);
    const u32 g = (nbDmers + 255) / 256;
    hipLaunchKernelGGL(dt_hash_kernel, dim3(g), dim3(256), 0, s, (const u8*)dSamples.p, nbDmers, f, d, (u32*)dHashes.p);
    hipLaunchKernelGGL(dt_freq_kernel, dim3(g), dim3(256), 0, s, (const u32*)dHashes.p, (const u64*)dOffsets.p, nbTrain, nbDmers,
                       kAccelSkip[accel] + 1, freq0);
    hipLaunchKernelGGL(dt_occ_kernel, dim3((nbDmers + kOccTile - 1) / kOccTile), dim3(256), 0, s, (const u32*)dHashes.p, nbDmers, wmax,
                       (u32*)dPrev.p, (u32*)dNext.p);
    for (u32 i = 0; i < nK; i++)
        if (hipMemcpyAsync(freqCand + fEntries * i, freq0, fEntries * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
    hipLaunchKernelGGL(dt_select_kernel, dim3(nK), dim3(kSelThreads), 0, s, (const u8*)dSamples.p, (const u32*)dHashes.p,
                       (const u32*)dPrev.p, (const u32*)dNext.p, freqCand, fEntries, (u8*)dDict.p, (u32)capacity, d, (SelCand*)dCands.p);
    std::vector<u8> dicts((u64)capacity * nK);
    if (hipMemcpyAsync(cands.data(), dCands.p, sizeof(SelCand) * nK, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(dicts.data(), dDict.p, dicts.size(), hipMemcpyDeviceToHost, s) != hipSuccess)
        return ZERR(kErrGeneric);
    if (isErr(stream_wait(s))) return ZERR(kErrGeneric);
    const unsigned nbFinalize = (unsigned)((u64)nbTrain * kAccelFinalize[accel] / 100);
    for (u32 i = 0; i < nK; i++) {
        const u8* const cand = dicts.data() + (u64)capacity * i;
        const u32 tail = cands[i].tail;
        if (fixed) return finalize(dev, dictOut, capacity, cand + tail, capacity - tail, samples, sizes, nbFinalize, dictID, level);
        std::vector<u8> fin(capacity);
        const size_t dictSize = finalize(dev, fin.data(), capacity, cand + tail, capacity - tail, samples, sizes, nbFinalize, dictID, level);
        size_t compressed = dictSize;
        if (!isErr(dictSize))
            compressed = check_total(fin.data(), dictSize, samples, sizes, offsets.data(), splitPoint < 1.0 ? nbTrain : 0, nbSamples, level);
        if (compressed < best->compressed) {          // COVER_best_finish: strict <, errors are (size_t)-code and never win
            best->compressed = compressed; best->dict.assign(fin.begin(), fin.begin() + dictSize); best->k = ks[i]; best->d = d;
        }
    }
    return 0;
}

} // namespace

extern "C" {

size_t ZDICT_finalizeDictionary(void* dstDictBuffer, size_t maxDictSize, const void* dictContent, size_t dictContentSize,
                                const void* samplesBuffer, const size_t* samplesSizes, unsigned nbSamples, ZDICT_params_t parameters)
{
    try {
        if (maxDictSize < dictContentSize || maxDictSize < 256) return ZERR(kErrDstSizeTooSmall);
        Device dev;
        { const size_t e = dev.open(); if (isErr(e)) return e; }
        return finalize(dev, dstDictBuffer, maxDictSize, dictContent, dictContentSize, samplesBuffer, samplesSizes, nbSamples, parameters.dictID,
                        parameters.compressionLevel ? parameters.compressionLevel : 3);
    } catch (const std::bad_alloc&) { return ZERR(kErrMemoryAllocation); } catch (...) { return ZERR(kErrGeneric); }
}

size_t ZDICT_trainFromBuffer_fastCover(void* dictBuffer, size_t dictBufferCapacity, const void* samplesBuffer, const size_t* samplesSizes,
                                       unsigned nbSamples, ZDICT_fastCover_params_t parameters)
{
    try {
        parameters.splitPoint = 1.0;
        parameters.f = parameters.f == 0 ? 20 : parameters.f;
        parameters.accel = parameters.accel == 0 ? 1 : parameters.accel;
        if (!check_parameters(parameters.k, parameters.d, dictBufferCapacity, parameters.f, parameters.accel, parameters.splitPoint))
            return ZERR(kErrParameterOutOfBound);
        if (nbSamples == 0) return ZERR(kErrSrcSizeWrong);
        if (dictBufferCapacity < 256) return ZERR(kErrDstSizeTooSmall);
        if (parameters.f > kMaxF || parameters.shrinkDict) return ZERR(kErrParameterUnsupported);
        // FASTCOVER_ctx_init's checks come before the device is touched
        u64 total = 0; for (unsigned i = 0; i < nbSamples; i++) total += samplesSizes[i];
        if (total < 8 || total >= 0xFFFFFFFFull || nbSamples < 5) return ZERR(kErrSrcSizeWrong);
        if (dictBufferCapacity > 0xFFFFFFFFull) return ZERR(kErrParameterUnsupported);
        Device dev;
        { const size_t e = dev.open(); if (isErr(e)) return e; }
        const u32 k = parameters.k;
        return train_d(dev, (u8*)dictBuffer, dictBufferCapacity, (const u8*)samplesBuffer, samplesSizes, nbSamples, &k, 1, parameters.d,
                       parameters.f, parameters.accel, 1.0, parameters.zParams.compressionLevel ? parameters.zParams.compressionLevel : 3,
                       parameters.zParams.dictID, true, nullptr);
    } catch (const std::bad_alloc&) { return ZERR(kErrMemoryAllocation); } catch (...) { return ZERR(kErrGeneric); }
}

size_t ZDICT_optimizeTrainFromBuffer_fastCover(void* dictBuffer, size_t dictBufferCapacity, const void* samplesBuffer,
                                               const size_t* samplesSizes, unsigned nbSamples, ZDICT_fastCover_params_t* parameters)
{
    try {
        if (!parameters) return ZERR(kErrGeneric);
        const double splitPoint = parameters->splitPoint <= 0.0 ? 0.75 : parameters->splitPoint;
        const u32 kMinD = parameters->d == 0 ? 6 : parameters->d, kMaxD = parameters->d == 0 ? 8 : parameters->d;
        const u32 kMinK = parameters->k == 0 ? 50 : parameters->k, kMaxK = parameters->k == 0 ? 2000 : parameters->k;
        const u32 kSteps = parameters->steps == 0 ? 40 : parameters->steps;
        const u32 kStepSize = (kMaxK - kMinK) / kSteps > 1 ? (kMaxK - kMinK) / kSteps : 1;
        const u32 f = parameters->f == 0 ? 20 : parameters->f, accel = parameters->accel == 0 ? 1 : parameters->accel;
        // ZDICT_optimizeTrainFromBuffer_fastCover's checks, in its order
        if (splitPoint <= 0 || splitPoint > 1) return ZERR(kErrParameterOutOfBound);
        if (accel == 0 || accel > 10) return ZERR(kErrParameterOutOfBound);
        if (kMinK < kMaxD || kMaxK < kMinK) return ZERR(kErrParameterOutOfBound);
        if (nbSamples == 0) return ZERR(kErrSrcSizeWrong);
        if (dictBufferCapacity < 256) return ZERR(kErrDstSizeTooSmall);
        if (f > kMaxF || parameters->shrinkDict) return ZERR(kErrParameterUnsupported);    // (nbThreads is accepted and ignored)
        // FASTCOVER_ctx_init's checks come before the device is touched
        {
            u64 total = 0; for (unsigned i = 0; i < nbSamples; i++) total += samplesSizes[i];
            const unsigned nbTrain = splitPoint < 1.0 ? (unsigned)((double)nbSamples * splitPoint) : nbSamples;
            const unsigned nbTest = splitPoint < 1.0 ? nbSamples - nbTrain : nbSamples;
            if (total < 8 || total >= 0xFFFFFFFFull || nbTrain < 5 || nbTest < 1) return ZERR(kErrSrcSizeWrong);
        }
        if (dictBufferCapacity > 0xFFFFFFFFull) return ZERR(kErrParameterUnsupported);
        Device dev;
        { const size_t e = dev.open(); if (isErr(e)) return e; }
        const int level = parameters->zParams.compressionLevel ? (int)parameters->zParams.compressionLevel : 3;
        Best best;
        for (u32 d = kMinD; d <= kMaxD; d += 2) {
            std::vector<u32> ks;
            for (u32 k = kMinK; k <= kMaxK; k += kStepSize)
                if (check_parameters(k, d, dictBufferCapacity, f, accel, splitPoint)) ks.push_back(k);
            for (size_t i = 0; i < ks.size(); i += kMaxCandidates) {
                const u32 n = (u32)(ks.size() - i < kMaxCandidates ? ks.size() - i : kMaxCandidates);
                const size_t e = train_d(dev, (u8*)dictBuffer, dictBufferCapacity, (const u8*)samplesBuffer, samplesSizes, nbSamples,
                                         ks.data() + i, n, d, f, accel, splitPoint, level, parameters->zParams.dictID, false, &best);
                if (isErr(e)) return e;
            }
        }
        if (isErr(best.compressed)) return best.compressed;
        parameters->k = best.k; parameters->d = best.d; parameters->steps = kSteps; parameters->splitPoint = splitPoint;
        parameters->f = f; parameters->accel = accel; parameters->shrinkDict = 0;
        memcpy(dictBuffer, best.dict.data(), best.dict.size());
        return best.dict.size();
    } catch (const std::bad_alloc&) { return ZERR(kErrMemoryAllocation); } catch (...) { return ZERR(kErrGeneric); }
}

size_t ZDICT_trainFromBuffer(void* dictBuffer, size_t dictBufferCapacity, const void* samplesBuffer, const size_t* samplesSizes,
                             unsigned nbSamples)
{
    ZDICT_fastCover_params_t params;
    memset(&params, 0, sizeof params);
    params.d = 8; params.steps = 4; params.zParams.compressionLevel = 3;
    return ZDICT_optimizeTrainFromBuffer_fastCover(dictBuffer, dictBufferCapacity, samplesBuffer, samplesSizes, nbSamples, &params);
}

} // extern "C"
