// digest.hip — digests of many pieces of one device buffer (ZSTDMI_digestPieces, ZSTDMI_contentCutsDigests; the functions: zmi_digest.h;
// DESIGN.md 5t).  Both functions are serial inside a piece; the parallelism is the number of pieces.
//   digest_xxh64    four lanes per piece, accumulator j on lane j (sixteen pieces per wave).  Lane j reads word j of every stripe; the
//                   next eight stripes' words are loaded into registers before the rounds over the current eight begin, so the chain
//                   never waits for a load it has just issued.  Lane 0 of the group merges, eats the 0 .. 31 bytes behind the whole
//                   stripes and writes the value.
//   digest_sha256   one lane per piece.  The state and the sixteen-word window are registers (every index of sha256_block is a constant
//                   once unrolled); the next block's sixteen words are loaded, as four 16-byte loads, before the 64 rounds of the
//                   current one.  The padding block or blocks are built from the piece's last bytes by sha256_pad_word.
// Pieces begin at any byte: every load here is an unaligned global load of bytes that lie inside the piece (whole stripes, whole blocks,
// or single bytes of the tail), never beyond it.
// Where the pieces are: `offs` (the general call: n + 1 u64 offsets from src, made and checked by the host) or `ends` (the fused call:
// cut_select's output, count then ends, which never left the device; the grid covers the most pieces the rule allows and the lanes
// behind the count leave).  A wave lasts as long as its longest piece: pieces are not sorted and not claimed (DESIGN.md 5t prices it).
#include <hip/hip_runtime.h>
#include "zmi_common.h"
#include "zmi_device.h"
#include "zmi_host.h"
#include "zmi_digest.h"

namespace zmi {

struct DeviceBytes {
    __device__ static u32 le32(const u8* p) { return readLE32(p); }
    __device__ static u64 le64(const u8* p) { return readLE64(p); }
};
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(1))) u32x4u;

// piece i of the table -> false: there is none.  The fused form trusts nothing it reads: an end outside [start, srcSize] is an empty
// piece (the host refuses such a list behind the read-back; here it only must not become an address).
template <bool CUT>
__device__ __forceinline__ bool piece_span(const DigestPieces& tab, u64 i, u64& start, u64& len)
{
    if (i >= tab.n) return false;
    if (CUT) {
        const u32 np = tab.ends[0];
        if (i >= np) return false;
        const u32 s = i ? tab.ends[i] : 0u, e = tab.ends[i + 1];
        start = s; len = (e >= s && (u64)e <= tab.srcSize) ? (u64)(e - s) : 0ull;
    } else {
        start = tab.offs[i]; len = tab.offs[i + 1] - start;
    }
    return true;
}

constexpr u32 kXxhAhead = 8;        // stripes whose words are in registers ahead of the chain

template <bool CUT>
__global__ __launch_bounds__(64) void digest_xxh64_kernel(const u8* __restrict__ src, const DigestPieces tab, u8* __restrict__ out)
{
    const u64 t = (u64)blockIdx.x * 64 + threadIdx.x;
    const u64 i = t >> 2; const u32 j = (u32)t & 3u;
    u64 start, len;
    if (!piece_span<CUT>(tab, i, start, len)) return;       // (the four lanes of a group leave together)
    const u8* const p = src + start;
    const u64 stripes = len >> 5;
    const u8* const q = p + 8 * j;
    u64 v = xxh64_start(j);
    u64 s = 0;
    if (stripes >= kXxhAhead) {
        u64 a[kXxhAhead], b[kXxhAhead];
#pragma unroll
        for (u32 k = 0; k < kXxhAhead; ++k) a[k] = readLE64(q + 32 * k);
        for (; s + kXxhAhead <= stripes; s += kXxhAhead) {
            const bool more = s + 2 * kXxhAhead <= stripes;
            if (more) {
#pragma unroll
                for (u32 k = 0; k < kXxhAhead; ++k) b[k] = readLE64(q + 32 * (s + kXxhAhead + k));
            }
#pragma unroll
            for (u32 k = 0; k < kXxhAhead; ++k) v = xxh64_round(v, a[k]);
            if (more) {
#pragma unroll
                for (u32 k = 0; k < kXxhAhead; ++k) a[k] = b[k];
            }
        }
    }
    for (; s < stripes; ++s) v = xxh64_round(v, readLE64(q + 32 * s));
    const u32 l0 = threadIdx.x & 60u;                       // the group's first lane
    const u64 v1 = __shfl(v, l0), v2 = __shfl(v, l0 + 1), v3 = __shfl(v, l0 + 2), v4 = __shfl(v, l0 + 3);
    if (j) return;
    const u64 h = xxh64_finish<DeviceBytes>(v1, v2, v3, v4, len, p + (stripes << 5));
    *(u64*)(out + 8 * i) = h;                               // (little-endian; out is an allocation's start)
}

__device__ __forceinline__ void sha_load_block(const u8* p, u32 w[16])
{
    const u32x4 x0 = *(const u32x4u*)p, x1 = *(const u32x4u*)(p + 16), x2 = *(const u32x4u*)(p + 32), x3 = *(const u32x4u*)(p + 48);
    w[0] = x0.x; w[1] = x0.y; w[2] = x0.z; w[3] = x0.w; w[4] = x1.x; w[5] = x1.y; w[6] = x1.z; w[7] = x1.w;
    w[8] = x2.x; w[9] = x2.y; w[10] = x2.z; w[11] = x2.w; w[12] = x3.x; w[13] = x3.y; w[14] = x3.z; w[15] = x3.w;
}

template <bool CUT>
__global__ __launch_bounds__(64) void digest_sha256_kernel(const u8* __restrict__ src, const DigestPieces tab, u8* __restrict__ out)
{
    const u64 i = (u64)blockIdx.x * 64 + threadIdx.x;
    u64 start, len;
    if (!piece_span<CUT>(tab, i, start, len)) return;
    const u8* const p = src + start;
    const u64 blocks = len >> 6;
    u32 h[8], w[16], nx[16];
    sha256_init(h);
    if (blocks) sha_load_block(p, w);
    for (u64 b = 0; b < blocks; ++b) {
        const bool more = b + 1 < blocks;
        if (more) sha_load_block(p + 64 * (b + 1), nx);
#pragma unroll
        for (u32 k = 0; k < 16; ++k) w[k] = __builtin_bswap32(w[k]);
        sha256_block(h, w);
        if (more) {
#pragma unroll
            for (u32 k = 0; k < 16; ++k) w[k] = nx[k];
        }
    }
    const u8* const tail = p + (blocks << 6);
    const u32 pads = sha256_pad_blocks(len);
    for (u32 k = 0; k < pads; ++k) {
#pragma unroll
        for (u32 x = 0; x < 16; ++x) w[x] = sha256_pad_word(tail, len, k, x);
        sha256_block(h, w);
    }
    u32x4 lo, hi;
    lo.x = __builtin_bswap32(h[0]); lo.y = __builtin_bswap32(h[1]); lo.z = __builtin_bswap32(h[2]); lo.w = __builtin_bswap32(h[3]);
    hi.x = __builtin_bswap32(h[4]); hi.y = __builtin_bswap32(h[5]); hi.z = __builtin_bswap32(h[6]); hi.w = __builtin_bswap32(h[7]);
    u32x4* const o = (u32x4*)(out + 32 * i);                // (out is an allocation's start)
    o[0] = lo; o[1] = hi;
}

// ---- host side ----
// out: tab.n * digest_size(kind) bytes; kind is 1 or 2 (the caller's check)
void launch_digest(unsigned kind, const u8* src, const DigestPieces& tab, u8* out, hipStream_t stream)
{
    if (!tab.n) return;
    const bool cut = tab.ends != nullptr;
    if (kind == kDigestXxh64) {
        const u32 grid = (u32)((tab.n * 4 + 63) / 64);
        if (cut) hipLaunchKernelGGL(digest_xxh64_kernel<true>, dim3(grid), dim3(64), 0, stream, src, tab, out);
        else     hipLaunchKernelGGL(digest_xxh64_kernel<false>, dim3(grid), dim3(64), 0, stream, src, tab, out);
    } else {
        const u32 grid = (u32)((tab.n + 63) / 64);
        if (cut) hipLaunchKernelGGL(digest_sha256_kernel<true>, dim3(grid), dim3(64), 0, stream, src, tab, out);
        else     hipLaunchKernelGGL(digest_sha256_kernel<false>, dim3(grid), dim3(64), 0, stream, src, tab, out);
    }
}

} // namespace zmi
