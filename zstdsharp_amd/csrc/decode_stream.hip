// decode_stream.hip — what a segment of a segmented stream leaves for the next one (ZSTDMI_DCtx_setStreamSegment).
// The stream adapter (zstd_mi355x_dec.hip) decodes a long frame as a run of fragments through the ordinary pipeline; between two
// fragments it carries the last window of output (device copies), the blocks that define the live tables (host bytes), and:
//   stream_carry   : the three repcodes behind the fragment's last block, into the triple block_offsets starts the next fragment from;
//   stream_xxh     : XXH64 of the frame's content with carried state — the arithmetic at the end of exec_matches (decode_seq.hip),
//                    which checks a frame it sees whole; here the four accumulators, the length and up to 31 bytes that have not
//                    filled a stripe yet live in a small device struct from one fragment's output to the next.
#include "zmi_decode.h"
#include "zmi_host.h"

namespace zmi {

// the repcodes behind the last block: its starting repcodes (block_offsets) through its own transfer function (seq_decode)
__global__ __launch_bounds__(64) void stream_carry_kernel(const BlockDesc* __restrict__ blocks, u32 nBlocks, DictInfo* __restrict__ reps)
{
    if (threadIdx.x != 0 || blockIdx.x != 0 || nBlocks == 0) return;
    const BlockDesc& B = blocks[nBlocks - 1];
    u32 r[3] = { B.repIn[0], B.repIn[1], B.repIn[2] };
    if (B.type == 2 && B.nbSeq != 0 && !B.err) {
        u32 n[3];
        for (u32 i = 0; i < 3; ++i) {
            const u32 kind = B.repKind[i], val = B.repVal[i];
            if (kind == 0) n[i] = val;
            else { const u32 in = kind == 1 ? r[0] : kind == 2 ? r[1] : r[2]; n[i] = in > val ? in - val : 1u; }
        }
        r[0] = n[0]; r[1] = n[1]; r[2] = n[2];
    }
    reps->rep[0] = r[0]; reps->rep[1] = r[1]; reps->rep[2] = r[2];
}

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

void launch_stream_carry(const BlockDesc* blocks, u32 nBlocks, DictInfo* reps, hipStream_t stream)
{
    hipLaunchKernelGGL(stream_carry_kernel, dim3(1), dim3(64), 0, stream, blocks, nBlocks, reps);
}
void launch_stream_xxh(XxhCarry* st, const u8* data, u64 n, u32 final, hipStream_t stream)
{
    hipLaunchKernelGGL(stream_xxh_kernel, dim3(1), dim3(64), 0, stream, st, data, n, final);
}

} // namespace zmi
