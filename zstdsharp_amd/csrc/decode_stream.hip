// decode_stream.hip — what a segment of a segmented stream leaves for the next one (ZSTDMI_DCtx_setStreamSegment).
// The stream adapter (zstd_mi355x_dec.hip) decodes a long frame as a run of fragments through the ordinary pipeline; between two
// fragments it carries the last window of output (device copies), the blocks that define the live tables (host bytes), and:
//   stream_carry   : the three repcodes behind the fragment's last block, into the triple block_offsets starts the next fragment from;
//   stream_xxh     : XXH64 of the frame's content with carried state (frame.hip, shared with the compressor's single-frame output) —
//                    the arithmetic at the end of exec_matches (decode_seq.hip), which checks a frame it sees whole; here the four
//                    accumulators, the length and up to 31 bytes that have not filled a stripe yet live in a small device struct
//                    from one fragment's output to the next.
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

void launch_stream_carry(const BlockDesc* blocks, u32 nBlocks, DictInfo* reps, hipStream_t stream)
{
    hipLaunchKernelGGL(stream_carry_kernel, dim3(1), dim3(64), 0, stream, blocks, nBlocks, reps);
}

} // namespace zmi
