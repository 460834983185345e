// zmi_frame.h — the two facts about framing that the encode kernels and the host share, each stated once: what a frame header looks
// like (its size for a frame length, and its bytes) and where a chunk lies in its frame.  Plain integer code without a HIP header:
// the kernels and the host of libzstd_mi355x.so include it under hipcc, tests/host/frame_layout_harness.cpp builds it for the CPU.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define ZMI_HD __host__ __device__ __forceinline__
#else
#define ZMI_HD inline
#endif

namespace zmi {

// ---- the frame header (ZSTD_writeFrameHeader, U/ZstdCompress.cs:4817-4929) ----
// A single segment with the content size; or, with noContentSize, a window descriptor alone: the smallest power of two that holds the
// frame (>= 1 KiB), so that no offset and no block exceeds the declared window; or, with an explicit windowLog (frames of independent
// blocks, each a window long; one frame across passes), a descriptor for exactly that window beside the content size (unless
// noContentSize).  dictIdBytes: the dictID field of 0, 1, 2 or 4 bytes (a formatted dictionary, ZSTD_c_dictIDFlag).
struct FrameHeaderSpec { uint32_t dictID; uint8_t dictIdBytes, checksum, noContentSize, windowLog; };

ZMI_HD uint32_t dict_id_bytes(uint32_t dictID) { return !dictID ? 0u : dictID < 256 ? 1u : dictID < 65536 ? 2u : 4u; }
// Frame_Content_Size code 0 .. 3: a field of 1 (single segment) or 0, 2, 4, 8 bytes
ZMI_HD uint32_t frame_fcs_code(uint64_t len) { return (uint32_t)(len >= 256) + (uint32_t)(len >= 65536 + 256) + (uint32_t)(len > 0xFFFFFFFFull); }
ZMI_HD bool frame_single_segment(const FrameHeaderSpec& h) { return !h.noContentSize && !h.windowLog; }
// -> bytes of the header of a frame of frameLen bytes
ZMI_HD uint32_t frame_header_bytes(const FrameHeaderSpec& h, uint64_t frameLen)
{
    const uint32_t code = frame_fcs_code(frameLen);
    if (frame_single_segment(h)) return 4 + 1 + h.dictIdBytes + (1u << code);
    return 4 + 1 + 1 + h.dictIdBytes + (h.noContentSize || !code ? 0u : 1u << code);
}
ZMI_HD void frame_put_le(uint8_t* p, uint64_t v, uint32_t bytes) { for (uint32_t i = 0; i < bytes; ++i) p[i] = (uint8_t)(v >> (8 * i)); }

// writes the header to dst -> bytes written (= frame_header_bytes)
ZMI_HD uint32_t frame_header_write(const FrameHeaderSpec& h, uint64_t frameLen, uint8_t* dst)
{
    const bool single = frame_single_segment(h);
    const uint32_t code = h.noContentSize ? 0u : frame_fcs_code(frameLen);
    const uint32_t didCode = h.dictIdBytes == 4 ? 3u : h.dictIdBytes;
    frame_put_le(dst, 0xFD2FB528u, 4);
    dst[4] = (uint8_t)(didCode + (h.checksum ? 4u : 0u) + (single ? 32u : 0u) + (code << 6));
    uint32_t n = 5;
    if (!single) {
        uint32_t wl = h.windowLog;
        if (!wl) { wl = 10; while (((uint64_t)1 << wl) < frameLen) ++wl; }
        dst[n++] = (uint8_t)((wl - 10) << 3);
    }
    frame_put_le(dst + n, h.dictID, h.dictIdBytes); n += h.dictIdBytes;
    // (code 1 stores the size minus 256; code 0 is one byte in a single segment and no field behind a window descriptor; constant
    //  widths, so that each store sequence is unrolled: this runs on one lane at the end of every frame's first block)
    if (h.noContentSize || (!single && !code)) return n;
    if (code == 0) frame_put_le(dst + n, frameLen, 1);
    else if (code == 1) frame_put_le(dst + n, frameLen - 256, 2);
    else if (code == 2) frame_put_le(dst + n, frameLen, 4);
    else frame_put_le(dst + n, frameLen, 8);
    return n + (1u << code);
}

// ---- a block's place in its frame ----
// block: its index inside the frame (kSingle: only whether it is the first, 0 or 1); frameLen: the frame's content size (kSingle: ~0
// while the frame goes on behind this pass); last: the frame's last block; front: bytes of the frame in front of the block.
struct BlockPlace { uint32_t block; uint64_t frameLen; bool last; uint64_t front; };
// How the chunks of a pass map to frames, in one of three forms.  `form` says which one holds (the host selects a kernel's instance
// by it, a kernel that serves two forms branches on it, block_place takes it at compile time: a kernel template's TAB parameter):
// kArith: every `frameBlocks` consecutive chunks of chunkBytes are one frame of the srcSize input bytes.
// kTable: a batch's entries differ in length, so a chunk's place comes from table[c] = chunk_frame_word(block index, frame length).
// kSingle: the input is ONE frame that passes and stream batches cut anywhere: `at` bytes of it lie in front of chunk 0 (readable
//          there, as far as the finders reach back), `total` is its content size.
enum FrameForm : int { kArith = 0, kTable = 1, kSingle = 2 };
struct FrameLayout {
    int form;                             // FrameForm
    uint32_t chunkBytes, frameBlocks;     // frameBlocks 0: every chunk a frame of its own (no place to compute: block_alone)
    uint64_t srcSize;                     // kArith
    const uint32_t* table;                // kTable
    uint64_t at, total;                   // kSingle
};
ZMI_HD FrameLayout layout_arith(uint32_t chunkBytes, uint32_t frameBlocks, uint64_t srcSize) { return FrameLayout{ kArith, chunkBytes, frameBlocks, srcSize, nullptr, 0, 0 }; }
ZMI_HD FrameLayout layout_table(uint32_t chunkBytes, uint32_t frameBlocks, const uint32_t* table) { return FrameLayout{ kTable, chunkBytes, frameBlocks, 0, table, 0, 0 }; }
ZMI_HD FrameLayout layout_single(uint32_t chunkBytes, uint32_t frameBlocks, uint64_t at, uint64_t total) { return FrameLayout{ kSingle, chunkBytes, frameBlocks, 0, nullptr, at, total }; }

// the table form's word: bits 24-31 the block index inside its frame, bits 0-23 the frame's content size
constexpr uint32_t kFrameWordBlocks = 256, kFrameWordLen = 1u << 24;
ZMI_HD uint32_t chunk_frame_word(uint32_t blockInFrame, uint32_t frameLen) { return (blockInFrame << 24) | frameLen; }
ZMI_HD uint32_t frame_word_block(uint32_t w) { return w >> 24; }
ZMI_HD uint32_t frame_word_len(uint32_t w) { return w & 0xFFFFFFu; }
// of `chunks` chunks, those that are whole frames (a pass never ends inside a frame of the arithmetic form)
ZMI_HD uint32_t whole_frame_chunks(uint32_t chunks, uint32_t frameBlocks) { return chunks - chunks % frameBlocks; }
// the arithmetic form's block index of chunk c
ZMI_HD uint32_t block_index(uint32_t c, uint32_t frameBlocks) { return c % frameBlocks; }
// a chunk that is a frame of its own, n bytes long
ZMI_HD BlockPlace block_alone(uint64_t n) { return BlockPlace{ 0u, n, true, 0u }; }
// the place of chunk c (g.frameBlocks != 0).  Callers read the fields they need; the rest folds away.
template <int FORM>
ZMI_HD BlockPlace block_place(const FrameLayout& g, uint32_t c)
{
    BlockPlace p;
    if (FORM == kSingle) {
        p.front = g.at + (uint64_t)c * g.chunkBytes; p.block = p.front != 0 ? 1u : 0u; p.frameLen = g.total;
        p.last = p.front + g.chunkBytes >= g.total;
        return p;
    }
    if (FORM == kTable) { p.block = frame_word_block(g.table[c]); p.frameLen = frame_word_len(g.table[c]); }
    else {
        p.block = block_index(c, g.frameBlocks);
        const uint64_t start = (uint64_t)(c - p.block) * g.chunkBytes, most = (uint64_t)g.frameBlocks * g.chunkBytes;
        p.frameLen = g.srcSize - start < most ? g.srcSize - start : most;
    }
    p.front = (uint64_t)p.block * g.chunkBytes;
    p.last = p.front + g.chunkBytes >= p.frameLen;
    return p;
}

// ---- the finder's frameBlocks argument: bit 31 says the frame's blocks are independent of each other (windows below 64 KiB, where a
// block IS the window: no history between them) ----
struct FrameBlocksArg { uint32_t frameBlocks; bool independent; };
ZMI_HD uint32_t frame_blocks_encode(uint32_t frameBlocks, bool independent) { return frameBlocks | (independent ? 0x80000000u : 0u); }
ZMI_HD FrameBlocksArg frame_blocks_decode(uint32_t arg) { return FrameBlocksArg{ arg & 0x7FFFFFFFu, (arg >> 31) != 0 }; }

} // namespace zmi
