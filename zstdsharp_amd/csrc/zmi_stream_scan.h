// zmi_stream_scan.h — the host scan of the segmented stream decoder (ZSTDMI_DCtx_setStreamSegment, zstd_mi355x_dec.hip).
// Plain C++ over byte buffers, no device and no allocation: which entropy tables a block DEFINES, so that the stream adapter knows
// which earlier blocks a later segment still needs in front of it.  A treeless literals section uses the Huffman table of the last
// block with a literals section of type 2 (U/ZstdDecompressBlock.cs:197-207); a sequences table in repeat mode uses the one of the
// last block with sequences whose mode for that table is not 3 (:1780-1786).  The scan reads a block's header, its literals-section
// header, the sequence count and the modes byte — the same fields as block_parse_kernel (decode_walk.hip), without the NCount
// descriptions.  A block it cannot parse defines nothing: the device finds that block's real error when it decodes it.
// tests/host/stream_scan_harness.cpp runs it under AddressSanitizer against a second implementation.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace zmi {

enum : uint32_t { kDefHuf = 1, kDefLL = 2, kDefOF = 4, kDefML = 8 };

struct ScanBlock {
    uint32_t type;      // 0 raw, 1 RLE, 2 compressed, 3 reserved
    uint32_t last;      // the last-block bit
    uint32_t body;      // bytes behind the 3-byte header (an RLE block: 1)
    uint32_t defines;   // kDef* bits
};

// which tables the body [b, b + bsz) of a compressed block defines (0 = none, or not parsable)
inline uint32_t scan_block_defines(const uint8_t* b, size_t bsz)
{
    if (bsz < 3 || bsz >= (1u << 17)) return 0;
    const uint32_t litType = b[0] & 3, lhl = (b[0] >> 2) & 3;
    size_t lhSize, litSize, litCSize = 0;
    if (litType >= 2) {
        if (bsz < 5) return 0;
        const uint32_t lhc = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        if (lhl <= 1)      { lhSize = 3; litSize = (lhc >> 4) & 0x3FF;   litCSize = (lhc >> 14) & 0x3FF; }
        else if (lhl == 2) { lhSize = 4; litSize = (lhc >> 4) & 0x3FFF;  litCSize = lhc >> 18; }
        else               { lhSize = 5; litSize = (lhc >> 4) & 0x3FFFF; litCSize = (lhc >> 22) + ((size_t)b[4] << 10); }
        if (litSize > (1u << 17) || lhSize + litCSize > bsz) return 0;
    } else {
        if (lhl == 0 || lhl == 2) { lhSize = 1; litSize = b[0] >> 3; }
        else if (lhl == 1)        { lhSize = 2; litSize = ((uint32_t)b[0] | ((uint32_t)b[1] << 8)) >> 4; }
        else                      { lhSize = 3; litSize = ((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16)) >> 4; }
        if (litSize > (1u << 17)) return 0;
        if (litType == 0 ? lhSize + litSize > bsz : lhSize + 1 > bsz) return 0;
    }
    size_t bp = litType >= 2 ? lhSize + litCSize : litType == 0 ? lhSize + litSize : lhSize + 1;
    if (bp >= bsz) return 0;
    const uint32_t huf = litType == 2 ? (uint32_t)kDefHuf : 0u;
    uint32_t nbSeq = b[bp++];
    if (!nbSeq) return bp == bsz ? huf : 0u;
    if (nbSeq > 0x7F) {
        if (nbSeq == 0xFF) { if (bp + 2 > bsz) return 0; bp += 2; }
        else { if (bp >= bsz) return 0; bp += 1; }
    }
    if (bp + 1 > bsz) return 0;
    const uint32_t modes = b[bp];
    uint32_t d = huf;
    if (((modes >> 6) & 3) != 3) d |= kDefLL;
    if (((modes >> 4) & 3) != 3) d |= kDefOF;
    if (((modes >> 2) & 3) != 3) d |= kDefML;
    return d;
}

// the block whose 3-byte header starts at p, of which `avail` bytes are there -> its size with the header (out filled), or 0: not all
// of it is there yet.  A block of the reserved type 3 is reported whole with 3 bytes and body 0 (the caller refuses the frame).
inline size_t scan_block(const uint8_t* p, size_t avail, ScanBlock* out)
{
    if (avail < 3) return 0;
    const uint32_t bh = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    out->last = bh & 1; out->type = (bh >> 1) & 3; out->defines = 0;
    out->body = out->type == 3 ? 0u : out->type == 1 ? 1u : bh >> 3;
    if (3 + (size_t)out->body > avail) return 0;
    if (out->type == 2) out->defines = scan_block_defines(p + 3, out->body);
    return 3 + (size_t)out->body;
}

} // namespace zmi
