// zmi_dictid.h — plain host code of ZSTD_getDictID_fromDict and ZSTD_getDictID_fromFrame (U/ZstdDecompress.cs:2014-2060): the dictID
// a formatted dictionary states, and the one a frame's header names.  No device code and no HIP header, so that
// tests/host/dictid_harness.cpp can build it for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zmi {

inline uint32_t dictid_le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// the dictID of a formatted dictionary (magic 0xEC30A437, then the ID); 0 for raw content, NULL and fewer than 8 bytes
inline uint32_t dictid_from_dict(const uint8_t* dict, size_t dictSize)
{
    if (!dict || dictSize < 8) return 0;
    if (dictid_le32(dict) != 0xEC30A437u) return 0;
    return dictid_le32(dict + 4);
}

// the dictID a zstd frame's header names (ZSTD_getFrameHeader's Dictionary_ID field); 0 for a frame without one, a skippable frame,
// another magic, a reserved descriptor bit and a header of which not every byte is there.  Reads src[0 .. srcSize) only.
inline uint32_t dictid_from_frame(const uint8_t* src, size_t srcSize)
{
    if (!src || srcSize < 5) return 0;
    if (dictid_le32(src) != 0xFD2FB528u) return 0;              // (skippable frames, 0x184D2A5?, carry none)
    const uint8_t fhd = src[4];
    if (fhd & 0x08) return 0;                                   // reserved bit: ZSTD_getFrameHeader refuses the header
    const bool single = (fhd >> 5) & 1;
    const uint32_t fcsId = fhd >> 6;
    static const uint8_t didBytes[4] = { 0, 1, 2, 4 }, fcsBytes[4] = { 0, 2, 4, 8 };
    const size_t did = didBytes[fhd & 3];
    const size_t headerSize = 5 + (single ? 0 : 1) + did + fcsBytes[fcsId] + ((single && !fcsId) ? 1 : 0);
    if (srcSize < headerSize) return 0;                         // (the reference answers a header it cannot read whole with 0)
    const uint8_t* const p = src + 5 + (single ? 0 : 1);
    switch (did) {
    case 1: return p[0];
    case 2: return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    case 4: return dictid_le32(p);
    default: return 0;
    }
}

} // namespace zmi
