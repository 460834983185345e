// Stand-alone CPU harness of the dictID parsers (zstdsharp_amd/csrc/zmi_dictid.h) behind ZSTD_getDictID_fromDict and
// ZSTD_getDictID_fromFrame.  tests/test_cdict_abi.py builds it with -fsanitize=address,undefined.  Every input is a heap block of exactly
// the size stated, so a byte read beyond it stops the program: each header is parsed whole and at every truncation.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zmi_dictid.h"

static uint32_t on_heap_frame(const std::vector<uint8_t>& v, size_t n)
{
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(p, v.data(), n);
    const uint32_t id = zmi::dictid_from_frame(n ? p : nullptr, n);
    free(p);
    return id;
}
static uint32_t on_heap_dict(const std::vector<uint8_t>& v, size_t n)
{
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(p, v.data(), n);
    const uint32_t id = zmi::dictid_from_dict(n ? p : nullptr, n);
    free(p);
    return id;
}

int main()
{
    int bad = 0;
    {   // every frame header descriptor without the reserved bit: dictID field of 0, 1, 2, 4 bytes; single segment or window; every FCS size
        int headers = 0;
        for (uint32_t fhd = 0; fhd < 256; ++fhd) {
            if (fhd & 0x08) continue;
            const bool single = (fhd >> 5) & 1;
            const uint32_t didId = fhd & 3, fcsId = fhd >> 6;
            const size_t did = didId == 3 ? 4 : didId, fcs = fcsId == 0 ? (single ? 1 : 0) : (size_t)1 << fcsId;
            const uint32_t want = did == 0 ? 0u : did == 1 ? 0xA7u : did == 2 ? 0xB6A7u : 0xD4C5B6A7u;
            std::vector<uint8_t> h = { 0x28, 0xB5, 0x2F, 0xFD, (uint8_t)fhd };
            if (!single) h.push_back(0x58);
            for (size_t i = 0; i < did; ++i) h.push_back((uint8_t)(0xA7 + 0x0F * i));
            for (size_t i = 0; i < fcs; ++i) h.push_back(0xEE);
            const size_t full = h.size();
            h.push_back(0x01); h.push_back(0x00); h.push_back(0x00);       // (an empty last block behind it)
            bool ok = on_heap_frame(h, h.size()) == want && on_heap_frame(h, full) == want;
            for (size_t n = 0; n < full; ++n) ok = ok && on_heap_frame(h, n) == 0;         // a header that is not all there names none
            bad += !ok; ++headers;
        }
        printf("frame headers: %d descriptors bad=%d\n", headers, bad);
    }
    {   // the reserved bit, a skippable frame, a wrong magic
        const std::vector<uint8_t> reserved = { 0x28, 0xB5, 0x2F, 0xFD, 0x2B, 1, 2, 3, 4, 5, 6, 7, 8 };
        const std::vector<uint8_t> skippable = { 0x53, 0x2A, 0x4D, 0x18, 4, 0, 0, 0, 9, 9, 9, 9 };
        const std::vector<uint8_t> wrong = { 0x29, 0xB5, 0x2F, 0xFD, 0x23, 1, 2, 3, 4, 5 };
        const bool ok = on_heap_frame(reserved, reserved.size()) == 0 && on_heap_frame(skippable, skippable.size()) == 0 && on_heap_frame(wrong, wrong.size()) == 0;
        printf("refused: reserved bit, skippable, wrong magic %s\n", ok ? "ok" : "WRONG");
        bad += !ok;
    }
    {   // dictionaries: the ID behind the magic; raw content; every size below 8
        const std::vector<uint8_t> fmt = { 0x37, 0xA4, 0x30, 0xEC, 0x78, 0x56, 0x34, 0x12, 0, 0 };
        const std::vector<uint8_t> raw = { 'r', 'a', 'w', ' ', 'b', 'y', 't', 'e', 's', '!' };
        bool ok = on_heap_dict(fmt, fmt.size()) == 0x12345678u && on_heap_dict(fmt, 8) == 0x12345678u && on_heap_dict(raw, raw.size()) == 0;
        for (size_t n = 0; n < 8; ++n) ok = ok && on_heap_dict(fmt, n) == 0;
        printf("dictionaries: formatted, raw, short %s\n", ok ? "ok" : "WRONG");
        bad += !ok;
    }
    printf("done bad=%d\n", bad);
    return bad ? 1 : 0;
}
