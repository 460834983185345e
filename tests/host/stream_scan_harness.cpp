// Stand-alone CPU harness of the segmented stream decoder's host scan (zstdsharp_amd/csrc/zmi_stream_scan.h): which blocks of a frame
// define its Huffman and FSE tables.  tests/test_stream_segment_abi.py builds it with -fsanitize=address,undefined and runs it over
// the .zst files it names: every file whole, and the files behind "--cut" at every truncation as well.  Each input is copied into a
// heap block of exactly its size, so a read beyond what has arrived stops the program.  The scan's answer — per block its size, type,
// last bit and the tables it defines, and per frame the block that owns each table after every block — is compared with a second
// implementation below that goes through bounds-checked accessors only and knows nothing of the first.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdexcept>
#include <string>
#include <vector>
#include "zmi_stream_scan.h"

// ---- the second implementation: a view that throws on any index outside it ----
struct View {
    const uint8_t* p; size_t n;
    uint8_t at(size_t i) const { if (i >= n) throw std::out_of_range("view"); return p[i]; }
    uint64_t le(size_t i, unsigned bytes) const { uint64_t v = 0; for (unsigned k = 0; k < bytes; ++k) v |= (uint64_t)at(i + k) << (8 * k); return v; }
    View sub(size_t i, size_t len) const { if (i > n || len > n - i) throw std::out_of_range("sub"); return View{ p + i, len }; }
};

// tables a compressed block's body defines: bit 0 Huffman, bits 1..3 LL, OF, ML (RFC 8878 3.1.1.3); anything malformed -> none
static unsigned ref_defines(View body)
{
    try {
        if (body.n < 3 || body.n >= 131072) return 0;
        const unsigned first = body.at(0), litType = first & 3, sizeFormat = (first >> 2) & 3;
        size_t headerBytes, regenerated, compressed = 0;
        if (litType == 2 || litType == 3) {
            if (body.n < 5) return 0;               // (the decoder reads four bytes of header at once, five for the long format)
            if (sizeFormat == 0 || sizeFormat == 1) { headerBytes = 3; const uint64_t v = body.le(0, 3); regenerated = (v >> 4) & 1023; compressed = (v >> 14) & 1023; }
            else if (sizeFormat == 2) { headerBytes = 4; const uint64_t v = body.le(0, 4); regenerated = (v >> 4) & 16383; compressed = (v >> 18) & 16383; }
            else { headerBytes = 5; const uint64_t v = body.le(0, 5); regenerated = (v >> 4) & 262143; compressed = (v >> 22) & 262143; }
            if (regenerated > 131072) return 0;
            (void)body.sub(0, headerBytes + compressed);
        } else {
            if (sizeFormat == 0 || sizeFormat == 2) { headerBytes = 1; regenerated = first >> 3; }
            else if (sizeFormat == 1) { headerBytes = 2; regenerated = body.le(0, 2) >> 4; }
            else { headerBytes = 3; regenerated = body.le(0, 3) >> 4; }
            if (regenerated > 131072) return 0;
            compressed = litType == 0 ? regenerated : 1;
            (void)body.sub(0, headerBytes + compressed);
        }
        View seq = body.sub(headerBytes + compressed, body.n - headerBytes - compressed);
        const unsigned huf = litType == 2 ? 1u : 0u;
        const unsigned b0 = seq.at(0);              // (an empty sequences section is malformed)
        if (b0 == 0) return seq.n == 1 ? huf : 0u;
        const size_t countBytes = b0 < 128 ? 1 : b0 < 255 ? 2 : 3;
        (void)seq.sub(0, countBytes);
        const unsigned modes = seq.at(countBytes);
        unsigned d = huf;
        for (unsigned t = 0; t < 3; ++t) if (((modes >> (6 - 2 * t)) & 3) != 3) d |= 2u << t;
        return d;
    } catch (const std::out_of_range&) { return 0; }
}

struct Block { size_t size; unsigned type, last, defines; };
// the whole blocks from `at` on, as far as they have arrived -> the position behind them
static size_t ref_blocks(View in, size_t at, std::vector<Block>& out)
{
    for (;;) {
        if (in.n - at < 3) return at;
        const uint64_t h = in.le(at, 3);
        Block b; b.last = h & 1; b.type = (h >> 1) & 3;
        const size_t body = b.type == 3 ? 0 : b.type == 1 ? 1 : (size_t)(h >> 3);
        if (in.n - at - 3 < body) return at;
        b.size = 3 + body; b.defines = b.type == 2 ? ref_defines(in.sub(at + 3, body)) : 0;
        out.push_back(b); at += b.size;
        if (b.last || b.type == 3) return at;
    }
}
static size_t scan_blocks(const uint8_t* p, size_t n, size_t at, std::vector<Block>& out)
{
    for (;;) {
        zmi::ScanBlock s;
        const size_t sz = zmi::scan_block(p + at, n - at, &s);
        if (!sz) return at;
        Block b; b.size = sz; b.type = s.type; b.last = s.last; b.defines = s.defines;
        out.push_back(b); at += sz;
        if (s.last || s.type == 3) return at;
    }
}

// a frame header's length, 0 = skippable frame (its size in *skip), -1 = not there / not a frame
static long header_bytes(View in, size_t at, size_t* skip, bool* checksum)
{
    try {
        const uint64_t magic = in.le(at, 4);
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) { *skip = (size_t)in.le(at + 4, 4) + 8; return 0; }
        if (magic != 0xFD2FB528u) return -1;
        const unsigned fhd = in.at(at + 4), single = (fhd >> 5) & 1, fcs = fhd >> 6, did = fhd & 3;
        const long n = 5 + !single + (did == 3 ? 4 : did) + (fcs == 0 ? single : 1 << fcs);
        (void)in.sub(at, (size_t)n);
        *checksum = (fhd >> 2) & 1;
        return n;
    } catch (const std::out_of_range&) { return -1; }
}

static int bad = 0;
static long long nBlocks = 0, nDefiners = 0, nInputs = 0;

// one input of exactly n bytes: every frame's blocks by both implementations, and the owner of each table after every block
static void check(const uint8_t* data, size_t n, const char* name)
{
    uint8_t* heap = (uint8_t*)malloc(n ? n : 1);
    memcpy(heap, data, n);
    const View in{ heap, n };
    size_t at = 0; ++nInputs;
    while (at < n) {
        size_t skip = 0; bool checksum = false;
        const long hb = header_bytes(in, at, &skip, &checksum);
        if (hb < 0) break;
        if (hb == 0) { at += skip; continue; }
        std::vector<Block> a, b;
        const size_t endA = scan_blocks(heap, n, at + hb, a), endB = ref_blocks(in, at + hb, b);
        if (endA != endB || a.size() != b.size()) { printf("%s (%zu bytes): the walks differ: %zu blocks to %zu, %zu blocks to %zu\n", name, n, a.size(), endA, b.size(), endB); ++bad; break; }
        int ownA[4] = { -1, -1, -1, -1 }, ownB[4] = { -1, -1, -1, -1 };
        for (size_t i = 0; i < a.size(); ++i) {
            if (a[i].size != b[i].size || a[i].type != b[i].type || a[i].last != b[i].last || a[i].defines != b[i].defines) {
                printf("%s (%zu bytes): block %zu: scan %zu/%u/%u/%x, second %zu/%u/%u/%x\n", name, n, i, a[i].size, a[i].type, a[i].last, a[i].defines, b[i].size, b[i].type, b[i].last, b[i].defines);
                ++bad;
            }
            for (int t = 0; t < 4; ++t) { if (a[i].defines & (1u << t)) ownA[t] = (int)i; if (b[i].defines & (1u << t)) ownB[t] = (int)i; }
            if (memcmp(ownA, ownB, sizeof ownA)) { printf("%s (%zu bytes): the definers differ behind block %zu\n", name, n, i); ++bad; }
            ++nBlocks; nDefiners += a[i].defines != 0;
        }
        if (a.empty() || !a.back().last) break;         // the frame is not whole
        at = endA + (checksum ? 4 : 0);
    }
    free(heap);
}

int main(int argc, char** argv)
{
    bool cut = false; int files = 0, cutFiles = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--cut")) { cut = true; continue; }
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("cannot open %s\n", argv[i]); return 2; }
        std::vector<uint8_t> d;
        uint8_t buf[65536]; size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
        fclose(f);
        check(d.data(), d.size(), argv[i]); ++files;
        if (cut) { for (size_t n = 0; n < d.size(); ++n) check(d.data(), n, argv[i]); ++cutFiles; }
    }
    printf("files %d cut %d inputs %lld blocks %lld definers %lld\n", files, cutFiles, nInputs, nBlocks, nDefiners);
    printf("done bad=%d\n", bad);
    return bad ? 1 : 0;
}
