// frame_layout_harness.cpp — zmi_frame.h on the CPU, under AddressSanitizer and UBSan (tests/test_frame_layout_host.py builds and runs it).
//   header: the size the match finder reserves (frame_header_bytes) against the bytes the sequence encoder writes (frame_header_write),
//           into a heap block of exactly that size, and a parser written from the zstd format (RFC 8878 section 3.1.1.1) reads them back.
//   place:  a block's place in its frame in the arithmetic, the table and the single-frame form, against a count done here.
// usage: frame_layout_harness header | place
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "zmi_frame.h"

using namespace zmi;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- a frame header as the format describes it ----
struct Parsed { bool ok; uint32_t size; bool single, checksum, hasContentSize; uint64_t contentSize; uint32_t windowLog, mantissa; uint32_t dictIdBytes, dictID; };
static uint64_t le(const uint8_t* p, uint32_t n) { uint64_t v = 0; for (uint32_t i = 0; i < n; ++i) v |= (uint64_t)p[i] << (8 * i); return v; }
static Parsed parse_header(const uint8_t* p, uint32_t avail)
{
    Parsed r = {};
    if (avail < 5 || le(p, 4) != 0xFD2FB528u) return r;
    const uint8_t fhd = p[4];
    const uint32_t fcsFlag = fhd >> 6, didFlag = fhd & 3;
    r.single = (fhd >> 5) & 1; r.checksum = (fhd >> 2) & 1;
    if (fhd & 0x18) return r;                       // the unused and the reserved bit
    uint32_t at = 5;
    if (!r.single) {
        if (at + 1 > avail) return r;
        r.windowLog = 10 + (p[at] >> 3); r.mantissa = p[at] & 7; ++at;
    }
    r.dictIdBytes = didFlag == 3 ? 4 : didFlag;
    if (at + r.dictIdBytes > avail) return r;
    r.dictID = (uint32_t)le(p + at, r.dictIdBytes); at += r.dictIdBytes;
    const uint32_t fcsBytes = fcsFlag == 0 ? (r.single ? 1 : 0) : fcsFlag == 1 ? 2 : fcsFlag == 2 ? 4 : 8;
    if (at + fcsBytes > avail) return r;
    r.hasContentSize = fcsBytes != 0;
    r.contentSize = le(p + at, fcsBytes) + (fcsBytes == 2 ? 256 : 0); at += fcsBytes;
    r.size = at; r.ok = true;
    return r;
}

static int run_header()
{
    const uint64_t lens[] = { 0, 1, 255, 256, 65791, 65792, 0xFFFFFFFFull, 0x100000000ull };
    const uint32_t widths[] = { 0, 1, 2, 4 };
    // the three forms: single segment | no content size | an explicit windowLog with and without the content size
    const struct { uint8_t noContentSize, windowLog; } forms[] = { {0, 0}, {1, 0}, {0, 10}, {1, 10}, {0, 17}, {1, 17}, {0, 27}, {1, 27} };
    int n = 0;
    for (uint64_t len : lens) for (uint32_t w : widths) for (int cks = 0; cks < 2; ++cks) for (const auto& f : forms) {
        FrameHeaderSpec h = {};
        h.dictID = w == 1 ? 0xABu : w == 2 ? 0xABCDu : 0xABCDEF12u;     // (width 0: a dictionary whose ID ZSTD_c_dictIDFlag = 0 keeps out)
        h.dictIdBytes = (uint8_t)w; h.checksum = (uint8_t)cks; h.noContentSize = f.noContentSize; h.windowLog = f.windowLog;
        if (w) CHECK(dict_id_bytes(h.dictID) == w, "width of %x", h.dictID);
        const uint32_t size = frame_header_bytes(h, len);
        CHECK(size >= 6 && size <= 18, "size %u", size);
        uint8_t* exact = new uint8_t[size];          // (a byte too many is the sanitizer's finding)
        const uint32_t wrote = frame_header_write(h, len, exact);
        CHECK(wrote == size, "len %llu w %u cks %d form %u/%u: size %u, wrote %u", (unsigned long long)len, w, cks, f.noContentSize, f.windowLog, size, wrote);
        uint8_t guarded[32]; memset(guarded, 0xA5, sizeof guarded);
        frame_header_write(h, len, guarded);
        for (uint32_t i = size; i < sizeof guarded; ++i) CHECK(guarded[i] == 0xA5, "byte %u behind a header of %u", i, size);
        CHECK(!memcmp(guarded, exact, size), "two writes differ");
        const Parsed p = parse_header(exact, size);
        CHECK(p.ok && p.size == size, "parser: ok %d size %u of %u", p.ok, p.size, size);
        CHECK(p.checksum == (cks != 0), "checksum flag");
        CHECK(p.dictIdBytes == w && p.dictID == (w ? h.dictID : 0u), "dictID %x in %u bytes", p.dictID, p.dictIdBytes);
        CHECK(p.single == (!f.noContentSize && !f.windowLog), "single segment");
        // the content size: asked for, and the format has a field for it (behind a window descriptor none below 256 bytes)
        const bool wantSize = !f.noContentSize && (p.single || len >= 256);
        CHECK(p.hasContentSize == wantSize, "content size present %d, wanted %d", p.hasContentSize, wantSize);
        if (p.hasContentSize) CHECK(p.contentSize == len, "content size %llu of %llu", (unsigned long long)p.contentSize, (unsigned long long)len);
        if (!p.single) {
            CHECK(p.mantissa == 0, "mantissa %u", p.mantissa);
            if (f.windowLog) CHECK(p.windowLog == f.windowLog, "windowLog %u of %u", p.windowLog, f.windowLog);
            else {      // the smallest power of two, at least 1 KiB, that holds the frame
                CHECK(((uint64_t)1 << p.windowLog) >= len && p.windowLog >= 10, "window 2^%u below the frame", p.windowLog);
                CHECK(p.windowLog == 10 || ((uint64_t)1 << (p.windowLog - 1)) < len, "window 2^%u not the smallest", p.windowLog);
            }
        }
        delete[] exact;
        ++n;
    }
    printf("header: %d combinations bad=%d\n", n, bad);
    return bad != 0;
}

static int run_place()
{
    const struct { uint32_t chunk, blocks; } geoms[] = { {16u << 10, 4}, {48u << 10, 5}, {32u << 10, 8} };
    int nChunksSeen = 0, nSingle = 0;
    for (const auto& g : geoms) {
        const uint64_t chunk = g.chunk, span = chunk * g.blocks;
        const uint64_t sizes[] = { 1, chunk - 1, chunk, chunk + 1, 3 * chunk, span, span + 1, 2 * span + 5 };
        for (uint64_t S : sizes) {
            const uint32_t nChunks = (uint32_t)((S + chunk - 1) / chunk);
            const FrameLayout arith = layout_arith(g.chunk, g.blocks, S);
            // the table as the host fills it for a batch's entry
            std::vector<uint32_t> table(nChunks);
            for (uint32_t c = 0; c < nChunks; ++c) {
                const BlockPlace a = block_place<kArith>(arith, c);
                CHECK(a.block < kFrameWordBlocks && a.frameLen < kFrameWordLen, "word fields");
                table[c] = chunk_frame_word(a.block, (uint32_t)a.frameLen);
            }
            const FrameLayout tab = layout_table(g.chunk, g.blocks, table.data());
            const FrameLayout one = layout_single(g.chunk, g.blocks, 0, S);
            for (uint32_t c = 0; c < nChunks; ++c, ++nChunksSeen) {
                // counted here: the frame that holds the chunk's first byte
                const uint64_t pos = c * chunk, fStart = pos / span * span, fLen = S - fStart < span ? S - fStart : span;
                const BlockPlace a = block_place<kArith>(arith, c), t = block_place<kTable>(tab, c);
                CHECK(a.block == (pos - fStart) / chunk && a.frameLen == fLen && a.front == pos - fStart && a.last == (pos + chunk >= fStart + fLen),
                      "arith S %llu c %u: block %u len %llu front %llu last %d", (unsigned long long)S, c, a.block, (unsigned long long)a.frameLen, (unsigned long long)a.front, a.last);
                CHECK(t.block == a.block && t.frameLen == a.frameLen && t.front == a.front && t.last == a.last, "table S %llu c %u", (unsigned long long)S, c);
                if (S <= span) {        // one frame: the single-frame form states the same (its block index: first or not)
                    const BlockPlace s = block_place<kSingle>(one, c);
                    CHECK((s.block == 0) == (a.block == 0) && s.frameLen == a.frameLen && s.front == a.front && s.last == a.last, "single S %llu c %u", (unsigned long long)S, c);
                    ++nSingle;
                }
            }
        }
    }
    // the "independent blocks" flag travels in bit 31 of the finder's frameBlocks argument
    for (uint32_t fb : { 0u, 1u, 4u, 0x7FFFFFFFu }) for (int ind = 0; ind < 2; ++ind) {
        const FrameBlocksArg d = frame_blocks_decode(frame_blocks_encode(fb, ind != 0));
        CHECK(d.frameBlocks == fb && d.independent == (ind != 0), "frameBlocks %u independent %d", fb, ind);
    }
    printf("place: %d chunks, %d of them also in the single-frame form bad=%d\n", nChunksSeen, nSingle, bad);
    return bad != 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "header")) return run_header();
    if (argc == 2 && !strcmp(argv[1], "place")) return run_place();
    fprintf(stderr, "usage: %s header | place\n", argv[0]);
    return 2;
}
