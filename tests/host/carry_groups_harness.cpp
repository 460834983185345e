// carry_groups_harness.cpp — zmi_carry.h on the CPU, under AddressSanitizer and UBSan (tests/test_carry_groups_host.py builds and runs it).
//   arith / table / single: the carry groups of a pass in the three layout forms against a count done here: the spans partition the
//           pass's chunks in order, a span's chunks are consecutive blocks of ONE frame with the same index / kCarryGroup, its first
//           chunk leads (index a multiple of kCarryGroup; the single form: or the pass's first chunk), and there are no other groups.
//   pass:   the rounding of a pass's chunks under the single frame.
// usage: carry_groups_harness arith | table | single | pass
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "zmi_carry.h"

using namespace zmi;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// what is known of chunk c here: its frame (any id) and its block index in that frame
struct Where { uint64_t frame; uint64_t block; };

// spans[g] for g in [0, nGroups) and two more behind them, against `where`; mayLeadAnywhere: chunk 0 may begin a group inside one
static void check_partition(const std::vector<Where>& where, const std::vector<CarrySpan>& spans, uint32_t nGroups, bool firstMayLeadAnywhere, const char* what)
{
    const uint32_t nChunks = (uint32_t)where.size();
    uint32_t at = 0;
    for (uint32_t g = 0; g < nGroups; ++g) {
        const CarrySpan s = spans[g];
        CHECK(s.count >= 1 && s.count <= kCarryGroup, "%s: group %u has %u chunks", what, g, s.count);
        CHECK(s.first == at, "%s: group %u begins at %u, expected %u", what, g, s.first, at);
        if (s.first + s.count > nChunks) { CHECK(false, "%s: group %u ends behind the pass", what, g); return; }
        const Where lead = where[s.first];
        CHECK(lead.block % kCarryGroup == 0 || (firstMayLeadAnywhere && s.first == 0), "%s: group %u led by block %llu", what, g, (unsigned long long)lead.block);
        for (uint32_t k = 0; k < s.count; ++k) {
            const Where w = where[s.first + k];
            CHECK(w.frame == lead.frame && w.block == lead.block + k && w.block / kCarryGroup == lead.block / kCarryGroup,
                  "%s: group %u chunk %u: frame %llu block %llu", what, g, s.first + k, (unsigned long long)w.frame, (unsigned long long)w.block);
        }
        // the group is whole: the chunk behind it, if any, is not one of its own
        if (s.first + s.count < nChunks) {
            const Where n = where[s.first + s.count];
            CHECK(n.frame != lead.frame || n.block / kCarryGroup != lead.block / kCarryGroup, "%s: group %u stops short", what, g);
        }
        at = s.first + s.count;
    }
    CHECK(at == nChunks, "%s: %u of %u chunks in groups", what, at, nChunks);
    for (uint32_t g = nGroups; g < nGroups + 2; ++g) CHECK(spans[g].count == 0, "%s: group %u behind the last has chunks", what, g);
}

static int run_arith()
{
    int passes = 0;
    for (uint32_t fb : { 1u, 2u, 5u, 8u, 9u, 17u }) {
        // whole frames, and a last one cut anywhere
        for (uint32_t nChunks = 1; nChunks <= 3 * fb + 2; ++nChunks, ++passes) {
            std::vector<Where> where(nChunks);
            for (uint32_t c = 0; c < nChunks; ++c) where[c] = Where{ c / fb, c % fb };
            const uint32_t nGroups = carry_groups_arith(nChunks, fb);
            std::vector<CarrySpan> spans;
            for (uint32_t g = 0; g < nGroups + 2; ++g) spans.push_back(carry_span_arith(nChunks, fb, g));
            char what[64]; snprintf(what, sizeof what, "arith fb %u n %u", fb, nChunks);
            check_partition(where, spans, nGroups, false, what);
            // through the form's one door as well
            const FrameLayout lay = layout_arith(48u << 10, fb, (uint64_t)nChunks * (48u << 10));
            for (uint32_t g = 0; g < nGroups + 2; ++g) {
                const CarrySpan s = carry_span<kArith>(lay, nChunks, nullptr, 0, g);
                CHECK(s.first == spans[g].first && s.count == spans[g].count, "%s: carry_span<kArith> group %u", what, g);
            }
        }
        CHECK(carry_groups_per_frame(fb) == (fb + 7) / 8, "groups per frame of %u", fb);
    }
    printf("arith: %d passes bad=%d\n", passes, bad);
    return bad != 0;
}

static int run_table()
{
    // a batch's pass: entries of mixed lengths, each framed as the single call frames it (frames of fb blocks)
    int passes = 0;
    const uint32_t entrySets[][6] = { { 2, 5, 9, 17, 8, 0 }, { 17, 17, 2, 0, 0, 0 }, { 9, 2, 2, 2, 40, 3 }, { 16, 24, 0, 0, 0, 0 } };
    for (uint32_t fb : { 2u, 5u, 8u, 9u, 17u }) for (const auto& set : entrySets) {
        std::vector<Where> where; std::vector<uint32_t> table;
        uint64_t frame = 0;
        for (uint32_t blocks : set) {
            if (!blocks) continue;
            const FrameLayout entry = layout_arith(32u << 10, fb, (uint64_t)blocks * (32u << 10) - 5);
            for (uint32_t k = 0; k < blocks; ++k) {
                const BlockPlace p = block_place<kArith>(entry, k);
                if (p.block == 0) ++frame;
                where.push_back(Where{ frame, p.block });
                table.push_back(chunk_frame_word(p.block, (uint32_t)p.frameLen));
            }
        }
        const uint32_t nChunks = (uint32_t)table.size();
        uint32_t* leaders = new uint32_t[nChunks + 1];           // (exactly the room the host gives it)
        const uint32_t nGroups = carry_leaders_table(table.data(), nChunks, leaders);
        CHECK(nGroups == carry_leaders_table(table.data(), nChunks, nullptr), "count without a list");
        CHECK(leaders[nGroups] == nChunks, "the list's last word");
        const FrameLayout lay = layout_table(32u << 10, fb, table.data());
        std::vector<CarrySpan> spans;
        for (uint32_t g = 0; g < nGroups + 2; ++g) spans.push_back(carry_span<kTable>(lay, nChunks, leaders, nGroups, g));
        char what[64]; snprintf(what, sizeof what, "table fb %u n %u", fb, nChunks);
        check_partition(where, spans, nGroups, false, what);
        delete[] leaders;
        ++passes;
    }
    printf("table: %d passes bad=%d\n", passes, bad);
    return bad != 0;
}

static int run_single()
{
    int passes = 0;
    const uint32_t chunk = 48u << 10;
    // `at` on a group boundary, inside a group, and (a stream's batch) not even on a block boundary
    const uint64_t ats[] = { 0, (uint64_t)8 * chunk, (uint64_t)16 * chunk, (uint64_t)3 * chunk, (uint64_t)15 * chunk, (uint64_t)9 * chunk + 777, 5 };
    for (uint64_t at : ats) for (uint32_t nChunks : { 1u, 2u, 5u, 8u, 9u, 17u, 64u }) {
        std::vector<Where> where(nChunks);
        for (uint32_t c = 0; c < nChunks; ++c) where[c] = Where{ 0, (at + (uint64_t)c * chunk) / chunk };
        const uint32_t nGroups = carry_groups_single(nChunks, at, chunk);
        const FrameLayout lay = layout_single(chunk, 0x7FFFFFFFu, at, ~(uint64_t)0);
        std::vector<CarrySpan> spans;
        for (uint32_t g = 0; g < nGroups + 2; ++g) spans.push_back(carry_span<kSingle>(lay, nChunks, nullptr, 0, g));
        char what[64]; snprintf(what, sizeof what, "single at %llu n %u", (unsigned long long)at, nChunks);
        check_partition(where, spans, nGroups, true, what);
        // the block with index 8 leads a group
        for (uint32_t g = 0; g < nGroups; ++g) for (uint32_t k = 1; k < spans[g].count; ++k)
            CHECK(where[spans[g].first + k].block % kCarryGroup != 0, "%s: block %llu inside a group", what, (unsigned long long)where[spans[g].first + k].block);
        ++passes;
    }
    printf("single: %d passes bad=%d\n", passes, bad);
    return bad != 0;
}

static int run_pass()
{
    int n = 0;
    for (uint32_t p = 1; p <= 100; ++p, ++n) {
        const uint32_t r = carry_pass_chunks(p);
        CHECK(r % kCarryGroup == 0 && r >= kCarryGroup, "pass %u -> %u", p, r);
        CHECK(p < kCarryGroup ? r == kCarryGroup : (r <= p && p - r < kCarryGroup), "pass %u -> %u", p, r);
    }
    CHECK(carry_pass_chunks(16384) == 16384 && carry_pass_chunks(2 * kCarryGroup) == 2 * kCarryGroup && carry_pass_chunks(1u << 20) == (1u << 20), "whole groups stay");
    // passes of whole groups keep every pass's first chunk on a group boundary: the groups of a call do not depend on the pass length
    const uint32_t chunk = 32u << 10, total = 77;
    for (uint32_t asked : { 3u, 8u, 20u, 77u, 1000u }) {
        const uint32_t pc = carry_pass_chunks(asked);
        uint32_t groups = 0;
        for (uint32_t c0 = 0; c0 < total; c0 += pc) {
            CHECK(carry_single_lead((uint64_t)c0 * chunk, chunk) == 0, "pass of %u begins inside a group", pc);
            groups += carry_groups_single(total - c0 < pc ? total - c0 : pc, (uint64_t)c0 * chunk, chunk);
        }
        CHECK(groups == (total + kCarryGroup - 1) / kCarryGroup, "asked %u: %u groups", asked, groups);
        ++n;
    }
    printf("pass: %d cases bad=%d\n", n, bad);
    return bad != 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "arith")) return run_arith();
    if (argc == 2 && !strcmp(argv[1], "table")) return run_table();
    if (argc == 2 && !strcmp(argv[1], "single")) return run_single();
    if (argc == 2 && !strcmp(argv[1], "pass")) return run_pass();
    fprintf(stderr, "usage: %s arith | table | single | pass\n", argv[0]);
    return 2;
}
