// batch_plan_harness.cpp — zmi_batch_plan.h on the CPU, under AddressSanitizer and UBSan (tests/test_batch_plan_host.py builds and runs it).
// For lists of entries the plan — verdicts, entFirst, and per chunk slot from / len / frame word, evaluated entry by entry and slot by
// slot as the plan kernels of frame.hip evaluate them — is held against a plain restatement of compress_entries' host loop
// (zstd_mi355x.hip): walk the entries in order, check the arguments, cut each good one into chunks with layout_arith / block_place.
//   plan:  seeded and hand-picked size lists under five framings, without a limit, and under a bound of three chunks and a bit.
//   limit: the same lists under maxChunks = total, total - 1, half, 1: who is refused, and that nothing in front of the cut changes.
//   owner: plan_owner over hand-made entFirst tables with runs of entries that own nothing.
// usage: batch_plan_harness plan | limit | owner
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "zmi_batch_plan.h"

using namespace zmi;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Entry { u64 src, size, dst, cap; };
struct Geometry { u32 chunkBytes, frameBlocks; const char* name; };
struct Plan { std::vector<u32> verdict, first; std::vector<u64> from; std::vector<u32> len, frame; };

static const u64 kDummy = 0x7000;
static const u32 kEmptyLen = 9;

// ---- the reference: compress_entries' loop, with the async call's extra checks (the bound, the empty frame's room) and the limit ----
static Plan host_loop(const std::vector<Entry>& in, u64 bound, const Geometry& g, u32 maxChunks)
{
    Plan p;
    u32 ck = 0; u64 counted = 0;
    for (const Entry& x : in) {
        p.first.push_back(ck);
        if (x.size > bound || (x.size && !x.src)) { p.verdict.push_back(kErrSrcSizeWrong); continue; }
        if (!x.dst) { p.verdict.push_back(x.cap ? kErrDstBufferNull : kErrDstSizeTooSmall); continue; }
        if (!x.size) { p.verdict.push_back(x.cap < kEmptyLen ? (u32)kErrDstSizeTooSmall : (u32)kAsyncEmpty); continue; }
        counted += (x.size + g.chunkBytes - 1) / g.chunkBytes;
        if (counted > maxChunks) { p.verdict.push_back(kErrWorkSpaceTooSmall); continue; }
        p.verdict.push_back(kAsyncGood);
        const FrameLayout entry = layout_arith(g.chunkBytes, g.frameBlocks, x.size);
        for (u64 o = 0, k = 0; o < x.size; o += g.chunkBytes, ++ck, ++k) {
            p.from.push_back(x.src + o);
            p.len.push_back((u32)(x.size - o < g.chunkBytes ? x.size - o : g.chunkBytes));
            u32 word = 0;
            if (g.frameBlocks) { const BlockPlace at = block_place<kArith>(entry, (u32)k); word = chunk_frame_word(at.block, (u32)at.frameLen); }
            p.frame.push_back(word);
        }
    }
    p.first.push_back(ck);
    return p;
}

// ---- the plan, as the kernels evaluate it: per entry (a serial sum in the place of the scan), then per chunk slot ----
static Plan device_plan(const std::vector<Entry>& in, u64 bound, const Geometry& g, u32 maxChunks, u32 nLaunch)
{
    const u32 n = (u32)in.size();
    Plan p;
    std::vector<u32> cnt(n), raw(n);
    u32 cut = kPlanNoCut; u64 run = 0;
    for (u32 e = 0; e < n; ++e) {
        raw[e] = plan_verdict(in[e].src, in[e].size, in[e].dst, in[e].cap, bound, kEmptyLen);
        cnt[e] = plan_chunks(raw[e], in[e].size, g.chunkBytes);
        if (plan_is_cut(run, cnt[e], maxChunks)) { CHECK(cut == kPlanNoCut, "a second cut at entry %u", e); cut = (u32)run; }
        run += cnt[e];
    }
    run = 0;
    for (u32 e = 0; e < n; ++e) {
        p.first.push_back(plan_first((u32)run, cut));
        p.verdict.push_back(plan_limited(raw[e], run, cnt[e], maxChunks));
        run += cnt[e];
    }
    p.first.push_back(plan_first((u32)run, cut));
    const u32 total = p.first[n];
    CHECK(total <= nLaunch, "total %u above the grid %u", total, nLaunch);
    for (u32 c = 0; c < nLaunch; ++c) {
        PlanChunk r = plan_chunk_idle(kDummy);
        if (c < total) {
            const u32 e = plan_owner(p.first.data(), n, c);
            CHECK(e < n && p.first[e] <= c && c < p.first[e + 1] && p.verdict[e] == kAsyncGood, "slot %u: owner %u", c, e);
            if (e >= n) continue;
            r = plan_chunk(in[e].src, in[e].size, c - p.first[e], g.chunkBytes, g.frameBlocks);
        }
        p.from.push_back(r.from); p.len.push_back(r.len); p.frame.push_back(r.frameWord);
    }
    return p;
}

static u32 compare(const std::vector<Entry>& in, u64 bound, const Geometry& g, u32 maxChunks, const char* what)
{
    const Plan want = host_loop(in, bound, g, maxChunks);
    const u32 total = want.first.back(), perEntry = (u32)((bound + g.chunkBytes - 1) / g.chunkBytes);
    const u64 most = (u64)in.size() * perEntry;
    const u32 nLaunch = (u32)(most < maxChunks ? most : maxChunks);
    const Plan got = device_plan(in, bound, g, maxChunks, nLaunch);
    CHECK(got.verdict == want.verdict, "%s %s: verdicts differ", g.name, what);
    CHECK(got.first == want.first, "%s %s: entFirst differs", g.name, what);
    CHECK(got.from.size() == nLaunch, "%s %s: %zu slots for a grid of %u", g.name, what, got.from.size(), nLaunch);
    for (u32 c = 0; c < nLaunch && c < got.from.size(); ++c) {
        if (c < total) {
            CHECK(got.from[c] == want.from[c] && got.len[c] == want.len[c] && got.frame[c] == want.frame[c], "%s %s: chunk %u: from %llx/%llx len %u/%u word %x/%x",
                  g.name, what, c, (unsigned long long)got.from[c], (unsigned long long)want.from[c], got.len[c], want.len[c], got.frame[c], want.frame[c]);
            CHECK(got.len[c] >= 1 && got.len[c] <= g.chunkBytes, "%s %s: chunk %u of %u bytes", g.name, what, c, got.len[c]);
        } else
            CHECK(got.from[c] == kDummy && got.len[c] == 1 && frame_word_block(got.frame[c]) == 0 && frame_word_len(got.frame[c]) == 1, "%s %s: idle slot %u", g.name, what, c);
    }
    return total;
}

static u64 rnd_state = 88172645463325252ull;
static u64 rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }

static const Geometry kGeometries[] = { { 16u << 10, 4, "16Kx4" }, { 48u << 10, 5, "48Kx5" }, { 32u << 10, 8, "32Kx8" }, { 32u << 10, 0, "32Kx0" }, { 64u << 10, 0, "64Kx0" } };

// the size lists: the edges of the geometry, failed and empty entries between good ones, then seeded lists
static std::vector<std::vector<Entry>> lists_for(const Geometry& g, u64 bound)
{
    const u64 cb = g.chunkBytes, span = cb * (g.frameBlocks ? g.frameBlocks : 1u);
    std::vector<u64> edges = { 0, 1, cb - 1, cb, cb + 1, span - 1, span, span + 1, 2 * span - 1, 2 * span + 1, kAsyncBoundMax };
    std::vector<std::vector<Entry>> out;
    u64 at = 0x10000000ull;
    auto good = [&](u64 S) { Entry x{ at, S, at + 0x40000000ull, S + 64 }; at += S + 5; return x; };
    std::vector<Entry> a;
    for (u64 S : edges) if (S <= bound) a.push_back(good(S));
    out.push_back(a);
    std::vector<Entry> b;           // failed entries in between, of every kind
    for (size_t i = 0; i < a.size(); ++i) {
        b.push_back(a[i]);
        Entry f = good(cb + 3);
        switch (i % 6) {
        case 0: f.src = 0; break;                       // NULL source with a size
        case 1: f.size = bound + 1; break;              // above the bound
        case 2: f.dst = 0; break;                       // NULL destination, capacity > 0
        case 3: f.dst = 0; f.cap = 0; break;            // NULL destination, capacity 0
        case 4: f.size = 0; f.cap = kEmptyLen - 1; break;   // empty without room for the empty frame
        default: f.size = 0; f.src = 0; break;          // empty (a NULL source is fine then)
        }
        b.push_back(f);
    }
    out.push_back(b);
    for (int list = 0; list < 6; ++list) {
        std::vector<Entry> r;
        const u32 n = 1 + (u32)(rnd() % 300);
        for (u32 i = 0; i < n; ++i) {
            const u64 pick = rnd() % 10;
            u64 S = pick < 6 ? 1 + rnd() % (3 * cb) : pick < 8 ? 1 + rnd() % bound : edges[rnd() % edges.size()];
            if (S > bound) S = bound;
            Entry x = good(S);
            if (rnd() % 11 == 0) x.src = 0;
            if (rnd() % 13 == 0) x.dst = 0;
            if (rnd() % 17 == 0) x.size = bound + 1 + rnd() % 100;
            r.push_back(x);
        }
        out.push_back(r);
    }
    return out;
}

static void part_plan()
{
    u32 lists = 0; u64 chunks = 0;
    for (const Geometry& g : kGeometries)
        for (const auto& in : lists_for(g, kAsyncBoundMax)) { chunks += compare(in, kAsyncBoundMax, g, 0xFFFFFFFFu, "plan"); ++lists; }
    // a bound below the edges: everything above it fails
    for (const Geometry& g : kGeometries)
        for (const auto& in : lists_for(g, 3 * (u64)g.chunkBytes + 7)) { chunks += compare(in, 3 * (u64)g.chunkBytes + 7, g, 0xFFFFFFFFu, "bound"); ++lists; }
    printf("plan: %u lists %llu chunks bad=%d\n", lists, (unsigned long long)chunks, bad);
}

static void part_limit()
{
    u32 runs = 0;
    for (const Geometry& g : kGeometries)
        for (const auto& in : lists_for(g, kAsyncBoundMax)) {
            const Plan all = host_loop(in, kAsyncBoundMax, g, 0xFFFFFFFFu);
            const u32 total = all.first.back();
            const u32 limits[] = { total, total - 1, total / 2, 1 };
            for (u32 lim : limits) {
                if (!total || !lim) continue;
                const u32 kept = compare(in, kAsyncBoundMax, g, lim, "limit");
                ++runs;
                CHECK(kept <= lim, "%s: %u chunks kept under a limit of %u", g.name, kept, lim);
                // the rule in the issue's words: refused iff the inclusive sum over the good entries exceeds the limit
                const Plan p = host_loop(in, kAsyncBoundMax, g, lim);
                u64 sum = 0; bool seen = false; u32 refused = 0;
                for (size_t e = 0; e < in.size(); ++e) {
                    if (all.verdict[e] != kAsyncGood) { CHECK(p.verdict[e] == all.verdict[e], "%s: failed entry %zu changed its answer", g.name, e); continue; }
                    sum += (in[e].size + g.chunkBytes - 1) / g.chunkBytes;
                    const bool out = sum > lim;
                    CHECK((p.verdict[e] == kErrWorkSpaceTooSmall) == out, "%s: entry %zu under limit %u", g.name, e, lim);
                    CHECK(!seen || out, "%s: a good entry %zu behind a refused one", g.name, e);
                    seen = seen || out; refused += out;
                    if (!out) CHECK(p.first[e] == all.first[e], "%s: entry %zu moved", g.name, e);
                }
                if (lim == total) CHECK(refused == 0, "%s: %u refused at the total", g.name, refused);
                if (lim == total - 1) {
                    size_t last = in.size();
                    for (size_t e = 0; e < in.size(); ++e) if (all.verdict[e] == kAsyncGood) last = e;
                    CHECK(refused == 1 && p.verdict[last] == kErrWorkSpaceTooSmall, "%s: total - 1 refuses exactly the last good entry (%u refused)", g.name, refused);
                }
            }
        }
    printf("limit: %u runs bad=%d\n", runs, bad);
}

static void part_owner()
{
    u32 tables = 0;
    const std::vector<std::vector<u32>> firsts = {
        { 0, 1 }, { 0, 0, 0, 3 }, { 0, 3, 3, 3 }, { 0, 2, 2, 5, 5, 5, 6 }, { 0, 0, 1, 1, 2, 2, 3, 3 }, { 0, 256, 256, 257, 513 },
    };
    for (const auto& f : firsts) {
        const u32 n = (u32)f.size() - 1;
        for (u32 c = 0; c < f[n]; ++c) {
            const u32 e = plan_owner(f.data(), n, c);
            CHECK(e < n && f[e] <= c && c < f[e + 1], "table %u chunk %u: owner %u", tables, c, e);
        }
        ++tables;
    }
    // 16384 entries of 1 .. 3 chunks with gaps
    std::vector<u32> f(16385);
    u32 at = 0;
    for (u32 e = 0; e < 16384; ++e) { f[e] = at; at += (u32)(rnd() % 4); }
    f[16384] = at;
    for (u32 c = 0; c < at; ++c) { const u32 e = plan_owner(f.data(), 16384, c); CHECK(f[e] <= c && c < f[e + 1], "large table chunk %u: owner %u", c, e); }
    printf("owner: %u tables bad=%d\n", tables + 1, bad);
}

int main(int argc, char** argv)
{
    const char* part = argc > 1 ? argv[1] : "";
    if (!strcmp(part, "plan")) part_plan();
    else if (!strcmp(part, "limit")) part_limit();
    else if (!strcmp(part, "owner")) part_owner();
    else { printf("usage: batch_plan_harness plan | limit | owner\n"); return 2; }
    return bad ? 1 : 0;
}
