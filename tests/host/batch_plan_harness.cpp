// batch_plan_harness.cpp — zmi_batch_plan.h on the CPU, under AddressSanitizer and UBSan (tests/test_batch_plan_host.py builds and runs it).
// For lists of entries the plan — verdicts, entFirst, and per chunk slot from / len / frame word, evaluated entry by entry and slot by
// slot as the plan kernels of frame.hip evaluate them — is held against a plain restatement of compress_entries' host loop
// (zstd_mi355x.hip): walk the entries in order, check the arguments, cut each good one into chunks with layout_arith / block_place.
//   plan:  seeded and hand-picked size lists under five framings, without a limit, and under a bound of three chunks and a bit.
//   limit: the same lists under maxChunks = total, total - 1, half, 1: who is refused, and that nothing in front of the cut changes.
//   owner: plan_owner over hand-made entFirst tables with runs of entries that own nothing.
// And zmi_batch_pass.h, which compress_entries calls for its host decisions, so that the loop that ships is the loop under test:
//   fill:   batch_pass_fill over the same lists == the restatement == the device plan, with entFirst, entDst, entCap, seek rows, span.
//   layout: batch_pass_tab == the inline offset arithmetic it replaced; the four tables' columns apart, aligned and covered.
//   cut:    batch_pass_cut == compress_entries' pass loop and ZSTDMI_compressPack's round expression as they were.
//   group:  same_group == the grouping condition compress_entries held inline, in both meanings (with and without per-entry CDicts).
// usage: batch_plan_harness plan | limit | owner | fill | layout | cut | group
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "zmi_batch_plan.h"
#include "zmi_batch_pass.h"

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

// ---- zmi_batch_pass.h: the host loop itself ----
// fill: the good entries of a list are one pass's members.  batch_pass_fill writes them into an image laid out by batch_pass_tab
// (allocated to exactly its bytes, so that a store outside it is AddressSanitizer's), and its columns are held against the
// restatement and the device plan.
static u32 fill_compare(const std::vector<Entry>& in, const Geometry& g, bool withDst, bool withSeek)
{
    const Plan want = host_loop(in, kAsyncBoundMax, g, 0xFFFFFFFFu);
    const u32 total = want.first.back();
    const Plan dev = device_plan(in, kAsyncBoundMax, g, 0xFFFFFFFFu, total);
    std::vector<size_t> members;
    std::vector<const u8*> srcs; std::vector<size_t> sizes, caps; std::vector<u8*> dsts; std::vector<u32> seekIdx;
    u64 lo = ~(u64)0, hi = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        srcs.push_back((const u8*)(uintptr_t)in[i].src); sizes.push_back((size_t)in[i].size);
        dsts.push_back((u8*)(uintptr_t)in[i].dst); caps.push_back((size_t)in[i].cap); seekIdx.push_back((u32)(7 * i + 3));
        if (want.verdict[i] != kAsyncGood) continue;
        members.push_back(i);
        if (in[i].dst < lo) lo = in[i].dst;
        if (in[i].dst + in[i].cap > hi) hi = in[i].dst + in[i].cap;
    }
    const u32 nEnt = (u32)members.size();
    if (!nEnt) return 0;
    const BatchPassTab t = batch_pass_tab(total, nEnt, g.frameBlocks != 0, withSeek, 0, false);
    std::vector<u8> image(t.bytes, 0xEE);
    const BatchPassCols h = batch_pass_cols(t, image.data());
    CHECK((h.frame != nullptr) == (g.frameBlocks != 0) && (h.entSeek != nullptr) == withSeek && !h.chunkSlot && !h.slots && !h.leaders, "%s: columns that are not there", g.name);
    const BatchPassEntries e = { members.data(), nEnt, srcs.data(), sizes.data(), withDst ? dsts.data() : nullptr, withDst ? caps.data() : nullptr, withSeek ? seekIdx.data() : nullptr };
    const BatchPassSpan at = batch_pass_fill(e, g.chunkBytes, g.frameBlocks, h);
    if (withDst) CHECK(at.lo == lo && at.span == hi - lo, "%s: span %llx + %llu", g.name, (unsigned long long)at.lo, (unsigned long long)at.span);
    else CHECK(at.lo == ~(uintptr_t)0 && at.span == 0, "%s: a span without destinations", g.name);
    for (u32 m = 0; m < nEnt; ++m) {
        const Entry& x = in[members[m]];
        CHECK(h.entFirst[m] == want.first[members[m]] && h.entFirst[m] == dev.first[members[m]], "%s: entFirst[%u] = %u", g.name, m, h.entFirst[m]);
        CHECK(h.entDst[m] == (withDst ? x.dst - lo : 0) && h.entCap[m] == (withDst ? x.cap : ~(u64)0), "%s: entDst / entCap of member %u", g.name, m);
        if (withSeek) CHECK(h.entSeek[m] == seekIdx[members[m]], "%s: entSeek[%u]", g.name, m);
    }
    CHECK(h.entFirst[nEnt] == total, "%s: entFirst[nEnt] = %u of %u", g.name, h.entFirst[nEnt], total);
    for (u32 c = 0; c < total; ++c) {
        CHECK(h.from[c] == want.from[c] && h.len[c] == want.len[c] && (!g.frameBlocks || h.frame[c] == want.frame[c]), "%s: chunk %u against the restatement: from %llx/%llx len %u/%u",
              g.name, c, (unsigned long long)h.from[c], (unsigned long long)want.from[c], h.len[c], want.len[c]);
        CHECK(h.from[c] == dev.from[c] && h.len[c] == dev.len[c] && (!g.frameBlocks || h.frame[c] == dev.frame[c]), "%s: chunk %u against the device plan", g.name, c);
    }
    return total;
}
static void part_fill()
{
    u32 lists = 0; u64 chunks = 0;
    for (const Geometry& g : kGeometries)
        for (const auto& in : lists_for(g, kAsyncBoundMax)) {
            chunks += fill_compare(in, g, true, false);
            fill_compare(in, g, true, true); fill_compare(in, g, false, false); fill_compare(in, g, false, true);
            ++lists;
        }
    printf("fill: %u lists %llu chunks bad=%d\n", lists, (unsigned long long)chunks, bad);
}

// layout: batch_pass_tab against the offset arithmetic compress_entries held inline before the table had a name, restated literally;
// then, for all four tables, that no two columns overlap, that the u64 and CDictSlot columns are 8-aligned and that `bytes` covers the last
struct Column { const char* name; size_t at, bytes; bool wide; };
static void check_columns(const char* tab, const std::vector<Column>& cols, size_t bytes, bool exact)
{
    size_t end = 0;
    for (const Column& c : cols) {
        CHECK(c.at >= end, "%s: column %s at %zu begins inside the one before it (ends %zu)", tab, c.name, c.at, end);
        CHECK(!c.wide || c.at % 8 == 0, "%s: column %s at %zu is not 8-aligned", tab, c.name, c.at);
        end = c.at + c.bytes;
    }
    CHECK(exact ? bytes == ((end + 7) & ~(size_t)7) || bytes == end : bytes >= end, "%s: %zu bytes for columns that end at %zu", tab, bytes, end);
}
static void part_layout()
{
    u32 cases = 0;
    const u32 chunkCounts[] = { 1, 2, 3, 255, 256, 16384 }, slotCounts[] = { 0, 2, 3 };
    for (u32 nCh : chunkCounts) for (u32 entSel = 0; entSel < 3; ++entSel) {
        const u32 nEnt = entSel == 0 ? 1 : entSel == 1 ? 2 : nCh;
        if (nEnt > nCh) continue;       // (a pass's entries have a chunk each)
        for (int frameBlocks = 0; frameBlocks < 2; ++frameBlocks) for (int seekOn = 0; seekOn < 2; ++seekOn) for (u32 nSlots : slotCounts) for (int carryOn = 0; carryOn < 2; ++carryOn) {
            const void* seekIdx = seekOn ? &cases : nullptr;
            const bool set = nSlots != 0, carry = carryOn != 0;
            // (the parent's lines, with slotTab.size() = nSlots)
            const size_t atDst = (size_t)nCh * 8, atCap = atDst + (size_t)nEnt * 8, atLen = atCap + (size_t)nEnt * 8, atFirst = atLen + (size_t)nCh * 4;
            const size_t atFrame = atFirst + ((size_t)nEnt + 1) * 4;
            const size_t atSeek = atFrame + (frameBlocks ? (size_t)nCh * 4 : 0);
            const size_t atChunkSlot = atSeek + (seekIdx ? (size_t)nEnt * 4 : 0);
            const size_t atSlots = (atChunkSlot + (set ? (size_t)nCh * 4 : 0) + 7) & ~(size_t)7;
            const size_t atLead = (atSlots + (set ? nSlots * sizeof(CDictSlot) : 0) + 7) & ~(size_t)7;
            const size_t tabBytes = (atLead + (carry ? ((size_t)nCh + 1) * 4 : 0) + 7) & ~(size_t)7;
            const BatchPassTab t = batch_pass_tab(nCh, nEnt, frameBlocks != 0, seekOn != 0, nSlots, carry);
            CHECK(t.atDst == atDst && t.atCap == atCap && t.atLen == atLen && t.atFirst == atFirst && t.atFrame == atFrame && t.atSeek == atSeek && t.atChunkSlot == atChunkSlot &&
                  t.atSlots == atSlots && t.atLead == atLead && t.bytes == tabBytes, "nCh %u nEnt %u frame %d seek %d slots %u carry %d: offsets differ from the parent's", nCh, nEnt, frameBlocks, seekOn, nSlots, carryOn);
            std::vector<Column> cols = { { "from", 0, (size_t)nCh * 8, true }, { "entDst", t.atDst, (size_t)nEnt * 8, true }, { "entCap", t.atCap, (size_t)nEnt * 8, true },
                                         { "len", t.atLen, (size_t)nCh * 4, false }, { "entFirst", t.atFirst, ((size_t)nEnt + 1) * 4, false } };
            if (frameBlocks) cols.push_back({ "frame", t.atFrame, (size_t)nCh * 4, false });
            if (seekOn) cols.push_back({ "entSeek", t.atSeek, (size_t)nEnt * 4, false });
            if (set) { cols.push_back({ "chunkSlot", t.atChunkSlot, (size_t)nCh * 4, false }); cols.push_back({ "slots", t.atSlots, nSlots * sizeof(CDictSlot), true }); }
            if (carry) cols.push_back({ "leaders", t.atLead, ((size_t)nCh + 1) * 4, false });
            check_columns("BatchPassTab", cols, t.bytes, true);
            CHECK(t.bytes % 8 == 0, "the sizes behind the table at %zu are not 8-aligned", t.bytes);
            // the view: every column where the table says, on any base
            std::vector<u8> image(t.bytes + 8);
            const BatchPassCols v = batch_pass_cols(t, image.data());
            CHECK((u8*)v.from == image.data() && (u8*)v.entDst == image.data() + atDst && (u8*)v.entCap == image.data() + atCap && (u8*)v.len == image.data() + atLen &&
                  (u8*)v.entFirst == image.data() + atFirst && (u8*)v.got == image.data() + tabBytes, "the view's columns");
            CHECK((u8*)v.frame == (frameBlocks ? image.data() + atFrame : nullptr) && (u8*)v.entSeek == (seekOn ? image.data() + atSeek : nullptr) &&
                  (u8*)v.chunkSlot == (set ? image.data() + atChunkSlot : nullptr) && (u8*)v.slots == (set ? image.data() + atSlots : nullptr) &&
                  (u8*)v.leaders == (carry ? image.data() + atLead : nullptr), "the view's optional columns");
            ++cases;
        }
        // the three tables of the calls enqueued from the device
        const AsyncTab a = async_tab(nCh);
        check_columns("AsyncTab", { { "from", 0, (size_t)nCh * 8, true }, { "entDst", a.atDst, (size_t)nCh * 8, true }, { "entCap", a.atCap, (size_t)nCh * 8, true },
                                    { "len", a.atLen, (size_t)nCh * 4, false }, { "entFirst", a.atFirst, ((size_t)nCh + 1) * 4, false }, { "verdict", a.atVerdict, (size_t)nCh * 4, false },
                                    { "dummy", a.atDummy, 8, true } }, a.bytes, true);
        const AsyncPlanTab q = async_plan_tab(nEnt, nCh);
        check_columns("AsyncPlanTab", { { "from", 0, (size_t)nCh * 8, true }, { "src", q.atSrc, (size_t)nEnt * 8, true }, { "size", q.atSize, (size_t)nEnt * 8, true },
                                        { "dst", q.atDst, (size_t)nEnt * 8, true }, { "cap", q.atCap, (size_t)nEnt * 8, true }, { "len", q.atLen, (size_t)nCh * 4, false },
                                        { "frame", q.atFrame, (size_t)nCh * 4, false }, { "first", q.atFirst, ((size_t)nEnt + 1) * 4, false },
                                        { "verdict", q.atVerdict, (size_t)nEnt * 4, false }, { "dummy", q.atDummy, 8, true } }, q.bytes, true);
        const u32 frameCounts[] = { 1, 2, 5 };
        for (u32 F : frameCounts) {
            const PackAsyncLayout k = pack_async_tab(nEnt, F);
            check_columns("PackAsyncLayout", { { "entAt", 0, (size_t)nEnt * 8, true }, { "state", k.atState, (size_t)kPackStateWords * 8, true }, { "entRow", k.atRow, (size_t)nEnt * 4, false },
                                               { "rows", k.atRows, (size_t)nEnt * F * 8, true } }, k.bytes, false);
        }
        cases += 5;
    }
    printf("layout: %u cases bad=%d\n", cases, bad);
}

// cut: batch_pass_cut over runs of chunk counts against compress_entries' loop and the round cut ZSTDMI_compressPack stated for
// itself, both as they stood before the cut had a name
static void part_cut()
{
    u32 runs = 0;
    const u32 limits[] = { 1, 2, 16384 };
    for (u32 limit : limits) {
        std::vector<std::vector<u32>> lists = {
            { 1 }, { limit }, { limit, limit, limit }, { 1, limit, 1 }, { limit, 1, limit }, { limit - limit / 2, limit / 2 + 1, 1 },       // exactly the limit; above what is left
            { 1, 1, 1, 1, 1 }, { limit + 1 }, { 1, limit + 1, 1 }, { limit + 1, limit + 1 },                                                // (more than a pass: never batched, but a pass's first all the same)
        };
        for (int list = 0; list < 8; ++list) {
            std::vector<u32> r;
            const u32 n = 1 + (u32)(rnd() % 200);
            for (u32 i = 0; i < n; ++i) r.push_back(1 + (u32)(rnd() % (rnd() % 3 ? 4 : limit)));
            lists.push_back(r);
        }
        for (const auto& chunks : lists) {
            const size_t n = chunks.size();
            // entries that go alone in between, as a pack meets them (every seventh; none in the first pass over the list)
            for (int holes = 0; holes < 2; ++holes) {
                std::vector<u8> batched(n, 1);
                if (holes) for (size_t i = 3; i < n; i += 7) batched[i] = 0;
                for (size_t i = 0; i < n; ) {
                    if (!batched[i]) { ++i; continue; }
                    // the pack's round, as it was
                    size_t j = i; u32 nCh = 0;
                    while (j < n && batched[j] && !(nCh && nCh + chunks[j] > limit)) { nCh += chunks[j]; ++j; }
                    // compress_entries' pass over the same run, as it was
                    size_t end = i; while (end < n && batched[end]) ++end;
                    size_t m1 = i; u32 mCh = 0;
                    while (m1 < end) { const u32 k = chunks[m1]; if (mCh && mCh + k > limit) break; mCh += k; ++m1; }
                    // both as they are
                    const size_t runEnd = batch_run_end(batched.data(), i, n < i + limit ? n : i + (size_t)limit);
                    u32 got = 0;
                    const size_t cut = batch_pass_cut(i, runEnd, limit, [&](size_t k) { return chunks[k]; }, got);
                    CHECK(runEnd == (end < i + limit ? end : i + (size_t)limit), "limit %u: the run of entry %zu ends at %zu, not %zu", limit, i, runEnd, end);
                    CHECK(cut == j && got == nCh, "limit %u: the cut at entry %zu is %zu (%u chunks), the pack's round %zu (%u)", limit, i, cut, got, j, nCh);
                    CHECK(cut == m1 && got == mCh, "limit %u: the cut at entry %zu is %zu (%u chunks), the pass %zu (%u)", limit, i, cut, got, m1, mCh);
                    // in the issue's words: whole entries, at least one, up to the limit unless the pass is one entry, and as many as fit
                    CHECK(cut > i && (got <= limit || cut == i + 1), "limit %u: a pass of %zu entries and %u chunks", limit, cut - i, got);
                    CHECK(cut == end || got + chunks[cut] > limit, "limit %u: entry %zu would have fitted", limit, cut);
                    i = cut; ++runs;
                }
            }
        }
    }
    printf("cut: %u passes bad=%d\n", runs, bad);
}

// group: same_group over BatchGroupKey views against the condition compress_entries held inline, restated with its own copy of what
// same_launch_params compared, for every pair of a small cross product of the fields, with and without per-entry CDicts
struct KeyFields { u32 prefixLen, chunkBytes, frameBlocks; bool dictIndex; Resolved rs; u32 slot; };
static bool old_same_group(const KeyFields& x, const KeyFields& y, bool cdicts)
{
    const bool xPlain = !x.prefixLen && !x.dictIndex, plain = !y.prefixLen && !y.dictIndex;
    const bool launch = x.rs.finder == y.rs.finder && x.rs.minStrideLog == y.rs.minStrideLog && x.rs.rawLiterals == y.rs.rawLiterals && x.rs.cp.strategy == y.rs.cp.strategy &&
                        x.rs.cp.searchLog == y.rs.cp.searchLog;
    return (cdicts ? (xPlain == plain && (!plain || x.slot == y.slot)) : x.prefixLen == y.prefixLen) && x.chunkBytes == y.chunkBytes && x.frameBlocks == y.frameBlocks && x.dictIndex == y.dictIndex &&
           (cdicts ? launch : !memcmp(&x.rs, &y.rs, sizeof(Resolved)));
}
static void part_group()
{
    std::vector<Resolved> rss;
    const Resolved base = { { 17, 16, 17, 1, 5, 0, 2 }, 1, 0, 0 };
    rss.push_back(base);
    for (int f = 0; f < 10; ++f) {      // one field apart from the base, each field once
        Resolved r = base;
        u32* const fields[10] = { &r.cp.windowLog, &r.cp.chainLog, &r.cp.hashLog, &r.cp.searchLog, &r.cp.minMatch, &r.cp.targetLength, &r.cp.strategy, &r.finder, &r.minStrideLog, &r.rawLiterals };
        *fields[f] += 1;
        rss.push_back(r);
    }
    std::vector<KeyFields> keys;
    const u32 prefixes[] = { 0, 4096, 8192 }, chunkSizes[] = { 32u << 10, 64u << 10 }, frames[] = { 0, 5 };
    for (u32 p : prefixes) for (u32 cb : chunkSizes) for (u32 fb : frames) for (int dix = 0; dix < 2; ++dix) for (u32 slot = 0; slot < 2; ++slot) for (const Resolved& r : rss)
        keys.push_back(KeyFields{ p, cb, fb, dix != 0, r, slot });
    u64 pairs = 0, same[2] = { 0, 0 };
    for (const KeyFields& x : keys) for (const KeyFields& y : keys) for (int cdicts = 0; cdicts < 2; ++cdicts) {
        const BatchGroupKey a = { x.prefixLen, x.chunkBytes, x.frameBlocks, x.dictIndex, x.rs, x.slot }, b = { y.prefixLen, y.chunkBytes, y.frameBlocks, y.dictIndex, y.rs, y.slot };
        const bool got = same_group(a, b, cdicts != 0), want = old_same_group(x, y, cdicts != 0);
        CHECK(got == want, "keys %zu and %zu, cdicts %d: %d, the old condition %d", (size_t)(&x - keys.data()), (size_t)(&y - keys.data()), cdicts, (int)got, (int)want);
        CHECK(got == same_group(b, a, cdicts != 0), "keys %zu and %zu, cdicts %d: not symmetric", (size_t)(&x - keys.data()), (size_t)(&y - keys.data()), cdicts);
        same[cdicts] += got; ++pairs;
    }
    // (both meanings were seen on both sides: without per-entry CDicts a pair shares a group iff it differs in nothing but the slot; with them more pairs do)
    CHECK(same[0] == keys.size() * 2 && same[1] > same[0], "%llu / %llu pairs share a group", (unsigned long long)same[0], (unsigned long long)same[1]);
    printf("group: %zu keys %llu pairs bad=%d\n", keys.size(), (unsigned long long)pairs, bad);
}

int main(int argc, char** argv)
{
    const char* part = argc > 1 ? argv[1] : "";
    if (!strcmp(part, "plan")) part_plan();
    else if (!strcmp(part, "limit")) part_limit();
    else if (!strcmp(part, "owner")) part_owner();
    else if (!strcmp(part, "fill")) part_fill();
    else if (!strcmp(part, "layout")) part_layout();
    else if (!strcmp(part, "cut")) part_cut();
    else if (!strcmp(part, "group")) part_group();
    else { printf("usage: batch_plan_harness plan | limit | owner | fill | layout | cut | group\n"); return 2; }
    return bad ? 1 : 0;
}
