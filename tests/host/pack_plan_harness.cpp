// pack_plan_harness.cpp — the pack arithmetic of zmi_batch_plan.h on the CPU, under AddressSanitizer and UBSan
// (tests/test_pack_plan_host.py builds and runs it).  For lists of entries and made-up per-chunk frame sizes, the pack — verdicts, the
// one answer, every chunk slot's address, the table's rows, the entry ends — is evaluated per entry and per chunk slot as the kernels of
// frame.hip evaluate it (pack_place_async_kernel, pack_place_chunks_kernel; serial sums in the place of the scans) and held against a
// plain host loop: walk the entries in order, stop at the first that fails, else lay frame behind frame and count the rows.
//   lists:    seeded lists (empties, oversize and NULL-source entries) under five framings, with and without a chunk limit that cuts
//             in the middle: failing entries in front of and behind the cut.
//   counts:   n = 1, 16, 17, 1024, 1025, 16384.
//   capacity: exactly fits / one byte short / the frames fit but the table does not / 0.
// usage: pack_plan_harness lists | counts | capacity
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "zmi_batch_plan.h"

using namespace zmi;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Entry { u64 src, size; };
struct Geometry { u32 chunkBytes, frameBlocks; const char* name; };
struct Pack {
    u64 answer = 0;                                 // the stream's length, or the error as a size_t holds it
    std::vector<u64> offsets;                       // per chunk slot of the grid
    std::vector<u32> rows;                          // two words a row
    std::vector<u64> ends;                          // per entry
    std::vector<u64> emptyAt;                       // where the empty frames are written (offsets from the destination)
    u64 tableAt = 0;
};

static const u32 kEmptyLen = 9;
static const u64 kDst = 0x7f0000001025ull;          // the destination: a device address at no alignment

static u64 rnd_state = 88172645463325252ull;
static u64 rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }
// the frame bytes chunk c compressed to (what ChunkMeta::outSize would hold): anything reproducible
static u32 out_size(u32 c) { return 12 + (u32)((c * 2654435761u) >> 19); }

// ---- the reference: a plain loop over the entries ----
static Pack host_loop(const std::vector<Entry>& in, u64 bound, const Geometry& g, u32 maxChunks, u64 cap, u32 nLaunch)
{
    Pack p;
    const u32 fb = g.frameBlocks ? g.frameBlocks : 1u;
    // the lowest failing entry, by the plan's rules (the chunk limit counts good entries only)
    u64 counted = 0;
    for (const Entry& x : in) {
        if (x.size > bound || (x.size && !x.src)) { p.answer = (u64)0 - kErrSrcSizeWrong; break; }
        if (!x.size) continue;
        counted += (x.size + g.chunkBytes - 1) / g.chunkBytes;
        if (counted > maxChunks) { p.answer = (u64)0 - kErrWorkSpaceTooSmall; break; }
    }
    p.offsets.assign(nLaunch, kAsyncSpan);
    if (p.answer) return p;
    u64 at = 0; u32 ck = 0;
    std::vector<u64> off; std::vector<u32> len;
    for (const Entry& x : in) {
        if (!x.size) { p.emptyAt.push_back(at); p.rows.push_back(kEmptyLen); p.rows.push_back(0); at += kEmptyLen; p.ends.push_back(at); continue; }
        const u32 cnt = (u32)((x.size + g.chunkBytes - 1) / g.chunkBytes);
        for (u32 k = 0; k < cnt; ++k, ++ck) {
            const u64 o = (u64)k * g.chunkBytes;
            const u32 l = (u32)(x.size - o < g.chunkBytes ? x.size - o : g.chunkBytes);
            if (k % fb == 0) { p.rows.push_back(0); p.rows.push_back(0); }
            p.rows[p.rows.size() - 2] += out_size(ck); p.rows[p.rows.size() - 1] += l;
            off.push_back(kDst - kAsyncBase + at);
            at += out_size(ck);
        }
        p.ends.push_back(at);
    }
    const u64 all = at + 17 + 8 * (u64)(p.rows.size() / 2);
    if (all > cap) { p = Pack(); p.answer = (u64)0 - kErrDstSizeTooSmall; p.offsets.assign(nLaunch, kAsyncSpan); return p; }
    for (u32 c = 0; c < ck; ++c) p.offsets[c] = off[c];
    p.answer = all; p.tableAt = at;
    return p;
}

// ---- the pack as the kernels evaluate it ----
static Pack device_pack(const std::vector<Entry>& in, u64 bound, const Geometry& g, u32 maxChunks, u64 cap, u32 nLaunch)
{
    const u32 n = (u32)in.size();
    Pack p;
    // plan (batch_plan_entries_kernel<true>): verdicts, chunk counts, the cut, entFirst
    std::vector<u32> cnt(n), raw(n), verdict(n), first(n + 1);
    u32 cut = kPlanNoCut; u64 run = 0;
    for (u32 e = 0; e < n; ++e) {
        raw[e] = pack_verdict(in[e].src, in[e].size, bound);
        cnt[e] = plan_chunks(raw[e], in[e].size, g.chunkBytes);
        if (plan_is_cut(run, cnt[e], maxChunks)) cut = (u32)run;
        run += cnt[e];
    }
    run = 0;
    for (u32 e = 0; e < n; ++e) { first[e] = plan_first((u32)run, cut); verdict[e] = plan_limited(raw[e], run, cnt[e], maxChunks); run += cnt[e]; }
    first[n] = plan_first((u32)run, cut);
    CHECK(first[n] <= nLaunch, "total %u above the grid %u", first[n], nLaunch);
    // chunk lengths (batch_plan_chunks_kernel)
    std::vector<u32> len(nLaunch, 1);
    for (u32 c = 0; c < first[n] && c < nLaunch; ++c) { const u32 e = plan_owner(first.data(), n, c); len[c] = plan_chunk(in[e].src, in[e].size, c - first[e], g.chunkBytes, g.frameBlocks).len; }
    // place, entries (pack_place_async_kernel): per entry bytes and rows, the scans, the lowest failing entry, the one decision
    std::vector<u64> bytes(n), entAt(n); std::vector<u32> nRows(n), entRow(n);
    u64 total = 0; u32 rowsAll = 0, fail = kPackNoFail;
    for (u32 e = 0; e < n; ++e) {
        u64 sum = 0;
        for (u32 c = first[e]; c < first[e + 1]; ++c) sum += out_size(c);
        bytes[e] = pack_bytes(verdict[e], sum, kEmptyLen);
        nRows[e] = pack_frames(verdict[e], first[e + 1] - first[e], g.frameBlocks);
        if (pack_fails(verdict[e]) && fail == kPackNoFail) fail = e;
        entAt[e] = total; entRow[e] = rowsAll;
        total += bytes[e]; rowsAll += nRows[e];
    }
    p.answer = pack_answer(fail == kPackNoFail ? kPackNoFail : verdict[fail], total, rowsAll, cap);
    const bool ok = pack_answer_ok(p.answer);
    p.offsets.assign(nLaunch, 0);
    if (ok) {
        p.tableAt = total;
        p.rows.assign(2 * (size_t)rowsAll, 0xDEADBEEFu);
        for (u32 e = 0; e < n; ++e) {
            if (verdict[e] == kAsyncEmpty) { p.emptyAt.push_back(entAt[e]); p.rows[2 * (size_t)entRow[e]] = kEmptyLen; p.rows[2 * (size_t)entRow[e] + 1] = 0; }
            p.ends.push_back(entAt[e] + bytes[e]);
        }
    }
    // place, chunks (pack_place_chunks_kernel): one slot at a time
    for (u32 c = 0; c < nLaunch; ++c) {
        u64 off = kAsyncSpan;
        if (ok && c < first[n]) {
            const u32 e = plan_owner(first.data(), n, c), c0 = first[e], k = c - c0;
            u64 inner = 0;
            for (u32 j = c0; j < c; ++j) inner += out_size(j);
            off = pack_chunk_at(true, kDst, entAt[e], inner);
            if (pack_row_lead(k, g.frameBlocks)) {
                const u32 fb = g.frameBlocks ? g.frameBlocks : 1u, row = pack_row(entRow[e], k, g.frameBlocks);
                u32 cs = 0, ds = 0;
                for (u32 j = c; j < c + fb && j < first[e + 1]; ++j) { cs += out_size(j); ds += len[j]; }
                CHECK(row < rowsAll && p.rows[2 * (size_t)row] == 0xDEADBEEFu, "row %u of %u written twice or out of range", row, rowsAll);
                if (row < rowsAll) { p.rows[2 * (size_t)row] = cs; p.rows[2 * (size_t)row + 1] = ds; }
            }
        }
        p.offsets[c] = off;
    }
    return p;
}

static u32 grid_of(size_t n, u64 bound, const Geometry& g, u32 maxChunks)
{
    const u64 most = (u64)n * ((bound + g.chunkBytes - 1) / g.chunkBytes);
    return (u32)(most < maxChunks ? most : maxChunks);
}

static u64 compare(const std::vector<Entry>& in, u64 bound, const Geometry& g, u32 maxChunks, u64 cap, const char* what)
{
    const u32 nLaunch = grid_of(in.size(), bound, g, maxChunks);
    const Pack want = host_loop(in, bound, g, maxChunks, cap, nLaunch), got = device_pack(in, bound, g, maxChunks, cap, nLaunch);
    CHECK(got.answer == want.answer, "%s %s n=%zu: answer %llx, expected %llx", g.name, what, in.size(), (unsigned long long)got.answer, (unsigned long long)want.answer);
    CHECK(got.offsets == want.offsets, "%s %s n=%zu: chunk offsets differ", g.name, what, in.size());
    CHECK(got.rows == want.rows, "%s %s n=%zu: rows differ (%zu / %zu words)", g.name, what, in.size(), got.rows.size(), want.rows.size());
    CHECK(got.ends == want.ends && got.emptyAt == want.emptyAt && got.tableAt == want.tableAt, "%s %s n=%zu: ends, empty frames or the table's place differ", g.name, what, in.size());
    if (pack_answer_ok(want.answer)) {
        CHECK(want.answer <= cap, "%s %s: %llu bytes in %llu", g.name, what, (unsigned long long)want.answer, (unsigned long long)cap);
        for (u64 o : got.offsets) if (o != kAsyncSpan) CHECK(o + kAsyncBase >= kDst && o + kAsyncBase < kDst + cap, "%s %s: a chunk outside the destination", g.name, what);
    } else
        for (u64 o : got.offsets) CHECK(o == kAsyncSpan, "%s %s: a failed pack places a chunk", g.name, what);
    return want.answer;
}

static const Geometry kGeometries[] = { { 16u << 10, 4, "16Kx4" }, { 48u << 10, 5, "48Kx5" }, { 32u << 10, 8, "32Kx8" }, { 32u << 10, 0, "32Kx0" }, { 64u << 10, 0, "64Kx0" } };
static const u64 kRoom = (u64)1 << 40;

// n seeded entries of 0 .. bound bytes (every seventh empty); the caller breaks some of them
static std::vector<Entry> seeded(u32 n, u64 bound, const Geometry& g)
{
    std::vector<Entry> r;
    u64 at = 0x10000000ull;
    for (u32 i = 0; i < n; ++i) {
        const u64 pick = rnd() % 10;
        u64 S = pick < 6 ? 1 + rnd() % (3 * (u64)g.chunkBytes) : pick < 9 ? 1 + rnd() % bound : bound;
        if (S > bound) S = bound;
        if (i % 7 == 3) S = 0;
        r.push_back(Entry{ S || (i & 1) ? at : 0, S });        // (an empty entry's source may be NULL)
        at += S + 5;
    }
    return r;
}
static u32 chunks_in(const std::vector<Entry>& in, size_t upTo, const Geometry& g)
{
    u64 s = 0;
    for (size_t e = 0; e < upTo && e < in.size(); ++e) s += (in[e].size + g.chunkBytes - 1) / g.chunkBytes;
    return (u32)s;
}

static void part_lists()
{
    u32 runs = 0, failed = 0;
    for (const Geometry& g : kGeometries) {
        const u64 bound = 5 * (u64)g.chunkBytes + 77;
        for (int list = 0; list < 6; ++list) {
            const std::vector<Entry> good = seeded(40 + (u32)(rnd() % 200), bound, g);
            const size_t n = good.size(), mid = n / 2;
            const u32 cutAt = chunks_in(good, mid + 1, g) - 1;          // entry `mid` (or the good one in front of it) is the first refused
            CHECK(pack_answer_ok(compare(good, bound, g, 0xFFFFFFFFu, kRoom, "good")), "%s: a good list failed", g.name);
            const u64 cutAnswer = compare(good, bound, g, cutAt, kRoom, "cut");
            CHECK(cutAnswer == (u64)0 - kErrWorkSpaceTooSmall, "%s: a cut list answered %llx", g.name, (unsigned long long)cutAnswer);
            runs += 2;
            for (int where = 0; where < 2; ++where) {                   // a failing entry in front of the cut, then behind it
                for (int kind = 0; kind < 2; ++kind) {
                    std::vector<Entry> in = good;
                    size_t at = where ? mid + 3 + rnd() % (n - mid - 3) : rnd() % (mid / 2);
                    while (!in[at].size) at = where ? at - 1 : at + 1;   // (an empty entry with a NULL source is fine)
                    if (kind) in[at].size = bound + 1 + rnd() % 100; else in[at].src = 0;
                    const u64 free = compare(in, bound, g, 0xFFFFFFFFu, kRoom, "one bad"), lim = compare(in, bound, g, cutAt, kRoom, "one bad, cut");
                    CHECK(free == (u64)0 - kErrSrcSizeWrong, "%s: a bad entry answered %llx", g.name, (unsigned long long)free);
                    // behind the cut the refused entry comes first; in front of it the bad one (whose chunks no longer count)
                    CHECK(lim == (where ? (u64)0 - kErrWorkSpaceTooSmall : (u64)0 - kErrSrcSizeWrong), "%s: bad at %zu, cut at entry %zu: %llx", g.name, at, mid, (unsigned long long)lim);
                    runs += 2; failed += 2;
                }
            }
        }
    }
    printf("lists: %u runs %u failing bad=%d\n", runs, failed, bad);
}

static void part_counts()
{
    const u32 counts[] = { 1, 16, 17, 1024, 1025, 16384 };
    u32 runs = 0;
    for (const Geometry& g : kGeometries)
        for (u32 n : counts) {
            const u64 bound = n > 2000 ? g.chunkBytes : 2 * (u64)g.chunkBytes + 5;      // (16384 entries: one chunk each, the pass limit)
            const std::vector<Entry> in = seeded(n, bound, g);
            CHECK(pack_answer_ok(compare(in, bound, g, 16384, kRoom, "count")), "%s n=%u failed", g.name, n);
            std::vector<Entry> allEmpty(n, Entry{ 0, 0 });
            CHECK(compare(allEmpty, bound, g, 16384, kRoom, "all empty") == (u64)n * kEmptyLen + 17 + 8 * (u64)n, "%s: %u empty entries", g.name, n);
            runs += 2;
        }
    const std::vector<Entry> none;
    CHECK(compare(none, 4096, kGeometries[4], 16, 17, "n=0") == 17, "the empty table");
    CHECK(compare(none, 4096, kGeometries[4], 16, 16, "n=0, 16 bytes") == (u64)0 - kErrDstSizeTooSmall, "the empty table in 16 bytes");
    printf("counts: %u runs bad=%d\n", runs + 2, bad);
}

static void part_capacity()
{
    u32 runs = 0;
    for (const Geometry& g : kGeometries)
        for (int list = 0; list < 4; ++list) {
            const u64 bound = 4 * (u64)g.chunkBytes;
            const std::vector<Entry> in = seeded(1 + (u32)(rnd() % 120), bound, g);
            const u64 size = compare(in, bound, g, 0xFFFFFFFFu, kRoom, "room");
            CHECK(pack_answer_ok(size), "%s: a good list failed", g.name);
            const Pack p = host_loop(in, bound, g, 0xFFFFFFFFu, kRoom, grid_of(in.size(), bound, g, 0xFFFFFFFFu));
            const u64 tooSmall = (u64)0 - kErrDstSizeTooSmall;
            CHECK(compare(in, bound, g, 0xFFFFFFFFu, size, "exact") == size, "%s: exactly fits", g.name);
            CHECK(compare(in, bound, g, 0xFFFFFFFFu, size - 1, "one short") == tooSmall, "%s: one byte short", g.name);
            CHECK(compare(in, bound, g, 0xFFFFFFFFu, p.tableAt, "frames only") == tooSmall, "%s: the frames fit, the table does not", g.name);
            CHECK(compare(in, bound, g, 0xFFFFFFFFu, p.tableAt + 16, "frames + 16") == tooSmall, "%s: the frames and 16 bytes", g.name);
            CHECK(compare(in, bound, g, 0xFFFFFFFFu, 0, "nothing") == tooSmall, "%s: capacity 0", g.name);
            runs += 6;
        }
    printf("capacity: %u runs bad=%d\n", runs, bad);
}

int main(int argc, char** argv)
{
    const char* part = argc > 1 ? argv[1] : "";
    if (!strcmp(part, "lists")) part_lists();
    else if (!strcmp(part, "counts")) part_counts();
    else if (!strcmp(part, "capacity")) part_capacity();
    else { printf("usage: pack_plan_harness lists | counts | capacity\n"); return 2; }
    return bad ? 1 : 0;
}
