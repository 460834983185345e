// cuts_harness.cpp — zmi_cuts.h on the CPU (tests/test_content_cuts_cpu.py builds it under AddressSanitizer / UBSan): the text the
// select kernel runs (cut_walk, cut_candidate, cut_gear, cut_bound) against tables exported from the numpy restatement of the rule.
//   cuts_harness gear            -> the 256 gear words, hex, one a line
//   cuts_harness bound N avgLog  -> the bound, or "overflow"
//   cuts_harness walk FILE       -> FILE: cases of "n avgLog nCand nEnds", the candidate ends, the expected piece ends; "walk: K cases bad=B"
//   cuts_harness mark FILE avgLog -> FILE: raw bytes; the candidate ends by the rolling form h = (h << 1) + gear[byte], one a line
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zmi_cuts.h"

using namespace zmi;

template <class U>
static std::vector<uint64_t> walk(const std::vector<uint64_t>& cand, uint64_t n, unsigned avgLog, uint64_t* pieces)
{
    std::vector<uint64_t> ends;
    size_t idx = 0;
    U lastTarget = 0;
    bool ordered = true;
    auto next = [&](U target, U& c) {
        if (target < lastTarget) ordered = false;
        lastTarget = target;
        while (idx < cand.size() && cand[idx] < target) ++idx;
        if (idx == cand.size()) return false;
        c = (U)cand[idx];
        return true;
    };
    auto run = [&](U first, U step, U count) { for (U j = 0; j < count; ++j) ends.push_back((uint64_t)(U)(first + j * step)); };
    *pieces = cut_walk<U>((U)n, cut_rule(avgLog), next, run);
    if (!ordered) ends.clear();
    return ends;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "gear")) {
        for (unsigned i = 0; i < 256; ++i) printf("%016llx\n", (unsigned long long)cut_gear(i));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "bound")) {
        uint64_t b = 0;
        const unsigned avgLog = (unsigned)strtoul(argv[3], nullptr, 10);
        if (!cut_avglog_ok(avgLog)) { printf("bad avgLog\n"); return 0; }
        if (cut_bound(strtoull(argv[2], nullptr, 10), cut_rule(avgLog), &b)) printf("%llu\n", (unsigned long long)b); else printf("overflow\n");
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "walk")) {
        FILE* f = fopen(argv[2], "r");
        if (!f) return 2;
        unsigned long long n, nCand, nEnds; unsigned avgLog;
        int cases = 0, bad = 0;
        while (fscanf(f, "%llu %u %llu %llu", &n, &avgLog, &nCand, &nEnds) == 4) {
            std::vector<uint64_t> cand(nCand), want(nEnds);
            for (auto& v : cand) { unsigned long long x; if (fscanf(f, "%llu", &x) != 1) return 2; v = x; }
            for (auto& v : want) { unsigned long long x; if (fscanf(f, "%llu", &x) != 1) return 2; v = x; }
            uint64_t pieces = 0;
            const std::vector<uint64_t> got = walk<uint64_t>(cand, n, avgLog, &pieces);
            bool ok = got == want && pieces == want.size() && pieces <= cut_max_pieces(n, cut_rule(avgLog));
            if (n <= kCutMaxSrc) {      // the select kernel's instance: positions in words
                uint64_t pieces32 = 0;
                ok = ok && walk<uint32_t>(cand, n, avgLog, &pieces32) == want && pieces32 == want.size();
            }
            if (!ok) { ++bad; printf("case %d: n=%llu avgLog=%u got %zu ends, want %zu\n", cases, n, avgLog, got.size(), want.size()); }
            ++cases;
        }
        fclose(f);
        printf("walk: %d cases bad=%d\n", cases, bad);
        return bad ? 1 : 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "mark")) {
        FILE* f = fopen(argv[2], "rb");
        if (!f) return 2;
        const unsigned avgLog = (unsigned)strtoul(argv[3], nullptr, 10);
        const CutRule r = cut_rule(avgLog);
        uint64_t gear[256];
        for (unsigned i = 0; i < 256; ++i) gear[i] = cut_gear(i);
        uint64_t h = 0, p = 0;
        for (int ch; (ch = fgetc(f)) != EOF; ++p) { h = (h << 1) + gear[ch & 255]; if (cut_candidate(h, r.bits)) printf("%llu\n", (unsigned long long)(p + 1)); }
        fclose(f);
        return 0;
    }
    return 2;
}
