// cut_rank_harness.cpp — zmi_cut_rank.h on the CPU (tests/test_cuts_async_cpu.py builds it under AddressSanitizer / UBSan): the
// successor rule, the doubling rounds and the scan that content_cuts_async.hip runs with a lane per node, here with plain loops,
// against piece ends exported from the numpy restatement of the rule.
//   cut_rank_harness rank FILE   -> FILE: cases of "n avgLog nCand nEnds", the candidate ends, the expected piece ends;
//                                   "rank: K cases bad=B maxSteps=S" (S: the most entries read and zones left for one node's successor)
//   cut_rank_harness rounds P    -> cut_rank_rounds(P)
// Every array is allocated at exactly the size the kernels' workspaces have per list (m + 2 nodes, cut_max_pieces ends), so that an index
// beyond either is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zmi_cut_rank.h"

using namespace zmi;

static bool rank(const std::vector<uint32_t>& cand, uint64_t n, unsigned avgLog, std::vector<uint32_t>& ends, uint32_t* maxSteps)
{
    const CutRule r = cut_rule(avgLog);
    const uint32_t m = (uint32_t)cand.size(), nodes = m + 2;
    const uint64_t P = cut_max_pieces(n, r);
    std::vector<uint32_t> succ(nodes), a(nodes), b(nodes), forced(nodes);
    std::vector<uint8_t> mark(nodes);
    for (uint32_t j = 0; j < nodes; ++j) {
        uint32_t steps = 0;
        cut_rank_init(cand.data(), m, n, r, j, succ.data(), forced.data(), mark.data(), steps);
        if (steps > *maxSteps) *maxSteps = steps;
        if (succ[j] <= j && j != m + 1) return false;   // (every pointer but the end's goes forward)
    }
    // the successors stay as they are (the ends are written from them): round 0 reads them, every later round the round before it
    const uint32_t* in = succ.data(); uint32_t* out = a.data();
    for (uint32_t k = 0; k < cut_rank_rounds(P); ++k) {
        // (descending: a lane order in which no mark set in a round is seen by it, the slowest the kernels' rounds can be)
        for (uint32_t j = nodes; j-- > 0;) cut_rank_round(j, in, out, mark.data());
        in = out; out = out == a.data() ? b.data() : a.data();
    }
    // the exclusive scan of the weights in list order, and every node's ends at its index
    std::vector<uint32_t> out1((size_t)P);
    uint64_t at = 0;
    for (uint32_t j = 0; j < nodes; ++j) {
        const uint64_t pos = cut_node_pos(cand.data(), m, n, j);
        const uint32_t w = cut_rank_weight(mark[j] != 0, pos, n, forced[j]);
        if (!w) continue;
        const uint64_t end = cut_node_pos(cand.data(), m, n, succ[j]);
        for (uint32_t k = 0; k < w; ++k) { if (at + k >= P) return false; out1[(size_t)(at + k)] = cut_rank_end(pos, k, forced[j], end, r); }
        at += w;
    }
    ends.assign(out1.begin(), out1.begin() + (size_t)at);
    return true;
}

int main(int argc, char** argv)
{
    if (argc >= 3 && !strcmp(argv[1], "rounds")) { printf("%u\n", cut_rank_rounds(strtoull(argv[2], nullptr, 10))); return 0; }
    if (argc >= 3 && !strcmp(argv[1], "rank")) {
        FILE* f = fopen(argv[2], "r");
        if (!f) return 2;
        unsigned long long n, nCand, nEnds; unsigned avgLog;
        int cases = 0, bad = 0;
        uint32_t maxSteps = 0;
        while (fscanf(f, "%llu %u %llu %llu", &n, &avgLog, &nCand, &nEnds) == 4) {
            std::vector<uint32_t> cand(nCand), want(nEnds), got;
            for (auto& v : cand) { unsigned long long x; if (fscanf(f, "%llu", &x) != 1) return 2; v = (uint32_t)x; }
            for (auto& v : want) { unsigned long long x; if (fscanf(f, "%llu", &x) != 1) return 2; v = (uint32_t)x; }
            const bool ok = n <= kCutMaxSrc && rank(cand, n, avgLog, got, &maxSteps) && got == want;
            if (!ok) { ++bad; printf("case %d: n=%llu avgLog=%u got %zu ends, want %zu\n", cases, n, avgLog, got.size(), want.size()); }
            ++cases;
        }
        fclose(f);
        printf("rank: %d cases bad=%d maxSteps=%u\n", cases, bad, maxSteps);
        return bad ? 1 : 0;
    }
    return 2;
}
