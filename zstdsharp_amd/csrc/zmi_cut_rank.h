// zmi_cut_rank.h — the selection of content-defined cuts (the rule: zmi_cuts.h) without a serial walk (ZSTDMI_contentCutsAsync;
// DESIGN.md 5u): per candidate the candidate its piece would end at, the candidates the walk from position 0 reaches by pointer
// doubling, and every reached candidate's ends at the index an exclusive scan gives it.  The successor rule, the round count, one
// node's part of a round and one node's ends are stated here once; content_cuts_async.hip runs them with a lane per node,
// tests/host/cut_rank_harness.cpp with plain loops under AddressSanitizer / UBSan.  Plain C++ without a HIP header.
//
// Why a successor exists per START and not per walk state: from a start s, cut_walk's forced cuts all lie on the lattice s + k max —
// also across its `continue`, which moves s by whole multiples of max.  So the real end behind s is the smallest candidate c >= s + min
// with ((c - s - 1) mod max) + 1 >= min: c's distance from the last forced cut in front of it, (c - s - 1) mod max + 1, is min or more.
// In front of it lie f = (c - s - 1) / max forced ends s + max, ..., s + f max.  Without such a candidate the end is n, f = (n - s - 1) / max.
// The candidates that fail the test lie in the BAD ZONES (s + k max, s + k max + min - 1], k = 0, 1, ...; the search leaves a zone by
// one lower bound at the zone's end, however many candidates lie inside.
//
// Nodes: 0 = the start (position 0), 1 + i = candidate i (position cand[i]), m + 1 = the end of the source (no successor of its own:
// it points at itself).  A node at position n (a candidate that is the source's end) starts no piece: weight 0.
#pragma once
#include "zmi_cuts.h"

namespace zmi {

// rounds of pointer doubling that reach every node of a path of at most maxPieces nodes in front of the end: after k rounds the nodes at
// distance < 2^k from the start are marked, and every node of the path but the end starts at least one piece
ZMI_CUTS_HD inline uint32_t cut_rank_rounds(uint64_t maxPieces)
{
    uint32_t k = 0;
    while (((uint64_t)1 << k) < maxPieces + 1) ++k;
    return k;
}

// the first index i in [from, m) with cand[i] >= target, m when there is none: doubling steps from `from`, then halving inside the last
// step (what a piece usually needs lies a few entries behind `from`).  steps: one per entry read.
ZMI_CUTS_HD inline uint32_t cut_lower_bound(const uint32_t* cand, uint32_t from, uint32_t m, uint64_t target, uint32_t& steps)
{
    uint32_t lo = from, hi = m;                 // entries in front of lo are below target, entries at or behind hi are not (or there are none)
    for (uint32_t step = 1; lo < hi; step = step < (1u << 30) ? step << 1 : step) {
        const uint32_t at = (hi - lo) > step ? lo + step - 1 : hi - 1;
        ++steps;
        if (cand[at] >= target) { hi = at; break; }
        lo = at + 1;
    }
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        ++steps;
        if (cand[mid] >= target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

struct CutSucc { uint32_t next, forced; };      // next: the index in cand of the real end, m = the source's end; forced: f
// the successor of a start s < n; from: an index with every entry in front of it below s + min (0, or the start's own index + 1)
ZMI_CUTS_HD inline CutSucc cut_successor(const uint32_t* cand, uint32_t m, uint32_t from, uint64_t s, uint64_t n, const CutRule& r, uint32_t& steps)
{
    uint64_t target = s + r.min;
    uint32_t i = from;
    for (;;) {
        i = cut_lower_bound(cand, i, m, target, steps);
        if (i >= m) break;
        const uint64_t c = cand[i];
        if (c > n) { i = m; break; }            // (a list that passes the source: nothing behind n is an end)
        const uint64_t d = c - s - 1, k = d / r.max;
        if (d - k * r.max + 1 >= r.min) return CutSucc{ i, (uint32_t)k };
        target = s + k * r.max + r.min;         // c lies in bad zone k: on to the zone's end (c is below it: the search goes on behind c)
        ++i; ++steps;
    }
    return CutSucc{ m, (uint32_t)((n - s - 1) / r.max) };
}

// position of node j of a list of m candidates over a source of n bytes
ZMI_CUTS_HD inline uint64_t cut_node_pos(const uint32_t* cand, uint32_t m, uint64_t n, uint32_t j) { return j == 0 ? 0 : j <= m ? cand[j - 1] : n; }

// node j's successor and forced count -> jump[j], forced[j]; mark[j] = it is the start.  j = 0 .. m + 1.
ZMI_CUTS_HD inline void cut_rank_init(const uint32_t* cand, uint32_t m, uint64_t n, const CutRule& r, uint32_t j, uint32_t* jump, uint32_t* forced, uint8_t* mark,
                                      uint32_t& steps)
{
    const uint64_t s = cut_node_pos(cand, m, n, j);
    CutSucc x{ m, 0 };
    if (j <= m && s < n) x = cut_successor(cand, m, j, s, n, r, steps);     // (from = j: the entries in front of index j are at or below s)
    jump[j] = x.next + 1; forced[j] = x.forced; mark[j] = j == 0;
}

// node j's part of one doubling round: a marked node marks the node its pointer names, and every pointer doubles.  in and out are
// different arrays; marks are only ever set, so a mark set in this round may or may not be seen by it — either way it names a node of the path.
ZMI_CUTS_HD inline void cut_rank_round(uint32_t j, const uint32_t* in, uint32_t* out, uint8_t* mark)
{
    const uint32_t t = in[j];
    if (mark[j]) mark[t] = 1;
    out[j] = in[t];
}

// ends a node writes: its forced run and its real end, none for a node that is not on the path or lies at the source's end
ZMI_CUTS_HD inline uint32_t cut_rank_weight(bool marked, uint64_t pos, uint64_t n, uint32_t forced) { return marked && pos < n ? forced + 1 : 0u; }
// end k (0 .. forced) of a node at pos whose real end is `end`
ZMI_CUTS_HD inline uint32_t cut_rank_end(uint64_t pos, uint32_t k, uint32_t forced, uint64_t end, const CutRule& r) { return (uint32_t)(k < forced ? pos + (uint64_t)(k + 1) * r.max : end); }

} // namespace zmi
