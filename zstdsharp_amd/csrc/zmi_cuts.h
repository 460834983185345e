// zmi_cuts.h — content-defined frame cuts (ZSTDMI_CCtx_setContentCuts; include/zstd_mi355x.h "Content-defined cuts"):
// the rule, version 1, stated once.  The gear table, the candidate test, the selection walk and the bound are here; content_cuts.hip's
// select kernel runs cut_walk with a wave behind its two callbacks, tests/host/cuts_harness.cpp runs the same text with plain loops
// under AddressSanitizer / UBSan.  Plain C++ without a HIP header.
//
// The rule.  gear[i] = splitmix64(i).  After byte p of the call's source h(p) = sum over k = 0 .. min(p, 63) of gear[src[p - k]] << k
// (mod 2^64): h = (h << 1) + gear[byte] from 0 at the first byte; it depends on the last 64 bytes only and never on earlier cuts.
// With bits = avgLog - 1, min = 1 << (avgLog - 2) and max = 65536, position p + 1 is a CANDIDATE end iff the top `bits` bits of h(p)
// are zero.  From a piece start s (first 0) the piece ends at the smallest candidate e with e - s >= min if e - s <= max, else at
// s + max; the source's end ends the last piece whatever its length; an empty source has no piece.  avgLog is 12 .. 16.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZMI_CUTS_HD __host__ __device__
#else
#define ZMI_CUTS_HD
#endif

namespace zmi {

constexpr unsigned kCutRuleVersion = 1;
constexpr unsigned kCutAvgLogMin = 12, kCutAvgLogMax = 16;
constexpr uint32_t kCutMax = 65536;             // the longest piece: one block of every framing
constexpr uint32_t kCutTile = 16384;            // bytes per workgroup of the mark kernel (256 lanes x 64 positions)
constexpr uint32_t kCutListBlock = 1024;        // candidates the select walk holds in LDS at a time (blocks begin at multiples of it)
constexpr uint64_t kCutMaxSrc = 0xFFFFFFFFull;  // ends are 32-bit words

ZMI_CUTS_HD inline uint64_t cut_gear(uint64_t i)     // splitmix64(i): ldm.hip's table
{
    uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct CutRule { uint32_t bits, min, max; };
ZMI_CUTS_HD inline bool cut_avglog_ok(unsigned avgLog) { return avgLog >= kCutAvgLogMin && avgLog <= kCutAvgLogMax; }
ZMI_CUTS_HD inline CutRule cut_rule(unsigned avgLog) { return CutRule{ avgLog - 1, 1u << (avgLog - 2), kCutMax }; }
ZMI_CUTS_HD inline bool cut_candidate(uint64_t h, uint32_t bits) { return (h >> (64 - bits)) == 0; }

// The selection.  next(target, c): the smallest candidate >= target into c, false when there is none; targets never decrease.
// run(first, step, count): `count` ends first, first + step, ... in order (the forced cuts of a stretch without a usable candidate are
// one call, however long the stretch).  -> the pieces.
// U: the type of a position, uint64_t or — for n <= kCutMaxSrc, where every end fits a word and the select kernel's scalar unit
// compares words — uint32_t.  The one sum that can pass n, s + min, saturates: a target at U's largest value can only find a candidate
// that is the source's end, which ends the piece either way.
template <class U> ZMI_CUTS_HD inline U cut_add_sat(U a, U b) { const U r = (U)(a + b); return r < a ? (U)~(U)0 : r; }
template <class U, class Next, class Run>
ZMI_CUTS_HD inline U cut_walk(U n, const CutRule& r, Next next, Run run)
{
    U s = 0, pieces = 0;
    while (s < n) {
        U c = 0;
        const bool have = next(cut_add_sat<U>(s, (U)r.min), c);
        const U far = have ? c : n;                     // (far > s: a candidate lies at or behind s + min, and s < n)
        if (far - s > r.max) {                          // (the common piece pays no division)
            const U forced = (U)((far - s - 1) / r.max);        // cuts at s + max, s + 2 max, ... in front of far
            run((U)(s + r.max), (U)r.max, forced);
            pieces += forced; s += forced * r.max;
            if (have && c - s < r.min) continue;        // the candidate lies too close behind the last forced cut: the next one
        }
        run(far, (U)0, (U)1);                           // now 1 <= far - s <= max: the candidate, or the source's end
        pieces += 1; s = far;
    }
    return pieces;
}

// the most pieces a source of srcSize bytes has: every piece but the last holds min bytes or more
ZMI_CUTS_HD inline uint64_t cut_max_pieces(uint64_t srcSize, const CutRule& r) { return srcSize / r.min + 1; }

// ZSTDMI_contentCutsBound: srcSize + (srcSize >> 8) + 64 P + 17 + 8 (srcSize / 4096 + P), P = srcSize / min + 1 — at least
// ZSTDMI_packBound of any piece list the rule allows (ZSTD_compressBound(s) <= s + (s >> 8) + 64; at most P pieces).  false: overflow.
inline bool cut_bound(uint64_t srcSize, const CutRule& r, uint64_t* out)
{
    const uint64_t P = cut_max_pieces(srcSize, r);
    uint64_t b = srcSize, t;
    if (__builtin_add_overflow(b, srcSize >> 8, &b)) return false;
    if (__builtin_mul_overflow(P, (uint64_t)64, &t) || __builtin_add_overflow(b, t, &b)) return false;
    if (__builtin_add_overflow(srcSize / 4096, P, &t) || __builtin_mul_overflow(t, (uint64_t)8, &t) || __builtin_add_overflow(b, t, &b)) return false;
    if (__builtin_add_overflow(b, (uint64_t)17, &b)) return false;
    *out = b;
    return true;
}

} // namespace zmi
