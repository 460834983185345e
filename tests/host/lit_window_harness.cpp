// Host sweep of huf_decode_stream_fs (decode_lit.hip) aimed at its window logic: the steady form keeps looking up from the
// registers of the step before while the re-base runs, and shifts only the registers the lookups left still need, so what
// matters is runs of the longest codes (eight 11-bit codes a step), the shortest ones, and where a stream changes form: from
// the steady groups to the general ones, to single steps, to the plain bit reader.  fs.inc / bb.inc are lifted out of the
// sources by tests/test_lit_window_host.py; built with -fsanitize=address,undefined; 0xAA guard bytes around every stream.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
typedef uint8_t u8; typedef uint16_t u16; typedef uint32_t u32; typedef uint64_t u64; typedef int32_t s32;
typedef u64 __attribute__((aligned(1))) u64u; typedef u32 __attribute__((aligned(1))) u32u; typedef u16 __attribute__((aligned(1))) u16u;
static inline u32 highbit32(u32 v) { return 31u - (u32)__builtin_clz(v); }
static inline u64 readLE64(const u8* p) { u64 v; memcpy(&v, p, 8); return v; }
static inline u32 __builtin_amdgcn_alignbit(u32 hi, u32 lo, u32 s) { s &= 31; return (u32)((((u64)hi << 32) | lo) >> s); }
static inline int __builtin_amdgcn_mov_dpp(int v, int, int, int, bool) { return v; }     // quad-transposed stores: GPU only, never taken here
static u8 g_lds[1 << 16];                      // stands in for the LDS: tables are addressed by offset
#define ZMI_LDS_U16(off) (*(const u16*)(g_lds + (off)))
static u32 g_paths;                            // which forms the call went through: bit 0 steady group, 1 general group or step, 2 bit reader
#define ZMI_LIT_PATHS(k) (g_paths |= 1u << (k))
static inline u32 huf_entry(u32 sym, u32 nbBits) { return (32u - nbBits) | (sym << 8); }
#include "bb.inc"
#include "fs.inc"

// A code whose symbol k (k = 0 .. L - 1) has length k + 1 and whose symbol L has length L: lengths 1, 2, .., L, L (Kraft sum 1),
// tableLog L.  Symbol values are spread over the byte range so that a wrong byte lane shows.
struct Code { u32 tableLog; u32 nb[256], val[256]; std::vector<u16> full; u32 n1; std::vector<u8> bySlot; };
static Code make_code(u32 L)
{
    Code c; memset(c.nb, 0, sizeof c.nb); memset(c.val, 0, sizeof c.val); c.tableLog = L; c.n1 = 0;
    u32 w[256] = {0};
    for (u32 k = 0; k <= L; k++) { const u32 sym = (k * 37u + 11u) & 255u, len = k < L ? k + 1 : L; c.nb[sym] = len; w[sym] = L + 1 - len; c.bySlot.push_back((u8)sym); }
    c.full.assign(1u << L, 0);
    u32 idx = 0;
    for (u32 ww = 1; ww <= L; ww++) for (u32 s = 0; s < 256; s++) if (w[s] == ww) {
        const u32 len = 1u << (ww - 1); c.val[s] = idx >> (ww - 1);
        for (u32 u = 0; u < len; u++) c.full[idx + u] = (u16)s;
        idx += len; if (ww == 1) c.n1++;
    }
    if (idx != (1u << L)) { printf("bad code\n"); exit(1); }
    return c;
}
static u8 sym_of_len(const Code& c, u32 len, u32 which) { return c.bySlot[len == c.tableLog && which ? c.tableLog : len - 1]; }

static long g_cases, g_bad, g_steady, g_general, g_reader;
static void run(const Code& c, const std::vector<u8>& syms, const char* what)
{
    const u32 n = (u32)syms.size();
    std::vector<u8> out((size_t)n * 2 + 16, 0); u64 bitpos = 0;
    auto put = [&](u32 v, u32 nb) { for (u32 b = 0; b < nb; b++) { if ((v >> b) & 1) out[bitpos >> 3] |= (u8)(1 << (bitpos & 7)); bitpos++; } };
    for (int i = (int)n - 1; i >= 0; i--) put(c.val[syms[i]], c.nb[syms[i]]);
    put(1, 1);
    const u32 sz = (u32)((bitpos + 7) >> 3);
    for (int form = 0; form < 2; form++) {
        const u32 IDX = form == 0 ? 11 : 10;
        if (c.tableLog > IDX + (form == 1 ? 1 : 0)) continue;
        std::vector<u16> tab(1u << IDX, 0); bool pairs = false;
        const u32 tOff = 8192;
        if (c.tableLog <= IDX) { const u32 up = IDX - c.tableLog; for (u32 i = 0; i < (1u << c.tableLog); i++) for (u32 u = 0; u < (1u << up); u++) tab[(i << up) + u] = (u16)huf_entry(c.full[i], c.nb[c.full[i]]); }
        else { pairs = true; for (u32 i = 0; i < (1u << c.tableLog); i += 2) tab[i >> 1] = i < c.n1 ? (u16)(c.full[i] | (c.full[i + 1] << 8)) : (u16)huf_entry(c.full[i], c.nb[c.full[i]]); }
        memcpy(g_lds + tOff, tab.data(), tab.size() * 2);
        std::vector<u8> buf(32 + sz + 32, 0xAA); memcpy(buf.data() + 32, out.data(), sz);
        std::vector<u8> dec(n + 64, 0);
        g_paths = 0;
        bool ok;
        if (form == 0) ok = huf_decode_stream_fs<11, false>(tOff, 0u, buf.data() + 32, sz, dec.data(), n);
        else ok = pairs ? huf_decode_stream_fs<10, true>(tOff, c.n1, buf.data() + 32, sz, dec.data(), n)
                        : huf_decode_stream_fs<10, false>(tOff, 0u, buf.data() + 32, sz, dec.data(), n);
        g_cases++; g_steady += g_paths & 1; g_general += (g_paths >> 1) & 1; g_reader += (g_paths >> 2) & 1;
        bool tail = true; for (u32 k = n; k < n + 64; k++) tail &= dec[k] == 0;
        if (!ok || !tail || memcmp(dec.data(), syms.data(), n)) {
            u32 k = 0; while (k < n && dec[k] == syms[k]) k++;
            printf("%s: form %d tableLog %u n %u sz %u ok %d tail %d firstbad %u\n", what, form, c.tableLog, n, sz, ok, tail, k);
            if (++g_bad > 20) { printf("done bad=%ld\n", g_bad); exit(1); }
        }
    }
}

int main()
{
    srand(11);
    std::vector<u32> counts;
    for (u32 n = 1; n <= 200; n++) counts.push_back(n);
    for (u32 k = 8; k <= 1100; k += 8) for (int d = -1; d <= 1; d++) if (k + d > 200 && k + d <= 1100) counts.push_back(k + d);
    counts.push_back(1100);
    const Code c10 = make_code(10), c11 = make_code(11);
    const Code* codes[2] = { &c10, &c11 };
    for (const Code* c : codes) {
        const u32 L = c->tableLog;
        for (u32 n : counts) {
            std::vector<u8> s(n);
            const u32 one[4] = { 1, 2, 10, 11 };
            for (u32 len : one) if (len <= L) {                                         // one length only
                for (u32 i = 0; i < n; i++) s[i] = sym_of_len(*c, len, i & 1); run(*c, s, "one length");
            }
            for (u32 i = 0; i < n; i++) s[i] = sym_of_len(*c, (i & 1) ? L : 1, (i >> 1) & 1); run(*c, s, "alternating 1 / max");
            for (u32 i = 0; i < n; i++) s[i] = sym_of_len(*c, (i & 7) == 7 ? 1 : L, i & 1); run(*c, s, "seven max, one 1");
            for (u32 i = 0; i < n; i++) s[i] = sym_of_len(*c, (i & 7) == 0 ? 1 : L, i & 1); run(*c, s, "one 1, seven max");
            for (u32 i = 0; i < n; i++) { const u32 len = 1 + rand() % L; s[i] = sym_of_len(*c, len, rand() & 1); } run(*c, s, "random lengths");
            for (u32 i = 0; i < n; i++) { const u32 len = (rand() & 3) ? L : L - 1; s[i] = sym_of_len(*c, len, rand() & 1); } run(*c, s, "long codes");
        }
        // stream sizes 15 .. 64 bytes: where srcSize >= 16 switches the reader, and steps that read below the stream's start
        for (u32 sz = 15; sz <= 64; sz++) for (u32 j = 0; j < 8; j++) {
            const u32 bits = 8 * sz - 1 - j;                                             // payload bits of a stream of sz bytes
            std::vector<u8> s(bits, sym_of_len(*c, 1, 0)); run(*c, s, "size, 1-bit codes");
            std::vector<u8> t(bits / L); for (u32 i = 0; i < t.size(); i++) t[i] = sym_of_len(*c, L, i & 1);
            for (u32 i = 0; i < bits % L; i++) t.push_back(sym_of_len(*c, 1, 0));
            run(*c, t, "size, max-length codes");
        }
        {   // a long stream of the longest codes: every group of the steady form moves by the most it can
            std::vector<u8> s(16384); for (u32 i = 0; i < s.size(); i++) s[i] = sym_of_len(*c, L, (i * 7u >> 2) & 1); run(*c, s, "16384 max-length");
            for (u32 i = 0; i < s.size(); i++) s[i] = sym_of_len(*c, 1 + rand() % L, rand() & 1); run(*c, s, "16384 random");
        }
    }
    printf("cases %ld steady %ld general %ld reader %ld\n", g_cases, g_steady, g_general, g_reader);
    if (!g_steady || !g_general || !g_reader) { printf("a form was never taken\n"); return 1; }
    printf("done bad=%ld\n", g_bad);
    return g_bad != 0;
}
