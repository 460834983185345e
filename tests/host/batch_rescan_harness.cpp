// Stand-alone CPU harness of the per-entry rescan behind ZSTDMI_DCtx_setBatchUnsized (zstdsharp_amd/csrc/zmi_batch_rescan.h): the
// placement rule batch_rescan_kernel runs — 64 frames a step, saturating sums, the verdict against the capacity — against a scalar
// loop of this file.  tests/test_batch_unsized_abi.py builds it with -fsanitize=address,undefined.  Sizes and places are heap blocks of
// exactly their length, so a step that reaches past an entry's frames stops the program.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zmi_batch_rescan.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// the scalar reference: places, the total (all ones once the true sum passes 2^64 - 1), fits
static bool reference(const uint64_t* sizes, uint32_t n, uint64_t entryOff, uint64_t cap, uint64_t* places, uint64_t* total)
{
    unsigned __int128 run = 0; const unsigned __int128 top = ~(uint64_t)0;
    for (uint32_t i = 0; i < n; ++i) { places[i] = entryOff + (uint64_t)(run > top ? top : run); run += sizes[i]; }
    *total = (uint64_t)(run > top ? top : run);
    return run < top && run <= cap;
}

// one entry through both; `placesMatter`: the places are compared too (always, except behind the point where the sum has saturated)
static int check(const std::vector<uint64_t>& sizes, uint64_t entryOff, uint64_t cap, bool wantFits, const char* what)
{
    const uint32_t n = (uint32_t)sizes.size();
    uint64_t* in = (uint64_t*)malloc(n ? n * sizeof(uint64_t) : 1);
    uint64_t* got = (uint64_t*)malloc(n ? n * sizeof(uint64_t) : 1);
    uint64_t* want = (uint64_t*)malloc(n ? n * sizeof(uint64_t) : 1);
    if (n) memcpy(in, sizes.data(), n * sizeof(uint64_t));
    uint64_t totalGot = 1, totalWant = 2;
    const bool fitsGot = zmi::rescan_entry(in, n, entryOff, cap, got, &totalGot);
    const bool fitsWant = reference(in, n, entryOff, cap, want, &totalWant);
    int bad = 0;
    bad += fitsGot != fitsWant || fitsWant != wantFits || totalGot != totalWant;
    for (uint32_t i = 0; i < n; ++i) bad += got[i] != want[i];
    printf("%s: %u frames cap %llu total %llu fits %d bad=%d\n", what, n, (unsigned long long)cap, (unsigned long long)totalGot, (int)fitsGot, bad);
    free(in); free(got); free(want);
    return bad;
}

int main()
{
    int bad = 0;
    const uint32_t counts[] = { 0, 1, 63, 64, 65, 5000 };
    for (uint32_t n : counts) {
        std::vector<uint64_t> sizes(n);
        uint64_t sum = 0;
        for (auto& s : sizes) { s = rnd() % 3 == 0 ? 0 : rnd() % 131073; sum += s; }
        char name[64];
        snprintf(name, sizeof name, "n=%u at capacity", n);            bad += check(sizes, 12345, sum, true, name);
        snprintf(name, sizeof name, "n=%u capacity + 1", n);           if (n) { sizes[n / 2] += 1; bad += check(sizes, 12345, sum, false, name); sizes[n / 2] -= 1; }
        snprintf(name, sizeof name, "n=%u roomy", n);                  bad += check(sizes, 0, sum + 1000, true, name);
        snprintf(name, sizeof name, "n=%u capacity 0", n);             bad += check(sizes, 7, 0, sum == 0, name);
        // sums at and beyond 2^64 - 1: the running total must stay at all ones (too small for every capacity), never wrap
        if (n >= 2) {
            std::vector<uint64_t> big = sizes;
            big[0] = ~(uint64_t)0 - sum + big[0];                   // the true sum is exactly 2^64 - 1
            snprintf(name, sizeof name, "n=%u sum 2^64-1", n);         bad += check(big, 0, ~(uint64_t)0, false, name);
            big[n - 1] += 1;                                        // one more: wraps to 0 in plain arithmetic
            snprintf(name, sizeof name, "n=%u sum 2^64", n);           bad += check(big, 0, ~(uint64_t)0, false, name);
            big[n / 2] = ~(uint64_t)0;                              // far beyond, saturating in the middle of a step
            snprintf(name, sizeof name, "n=%u sum far beyond", n);     bad += check(big, 0, 1000, false, name);
            snprintf(name, sizeof name, "n=%u sum far beyond, cap max", n); bad += check(big, 0, ~(uint64_t)0, false, name);
        }
    }
    {   // the lane rules one by one
        int b = 0;
        b += zmi::rescan_add(~(uint64_t)0, 1) != ~(uint64_t)0 || zmi::rescan_add(5, 6) != 11 || zmi::rescan_add(~(uint64_t)0 - 1, 1) != ~(uint64_t)0;
        b += zmi::rescan_round(5, 9, 3, 4) != 5 || zmi::rescan_round(5, 9, 4, 4) != 14;
        b += zmi::rescan_before(100, 999, 0) != 100 || zmi::rescan_before(100, 7, 1) != 107;
        b += !zmi::rescan_fits(10, 10) || zmi::rescan_fits(11, 10) || zmi::rescan_fits(~(uint64_t)0, ~(uint64_t)0) || !zmi::rescan_fits(0, 0);
        printf("lane rules %s\n", b ? "WRONG" : "ok");
        bad += b;
    }
    printf("done bad=%d\n", bad);
    return bad ? 1 : 0;
}
