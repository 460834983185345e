// Stand-alone CPU harness of pack_runs (zstdsharp_amd/csrc/zmi_pack_runs.h), the host step of ZSTDMI_decompressRanges that packs the
// touched frames' compressed bytes into one staging buffer.  tests/test_ranges_abi.py builds it with -fsanitize=address,undefined.
// The buffers are heap blocks of exactly the sizes stated, so a byte read or written beyond them stops the program.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "zmi_pack_runs.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main()
{
    int bad = 0;
    const size_t srcSize = 100000;
    uint8_t* src = (uint8_t*)malloc(srcSize);
    for (size_t i = 0; i < srcSize; ++i) src[i] = (uint8_t)(i * 131 + (i >> 8));

    {   // an empty list: nothing is read, nothing written (no buffers at all)
        const size_t n = zmi::pack_runs(nullptr, 0, nullptr, 0, nullptr, 0);
        printf("empty list: %zu bytes\n", n);
        bad += n != 0;
    }
    {   // one run that is the whole front of the stream, into a destination of exactly that size
        const uint64_t run[2] = {0, srcSize};
        uint8_t* dst = (uint8_t*)malloc(srcSize);
        const size_t n = zmi::pack_runs(run, 1, src, srcSize, dst, srcSize);
        const bool ok = n == srcSize && memcmp(dst, src, srcSize) == 0;
        printf("whole front: %zu bytes %s\n", n, ok ? "ok" : "WRONG");
        bad += !ok;
        free(dst);
    }
    {   // 1000 seeded runs, ascending and disjoint as the plan kernel writes them (some empty, the last one ends at the source's end)
        std::vector<uint64_t> cuts(2000);
        for (auto& c : cuts) c = rnd() % (srcSize + 1);
        cuts[1999] = srcSize;
        for (size_t i = 1; i < cuts.size(); ++i) { size_t j = i; while (j && cuts[j - 1] > cuts[j]) { uint64_t t = cuts[j]; cuts[j] = cuts[j - 1]; cuts[j - 1] = t; --j; } }
        size_t want = 0;
        for (size_t r = 0; r < 1000; ++r) want += (size_t)(cuts[2 * r + 1] - cuts[2 * r]);
        uint8_t* dst = (uint8_t*)malloc(want ? want : 1);
        const size_t n = zmi::pack_runs(cuts.data(), 1000, src, srcSize, dst, want);
        bool ok = n == want;
        size_t at = 0;
        for (size_t r = 0; ok && r < 1000; ++r) { const size_t len = (size_t)(cuts[2 * r + 1] - cuts[2 * r]); ok = memcmp(dst + at, src + cuts[2 * r], len) == 0; at += len; }
        printf("1000 seeded runs: %zu bytes %s\n", n, ok ? "ok" : "WRONG");
        bad += !ok;
        free(dst);
    }
    {   // lists the kernels never write are refused, with nothing written past what fits
        uint8_t* dst = (uint8_t*)malloc(64);
        const uint64_t reversed[2] = {50, 40}, beyond[2] = {srcSize - 10, srcSize + 1}, large[4] = {0, 60, 60, 70};
        const bool ok = zmi::pack_runs(reversed, 1, src, srcSize, dst, 64) == (size_t)-1 && zmi::pack_runs(beyond, 1, src, srcSize, dst, 64) == (size_t)-1 &&
                        zmi::pack_runs(large, 2, src, srcSize, dst, 64) == (size_t)-1;
        printf("refused: reversed, beyond the source, beyond the destination %s\n", ok ? "ok" : "WRONG");
        bad += !ok;
        free(dst);
    }
    free(src);
    printf("done bad=%d\n", bad);
    return bad ? 1 : 0;
}
