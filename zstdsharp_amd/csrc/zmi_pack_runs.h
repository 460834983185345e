// zmi_pack_runs.h — plain host code of ZSTDMI_decompressRanges: the compressed bytes of the touched frames of a host source, packed
// one run behind the other into the staging buffer that travels to the device in one copy.  No device code and no HIP header, so that
// tests/host/pack_runs_harness.cpp can build it for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace zmi {

// runs: nRuns pairs [lo, hi) of byte offsets into src (srcSize bytes).  Copies them in list order to dst (dstCapacity bytes) and
// returns the bytes written, or (size_t)-1 — with nothing further written — at the first run that is reversed, leaves the source or
// does not fit (the kernels that write the list never produce one: DESIGN.md §5h; the host checks all the same).
inline size_t pack_runs(const uint64_t* runs, size_t nRuns, const uint8_t* src, size_t srcSize, uint8_t* dst, size_t dstCapacity)
{
    size_t at = 0;
    for (size_t r = 0; r < nRuns; ++r) {
        const uint64_t lo = runs[2 * r], hi = runs[2 * r + 1];
        if (lo > hi || hi > srcSize || hi - lo > dstCapacity - at) return (size_t)-1;
        if (hi > lo) memcpy(dst + at, src + lo, (size_t)(hi - lo));
        at += (size_t)(hi - lo);
    }
    return at;
}

} // namespace zmi
