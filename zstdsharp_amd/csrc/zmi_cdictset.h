// zmi_cdictset.h — the dictionaries of one ZSTDMI_compressBatchCDicts call: the slot record the set instances of the encode kernels
// read per chunk, and the host-side assignment of the caller's per-entry CDict pointers to slots.  Nothing here needs a HIP header, so
// that tests/host/cdictset_harness.cpp builds the assignment for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <unordered_map>
#include <vector>

namespace zmi {

struct DictCTables;     // zmi_common.h

// an indexed dictionary (ZSTDMI_CCtx_setDictIndex; lz_fast.hip): `end` = the byte behind its content on the device (readable for 64
// bytes more), `len` = the indexed bytes in front of `end`, `table` = 1 << log buckets under the fast finder's hash; tableLong /
// tableShort (ZSTDMI_CCtx_setDictIndexStrategy(2); else null) = as many under each of the dual finder's two
struct DictIndexRef { const uint8_t* end; uint32_t len; const uint32_t* table; uint32_t log; const uint32_t* tableLong; const uint32_t* tableShort; };

// One dictionary as the encode kernels' set instances take it: everything the single-dictionary instances get as launch constants.
// A pass uploads one record per distinct CDict among its entries and, beside chunkLens, each chunk's index into them.  The index is
// the same for every lane of a workgroup (of a wave in seq_encode), so the fields arrive by scalar loads.
struct CDictSlot {
    const uint8_t* tail;            // the staged tail: tailLen bytes in front of every chunk (null with tailLen 0: none, or indexed)
    const DictCTables* dct;         // the dictionary's entropy tables (null: raw content, or ZSTDMI_CCtx_setDictEntropy off)
    DictIndexRef dix;               // the indexed content (read by the indexed instances alone)
    uint32_t tailLen;
    uint32_t dictID, dictIdBytes;   // as the frame header writes them (ZSTD_c_dictIDFlag = 0: no bytes)
    uint32_t rep[3];                // the repcodes in front of every frame
};
static_assert(sizeof(DictIndexRef) == 48 && sizeof(CDictSlot) == 88, "CDictSlot is read by device code as laid out here");

constexpr uint32_t kCDictSetMax = 65536;    // distinct CDicts one call takes at most (parameter_unsupported beyond)

// The caller's n pointers (null = an entry without a dictionary: a slot like any other, but no CDict: it does not count toward the
// bound) -> distinct[] in order of first appearance and slotOf[i] = the index of refs[i] in it.  0: done; 1: more than kCDictSetMax
// distinct CDicts; 2: memory ran out.
inline int cdict_slots_assign(const void* const* refs, size_t n, std::vector<const void*>& distinct, std::vector<uint32_t>& slotOf)
{
    try {
        distinct.clear(); slotOf.assign(n, 0);
        std::unordered_map<const void*, uint32_t> seen;
        size_t nulls = 0;       // 1 once a null entry has its slot
        for (size_t i = 0; i < n; ++i) {
            // (a run of entries behind one dictionary, the usual order of a store's writer, asks the map once)
            if (i && refs[i] == refs[i - 1]) { slotOf[i] = slotOf[i - 1]; continue; }
            const auto it = seen.find(refs[i]);
            if (it != seen.end()) { slotOf[i] = it->second; continue; }
            if (refs[i] && distinct.size() - nulls >= kCDictSetMax) return 1;
            if (!refs[i]) nulls = 1;
            slotOf[i] = (uint32_t)distinct.size();
            seen.emplace(refs[i], slotOf[i]);
            distinct.push_back(refs[i]);
        }
    } catch (...) { return 2; }
    return 0;
}

// A pass's image: of[k] = the call-wide slot of the pass's chunk k -> used[] = the slots the pass holds, ascending (the order of its
// slot table), and of[k] rewritten to the chunk's index in used[].  false: memory ran out (`of` is then as it was).
inline bool cdict_pass_image(std::vector<uint32_t>& of, std::vector<uint32_t>& used)
{
    try {
        used.assign(of.begin(), of.end());
        std::sort(used.begin(), used.end());
        used.erase(std::unique(used.begin(), used.end()), used.end());
    } catch (...) { return false; }
    for (uint32_t& s : of) s = (uint32_t)(std::lower_bound(used.begin(), used.end(), s) - used.begin());
    return true;
}

} // namespace zmi
