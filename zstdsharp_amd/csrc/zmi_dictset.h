// zmi_dictset.h — the set of digested dictionaries behind ZSTD_d_refMultipleDDicts (U/ZstdDecompress.cs:8-115, 343-366, 2300-2339):
// the slot table the decode kernels read, the lookup of a frame's dictID in it, and the host-side set the table is made from.
// The lookup is __host__ __device__ and nothing here needs a HIP header, so that tests/host/dictset_harness.cpp can build the very
// search the walk kernels run, and the set's insert / replace / sorted image, for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <new>
#include <vector>

#if defined(__HIPCC__)
#define ZMI_SET_HD __host__ __device__
#else
#define ZMI_SET_HD
#endif

namespace zmi {

// One dictionary as the decode kernels take it: what DecodeDict and DictInfo say of it (zstd_mi355x_dec.hip, zmi_common.h).  The
// table holds one record per DDict of the set, sorted by dictID (raw-content DDicts, dictID 0, in front), and behind them one more
// record for the context's current DDict: FrameDesc::dictSlot indexes it.  A few KiB; every workgroup reads it from L2.
struct DictSlot {
    const uint8_t* dictFull;        // a formatted dictionary's bytes, header included (null: raw content)
    const uint8_t* content;         // the history in front of every frame behind this dictionary (null: none)
    const uint32_t* seqTabs;        // a formatted DDict's ready-made sequence tables (kDictTabWords words)
    uint32_t contentSize;
    uint32_t dictID;                // 0: raw content, never selected by a frame
    uint32_t formatted;             // 1: frames start from the dictionary's Huffman table, FSE tables and repcodes
    uint32_t hufOff, hufSize;       // DictInfo's fields, for a formatted dictionary
    uint32_t ofOff, mlOff, llOff, repOff;
    uint32_t rep[3];
};
static_assert(sizeof(DictSlot) == 72, "DictSlot is read by device code as laid out here");

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kDictSetMax = 65536;     // entries a set holds at most (ZSTD_DCtx_refDDict: memory_allocation beyond)

// index of the record with this dictID among slots[0, n), sorted by dictID; kNoSlot when there is none.  dictID 0 names no dictionary.
ZMI_SET_HD inline uint32_t dictset_find(const DictSlot* slots, uint32_t n, uint32_t dictID)
{
    if (!dictID) return kNoSlot;
    uint32_t lo = 0, hi = n;                // the first record whose dictID is >= the one looked for
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (slots[mid].dictID < dictID) lo = mid + 1; else hi = mid; }
    return (lo < n && slots[lo].dictID == dictID) ? lo : kNoSlot;
}

// The rule of ZSTD_d_refMultipleDDicts for one frame, independent of its neighbours: a dictID found in the set selects that record
// (*inSet = 1); every other frame is the current DDict's (record n), and is wrong (*wrong = 1) when it names a dictID that is not the
// current one's (U/ZstdDecompress.cs:1404-1412).
ZMI_SET_HD inline uint32_t dictset_select(const DictSlot* slots, uint32_t n, uint32_t dictID, uint32_t* inSet, uint32_t* wrong)
{
    const uint32_t k = dictset_find(slots, n, dictID);
    *inSet = k != kNoSlot ? 1u : 0u;
    *wrong = (k == kNoSlot && dictID && dictID != slots[n].dictID) ? 1u : 0u;
    return k != kNoSlot ? k : n;
}

// The host side: (dictID, the caller's DDict) pairs kept sorted by dictID; a DDict whose dictID is there already replaces that entry
// (ZSTD_DDictHashSet_emplaceDDict, U/ZstdDecompress.cs:33-38).  References only; the DDicts are the caller's.
template <class Ref>
struct DictSet {
    struct Entry { uint32_t dictID; Ref ref; };
    std::vector<Entry> entries;
    uint64_t gen = 0;               // bumped by every change: the device image is uploaded again when it differs

    size_t size() const { return entries.size(); }
    size_t lower(uint32_t dictID) const
    {
        size_t lo = 0, hi = entries.size();
        while (lo < hi) { const size_t mid = lo + ((hi - lo) >> 1); if (entries[mid].dictID < dictID) lo = mid + 1; else hi = mid; }
        return lo;
    }
    // -> false: the set is full or memory ran out; the set is then as it was
    bool insert(uint32_t dictID, Ref ref)
    {
        const size_t at = lower(dictID);
        if (at < entries.size() && entries[at].dictID == dictID) { entries[at].ref = ref; gen++; return true; }
        if (entries.size() >= kDictSetMax) return false;
        try { entries.insert(entries.begin() + (ptrdiff_t)at, Entry{ dictID, ref }); } catch (...) { return false; }
        gen++;
        return true;
    }
    // the sorted image: one record per entry by fill(ref, record), then the record of `current` -> false: memory ran out
    template <class Fill>
    bool image(std::vector<DictSlot>& out, Ref current, Fill fill) const
    {
        try { out.assign(entries.size() + 1, DictSlot{}); } catch (...) { return false; }
        for (size_t i = 0; i < entries.size(); ++i) fill(entries[i].ref, out[i]);
        fill(current, out[entries.size()]);
        return true;
    }
};

} // namespace zmi
