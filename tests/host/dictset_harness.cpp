// Stand-alone CPU harness of the DDict set behind ZSTD_d_refMultipleDDicts (zstdsharp_amd/csrc/zmi_dictset.h): the host-side set
// (insert in any order, replace by equal dictID, the sorted image) and the very lookup the walk kernels run over that image.
// tests/test_ddict_set_abi.py builds it with -fsanitize=address,undefined.  Every image searched is a heap block of exactly its size, so
// a probe beyond the table stops the program.  The set's references are plain integers here (the library's are DDict pointers).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>
#include "zmi_dictset.h"

using zmi::DictSlot;
using zmi::kNoSlot;
typedef zmi::DictSet<uint64_t> Set;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// the image as the device would hold it: n + 1 records on the heap, exactly
struct Image {
    DictSlot* p; uint32_t n;
    Image(const Set& s, uint64_t current, uint32_t currentID)
    {
        std::vector<DictSlot> v;
        const bool ok = s.image(v, current, [&](uint64_t ref, DictSlot& r) { r.dictID = ref == current && ref == ~0ull ? currentID : (uint32_t)(ref >> 32); r.contentSize = (uint32_t)ref; });
        if (!ok) { printf("image: out of memory\n"); exit(2); }
        n = (uint32_t)s.size();
        p = (DictSlot*)malloc(v.size() * sizeof(DictSlot));
        memcpy(p, v.data(), v.size() * sizeof(DictSlot));
    }
    ~Image() { free(p); }
};
static uint64_t ref_of(uint32_t id, uint32_t payload) { return ((uint64_t)id << 32) | payload; }

// a set of the given ids inserted in random order, some twice (the second insert replaces): model = id -> the payload that must win
static int check_set(const std::vector<uint32_t>& ids, const std::vector<uint32_t>& absent, const char* what)
{
    int bad = 0;
    Set s; std::map<uint32_t, uint32_t> model;
    std::vector<uint32_t> order = ids;
    for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[rnd() % i]);
    for (uint32_t id : order) { const uint32_t pay = rnd(); bad += !s.insert(id, ref_of(id, pay)); model[id] = pay; }
    for (size_t k = 0; k < order.size(); k += 3) { const uint32_t id = order[k], pay = rnd(); const uint64_t g = s.gen; bad += !s.insert(id, ref_of(id, pay)); bad += s.gen == g; model[id] = pay; }
    bad += s.size() != model.size();
    // the sorted image: strictly ascending dictIDs, each with the payload that was inserted last
    const uint32_t currentID = 0x0C0FFEE0u;
    Image im(s, ~0ull, currentID);
    size_t i = 0;
    for (const auto& kv : model) { bad += im.p[i].dictID != kv.first || im.p[i].contentSize != kv.second; if (i) bad += im.p[i - 1].dictID >= im.p[i].dictID; ++i; }
    bad += im.p[im.n].dictID != currentID;
    // the lookup: every present id at its index; absent ids nowhere; dictID 0 never
    i = 0;
    for (const auto& kv : model) { if (kv.first) bad += zmi::dictset_find(im.p, im.n, kv.first) != (uint32_t)i; ++i; }
    bad += zmi::dictset_find(im.p, im.n, 0) != kNoSlot;
    for (uint32_t id : absent) if (!model.count(id)) bad += zmi::dictset_find(im.p, im.n, id) != kNoSlot;
    // the rule: found -> its record, in the set; not found -> the current DDict's record, wrong unless it is the current one's id or none
    for (uint32_t id : absent) {
        uint32_t inSet = 9, wrong = 9;
        const uint32_t slot = zmi::dictset_select(im.p, im.n, id, &inSet, &wrong);
        if (id && model.count(id)) bad += slot == im.n || !inSet || wrong || im.p[slot].dictID != id;
        else bad += slot != im.n || inSet || wrong != (id != 0 && id != currentID ? 1u : 0u);
    }
    { uint32_t inSet = 9, wrong = 9; bad += zmi::dictset_select(im.p, im.n, currentID, &inSet, &wrong) != im.n || inSet || wrong; }
    { uint32_t inSet = 9, wrong = 9; bad += zmi::dictset_select(im.p, im.n, 0, &inSet, &wrong) != im.n || inSet || wrong; }
    printf("%s: %zu entries bad=%d\n", what, model.size(), bad);
    return bad;
}

int main()
{
    int bad = 0;
    const std::vector<uint32_t> probes = { 0, 1, 2, 3, 5, 6, 7, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu, 1000, 1001, 1002 };
    bad += check_set({}, probes, "empty");
    bad += check_set({ 0x80000000u }, probes, "one");
    bad += check_set({ 1, 0xFFFFFFFFu }, probes, "two (first and last id)");
    bad += check_set({ 0x7FFFFFFFu, 0x80000000u, 1 }, probes, "three (adjacent across the sign bit)");
    bad += check_set({ 0, 1, 2, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 5, 7, 1000, 1002 }, probes, "ten (raw content in front, 6 and 1001 absent between neighbours)");
    {   // 4096 entries: odd ids (every even id is absent between two present ones), plus the extremes
        std::vector<uint32_t> ids, absent = probes;
        for (uint32_t i = 0; i < 4094; ++i) { ids.push_back(2 * i + 1); if (i % 97 == 0) absent.push_back(2 * i + 2); }
        ids.push_back(0x80000000u); ids.push_back(0xFFFFFFFFu);
        for (uint32_t id : ids) if (id % 5 == 0) absent.push_back(id);
        bad += check_set(ids, absent, "4096");
    }
    {   // the cap: kDictSetMax entries, then one more is refused and the set is as it was; a replacement still goes through
        Set s; int b = 0;
        for (uint32_t i = 0; i < zmi::kDictSetMax; ++i) b += !s.insert(i * 3 + 1, i);
        const uint64_t g = s.gen;
        b += s.insert(2, 7) || s.size() != zmi::kDictSetMax || s.gen != g;
        b += !s.insert(4, 99) || s.size() != zmi::kDictSetMax || s.entries[1].ref != 99;
        printf("cap: %u entries, one more refused %s\n", zmi::kDictSetMax, b ? "WRONG" : "ok");
        bad += b;
    }
    printf("done bad=%d\n", bad);
    return bad ? 1 : 0;
}
