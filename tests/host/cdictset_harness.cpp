// cdictset_harness.cpp — the slot assignment of ZSTDMI_compressBatchCDicts (zmi_cdictset.h) built for the CPU, so that it runs under
// AddressSanitizer / UBSan (tests/test_cdict_batch_abi.py): dedupe of the per-entry pointers, NULL entries, the bound of 65536
// distinct CDicts (NULL is none), and a pass's image (its sorted slot list and the per-chunk index into it).
#include <stdio.h>
#include <vector>
#include "zmi_cdictset.h"

using namespace zmi;

static int bad = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); ++bad; } } while (0)

// pointers that are never dereferenced: the addresses of the elements of one array
static std::vector<char> pool(kCDictSetMax + 2);
static const void* ptr(size_t k) { return &pool[k]; }

int main()
{
    std::vector<const void*> distinct; std::vector<uint32_t> slotOf;

    // no entries
    CHECK(cdict_slots_assign(nullptr, 0, distinct, slotOf) == 0 && distinct.empty() && slotOf.empty());
    printf("empty: %zu slots bad=%d\n", distinct.size(), bad);

    {   // dedupe, in order of first appearance, NULL a reference like any other; runs and returns to an earlier pointer
        const void* refs[] = { ptr(5), ptr(5), nullptr, ptr(9), ptr(5), nullptr, nullptr, ptr(2), ptr(9) };
        CHECK(cdict_slots_assign(refs, 9, distinct, slotOf) == 0);
        CHECK(distinct.size() == 4 && distinct[0] == ptr(5) && distinct[1] == nullptr && distinct[2] == ptr(9) && distinct[3] == ptr(2));
        const uint32_t want[] = { 0, 0, 1, 2, 0, 1, 1, 3, 2 };
        for (int i = 0; i < 9; ++i) CHECK(slotOf[i] == want[i]);
        printf("dedupe: %zu slots bad=%d\n", distinct.size(), bad);
    }
    {   // all NULL, and all one pointer: one slot
        std::vector<const void*> refs(1000, nullptr);
        CHECK(cdict_slots_assign(refs.data(), refs.size(), distinct, slotOf) == 0 && distinct.size() == 1 && distinct[0] == nullptr);
        refs.assign(1000, ptr(1));
        CHECK(cdict_slots_assign(refs.data(), refs.size(), distinct, slotOf) == 0 && distinct.size() == 1 && distinct[0] == ptr(1));
        for (uint32_t s : slotOf) CHECK(s == 0);
        printf("one for all: %zu slots bad=%d\n", distinct.size(), bad);
    }
    {   // 65536 distinct CDicts, each named twice, and a NULL entry in the middle, which is no CDict: accepted, 65537 slots; one more
        // CDict: refused, wherever the NULL entry stands
        std::vector<const void*> refs;
        for (size_t k = 0; k < kCDictSetMax; ++k) { if (k == 77) refs.push_back(nullptr); refs.push_back(ptr(k)); }
        for (size_t k = refs.size(); k-- > 0; ) refs.push_back(refs[k]);
        CHECK(cdict_slots_assign(refs.data(), refs.size(), distinct, slotOf) == 0 && distinct.size() == kCDictSetMax + 1);
        for (size_t i = 0; i < refs.size(); ++i) CHECK(slotOf[i] <= kCDictSetMax && distinct[slotOf[i]] == refs[i]);
        printf("65536: %zu slots bad=%d\n", distinct.size(), bad);
        refs.push_back(ptr(kCDictSetMax));
        CHECK(cdict_slots_assign(refs.data(), refs.size(), distinct, slotOf) == 1);
        refs.back() = ptr(3);                                       // (a further entry that names a known pointer is no 65537th CDict)
        CHECK(cdict_slots_assign(refs.data(), refs.size(), distinct, slotOf) == 0 && distinct.size() == kCDictSetMax + 1);
        refs.back() = nullptr;
        CHECK(cdict_slots_assign(refs.data(), refs.size(), distinct, slotOf) == 0 && distinct.size() == kCDictSetMax + 1);
        std::vector<const void*> late;                              // 65536 CDicts first, NULL behind them: accepted; 65537 and NULL: refused
        for (size_t k = 0; k < kCDictSetMax; ++k) late.push_back(ptr(k));
        late.push_back(nullptr);
        CHECK(cdict_slots_assign(late.data(), late.size(), distinct, slotOf) == 0 && distinct.size() == kCDictSetMax + 1 && slotOf.back() == kCDictSetMax);
        late.push_back(ptr(kCDictSetMax));
        CHECK(cdict_slots_assign(late.data(), late.size(), distinct, slotOf) == 1);
        printf("one more refused ok bad=%d\n", bad);
    }
    {   // a pass's image: the slots it holds, ascending, and each chunk's index among them
        std::vector<uint32_t> of = { 40, 7, 7, 65535, 40, 0, 7 }, used;
        CHECK(cdict_pass_image(of, used));
        CHECK(used.size() == 4 && used[0] == 0 && used[1] == 7 && used[2] == 40 && used[3] == 65535);
        const uint32_t want[] = { 2, 1, 1, 3, 2, 0, 1 };
        for (int i = 0; i < 7; ++i) CHECK(of[i] == want[i]);
        std::vector<uint32_t> one(5000, 9);
        CHECK(cdict_pass_image(one, used) && used.size() == 1 && used[0] == 9);
        for (uint32_t s : one) CHECK(s == 0);
        std::vector<uint32_t> none;
        CHECK(cdict_pass_image(none, used) && used.empty());
        printf("image: bad=%d\n", bad);
    }
    static_assert(sizeof(CDictSlot) == 88, "the record the kernels read");
    printf("done bad=%d\n", bad);
    return bad ? 1 : 0;
}
