// zmi_carry.h — carry groups (ZSTDMI_CCtx_setEntropyCarry): which chunks of a pass the entropy stage walks in order, one behind the
// other, so that a block may reuse the Huffman table, the FSE tables and the repcodes the blocks before it left in the decoder.
// A group is kCarryGroup consecutive blocks of ONE frame, aligned to multiples of kCarryGroup of the block's index in its frame; a
// group's first block carries nothing in.  Plain integer code in the manner of zmi_frame.h: seq_enc.hip and the host include it under
// hipcc, tests/host/carry_groups_harness.cpp builds it for the CPU.
#pragma once
#include "zmi_frame.h"

namespace zmi {

// A choice, not a measurement: it bounds the serial chain of one wave (eight blocks instead of one) and leaves a large input thousands
// of groups to run side by side (a pass of 16384 chunks has at least 2048).
constexpr uint32_t kCarryGroup = 8;

// chunks [first, first + count) of the pass; count 0: the pass has no such group
struct CarrySpan { uint32_t first, count; };

ZMI_HD uint32_t carry_groups_per_frame(uint32_t frameBlocks) { return (frameBlocks + kCarryGroup - 1) / kCarryGroup; }

// ---- kArith: every frameBlocks consecutive chunks are a frame (the pass's last one may be shorter) ----
ZMI_HD uint32_t carry_groups_arith(uint32_t nChunks, uint32_t frameBlocks)
{
    return nChunks / frameBlocks * carry_groups_per_frame(frameBlocks) + carry_groups_per_frame(nChunks % frameBlocks);
}
ZMI_HD CarrySpan carry_span_arith(uint32_t nChunks, uint32_t frameBlocks, uint32_t group)
{
    const uint32_t per = carry_groups_per_frame(frameBlocks), frame = group / per;
    const uint64_t first = (uint64_t)frame * frameBlocks + (uint64_t)(group % per) * kCarryGroup;
    if (first >= nChunks) return CarrySpan{ 0u, 0u };
    uint64_t end = first + kCarryGroup;
    const uint64_t frameEnd = ((uint64_t)frame + 1) * frameBlocks;
    if (end > frameEnd) end = frameEnd;
    if (end > nChunks) end = nChunks;
    return CarrySpan{ (uint32_t)first, (uint32_t)(end - first) };
}

// ---- kSingle: ONE frame; chunk c is its block (at + c * chunkBytes) / chunkBytes.  A pass or a stream batch that begins inside a
// group begins a group of its own there (nothing is carried across a launch), and ends one where it ends ----
ZMI_HD uint32_t carry_single_lead(uint64_t at, uint32_t chunkBytes) { return (uint32_t)(at / chunkBytes % kCarryGroup); }
ZMI_HD uint32_t carry_groups_single(uint32_t nChunks, uint64_t at, uint32_t chunkBytes)
{
    return (uint32_t)(((uint64_t)carry_single_lead(at, chunkBytes) + nChunks + kCarryGroup - 1) / kCarryGroup);
}
ZMI_HD CarrySpan carry_span_single(uint32_t nChunks, uint64_t at, uint32_t chunkBytes, uint32_t group)
{
    const uint32_t lead = carry_single_lead(at, chunkBytes);
    const uint64_t first = group ? (uint64_t)group * kCarryGroup - lead : 0u;
    if (first >= nChunks) return CarrySpan{ 0u, 0u };
    uint64_t end = ((uint64_t)group + 1) * kCarryGroup - lead;
    if (end > nChunks) end = nChunks;
    return CarrySpan{ (uint32_t)first, (uint32_t)(end - first) };
}
// chunks per pass of a one-shot call under the single frame: whole groups (at least one), so that where a group begins is a function of
// the input and the parameters alone, whatever ZSTDMI_CCtx_setPassChunks says
ZMI_HD uint32_t carry_pass_chunks(uint32_t passChunks) { return passChunks < kCarryGroup ? kCarryGroup : passChunks - passChunks % kCarryGroup; }

// ---- kTable: a batch's entries differ in length, so the host lists the chunks that lead a group beside the table it already
// builds: leaders[g] = the first chunk of group g, leaders[nGroups] = nChunks ----
ZMI_HD bool carry_word_leads(uint32_t frameWord) { return frame_word_block(frameWord) % kCarryGroup == 0; }
// -> groups; leaders (nullptr: count only) has room for nChunks + 1 words
ZMI_HD uint32_t carry_leaders_table(const uint32_t* table, uint32_t nChunks, uint32_t* leaders)
{
    uint32_t g = 0;
    for (uint32_t c = 0; c < nChunks; ++c) if (carry_word_leads(table[c])) { if (leaders) leaders[g] = c; ++g; }
    if (leaders) leaders[g] = nChunks;
    return g;
}
ZMI_HD CarrySpan carry_span_table(const uint32_t* leaders, uint32_t nGroups, uint32_t group)
{
    if (group >= nGroups) return CarrySpan{ 0u, 0u };
    return CarrySpan{ leaders[group], leaders[group + 1] - leaders[group] };
}

// the span of group `group` of a pass of nChunks chunks laid out as g says
template <int FORM>
ZMI_HD CarrySpan carry_span(const FrameLayout& g, uint32_t nChunks, const uint32_t* leaders, uint32_t nGroups, uint32_t group)
{
    if (FORM == kSingle) return carry_span_single(nChunks, g.at, g.chunkBytes, group);
    if (FORM == kTable) return carry_span_table(leaders, nGroups, group);
    return carry_span_arith(nChunks, g.frameBlocks, group);
}

} // namespace zmi
