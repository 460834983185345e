// zmi_batch_pass.h — the host decisions of a batched compress pass (compress_entries, zstd_mi355x.hip), each stated once:
// which entries share a group, where a group is cut into passes, how a pass's upload table is laid out, and what the host writes into
// it.  Beside the synchronous table, the three layouts of the calls enqueued from the device, so that every
// layout of the context's batchTab and packAsync stands in this file.  Plain C++ without a HIP header: the host includes it under
// hipcc (zmi_host.h), tests/host/batch_plan_harness.cpp builds it for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <assert.h>
#include <string.h>
#include "zmi_cparams.h"
#include "zmi_batch_plan.h"
#include "zmi_cdictset.h"
#include "zmi_carry.h"

namespace zmi {

// ---- the group key: what has to be equal for two entries' chunks to share a pass ----
// what a call's parameters resolve to for an entry's size: the compression parameters and what the finder is launched with
struct Resolved { CParams cp; u32 finder, minStrideLog, rawLiterals; };
// What of two entries' resolved parameters has to be equal for their chunks to share a launch: the parts the kernels act on (finder,
// probing stride, raw literals, seq_encode's strategy constants, the chain search's depth).  The rest of a CParams — windowLog, hashLog
// and chainLog, which ZSTD_adjustCParams shrinks with the entry's size — reaches no kernel.
inline bool same_launch_params(const Resolved& a, const Resolved& b)
{
    return a.finder == b.finder && a.minStrideLog == b.minStrideLog && a.rawLiterals == b.rawLiterals && a.cp.strategy == b.cp.strategy && a.cp.searchLog == b.cp.searchLog;
}
// An entry's framing as far as a group asks: a view, built where two entries are compared (rs is not copied: the comparison
// runs once per entry of a call).  slot: its CDict's index among the call's (per-entry CDicts; else 0).
// plain: nothing of a dictionary is staged or indexed for it (the finder's plain instance: no set form).
struct BatchGroupKey {
    u32 prefixLen, chunkBytes, frameBlocks; bool dictIndex; const Resolved& rs; u32 slot;
    bool plain() const { return !prefixLen && !dictIndex; }
};
// A call without per-entry CDicts keeps its classes by the dictionary's staged tail and the whole of Resolved, and so its passes.
// With them (perEntry), entries share a group by what has to be equal for their chunks to share a launch — chunk size (the staged tail
// in whole 4 KiB tiles), blocks per frame, indexed or not, same_launch_params — not by the dictionary nor by the tail's exact length.
// Only where nothing of the dictionary is staged or indexed — no dictionary, content below 8 bytes — the finder runs its plain
// instance, which has no set form and takes the header's dictID bytes as launch constants: such entries group by CDict as well, and
// never with staged or indexed ones, whatever else is equal: under ZSTD_c_windowLog 10 .. 15 both kinds have chunks of one window.
inline bool same_group(const BatchGroupKey& a, const BatchGroupKey& b, bool perEntry)
{
    if (a.chunkBytes != b.chunkBytes || a.frameBlocks != b.frameBlocks || a.dictIndex != b.dictIndex) return false;
    if (!perEntry) return a.prefixLen == b.prefixLen && !memcmp(&a.rs, &b.rs, sizeof(Resolved));
    return a.plain() == b.plain() && (!a.plain() || a.slot == b.slot) && same_launch_params(a.rs, b.rs);
}

// ---- the pass cut ----
// A pass holds whole entries, up to passLimit chunks, and an entry larger than what is left starts the next pass — except as a pass's
// first (an entry of more chunks than a pass is not batched at all: entry_batched).  -> the end m1 of the pass that begins at member m0
// of [m0, end), and its chunks in nCh; chunksOf(m) = the chunks of member m.  ZSTDMI_compressPack cuts its rounds by it.
template <class ChunksOf>
inline size_t batch_pass_cut(size_t m0, size_t end, u32 passLimit, ChunksOf chunksOf, u32& nCh)
{
    size_t m1 = m0; nCh = 0;
    while (m1 < end) {
        const u32 k = chunksOf(m1);
        if (nCh && nCh + k > passLimit) break;
        nCh += k; ++m1;
    }
    return m1;
}
// A pack's rounds lie inside runs of entries the batch takes (flag[k] != 0): the end of the run that begins at i, looked for up to `end`.
// (A round holds at most passLimit entries, each of a chunk or more, so i + passLimit bounds what a round asks.)
inline size_t batch_run_end(const u8* flag, size_t i, size_t end) { while (i < end && flag[i]) ++i; return i; }

// ---- the pass's table, one upload ----
// from[nCh] | entDst[nEnt] | entCap[nEnt] (u64) | len[nCh] | entFirst[nEnt + 1] | with multi-block frames frame[nCh] | a pack:
// entSeek[nEnt] | a set pass (nSlots >= 2 distinct CDicts; 0: none): chunkSlot[nCh] (u32) | slots[nSlots] (CDictSlot) | carried
// entropy state: leaders[nCh + 1] (u32).  Behind it, at `bytes`, the entries' sizes that come back (u64[nEnt], device only).
// A column that is not there has the offset of the one behind it.
struct BatchPassTab {
    size_t atDst, atCap, atLen, atFirst, atFrame, atSeek, atChunkSlot, atSlots, atLead, bytes;
    bool frameWords, seek, set, carry;
};
inline BatchPassTab batch_pass_tab(u32 nCh, u32 nEnt, bool frameWords, bool seek, u32 nSlots, bool carry)
{
    BatchPassTab t;
    t.frameWords = frameWords; t.seek = seek; t.set = nSlots != 0; t.carry = carry;
    t.atDst = (size_t)nCh * 8; t.atCap = t.atDst + (size_t)nEnt * 8; t.atLen = t.atCap + (size_t)nEnt * 8; t.atFirst = t.atLen + (size_t)nCh * 4;
    t.atFrame = t.atFirst + ((size_t)nEnt + 1) * 4;
    t.atSeek = t.atFrame + (frameWords ? (size_t)nCh * 4 : 0);
    t.atChunkSlot = t.atSeek + (seek ? (size_t)nEnt * 4 : 0);
    t.atSlots = (t.atChunkSlot + (t.set ? (size_t)nCh * 4 : 0) + 7) & ~(size_t)7;
    t.atLead = (t.atSlots + (size_t)nSlots * sizeof(CDictSlot) + 7) & ~(size_t)7;
    t.bytes = (t.atLead + (carry ? ((size_t)nCh + 1) * 4 : 0) + 7) & ~(size_t)7;
    return t;
}
// the columns of an image of the table, on the host or on the device: null where the pass has no such column
struct BatchPassCols {
    u64* from; u64* entDst; u64* entCap; u32* len; u32* entFirst; u32* frame; u32* entSeek; u32* chunkSlot; CDictSlot* slots; u32* leaders;
    u64* got;       // (behind the table: on the device only)
};
inline BatchPassCols batch_pass_cols(const BatchPassTab& t, u8* image)
{
    return BatchPassCols{ (u64*)image, (u64*)(image + t.atDst), (u64*)(image + t.atCap), (u32*)(image + t.atLen), (u32*)(image + t.atFirst),
                          t.frameWords ? (u32*)(image + t.atFrame) : nullptr, t.seek ? (u32*)(image + t.atSeek) : nullptr,
                          t.set ? (u32*)(image + t.atChunkSlot) : nullptr, t.set ? (CDictSlot*)(image + t.atSlots) : nullptr,
                          t.carry ? (u32*)(image + t.atLead) : nullptr, (u64*)(image + t.bytes) };
}

// ---- the fill ----
// A pass's members: entry members[m] of the call's arrays, m < nEnt.  srcs: addresses, read as integers and never followed.
// dsts / caps: the destinations and their capacities, or null (sizes only).  seekIdx: a pack's seek rows, or null.
struct BatchPassEntries { const size_t* members; u32 nEnt; const u8* const* srcs; const size_t* sizes; u8* const* dsts; const size_t* caps; const u32* seekIdx; };
// the destinations' span: [lo, lo + span) holds every member's [dst, dst + cap); without destinations lo = ~0 and span = 0
struct BatchPassSpan { uintptr_t lo; u64 span; };
// Writes from / len / frame per chunk (plan_chunk: the record the device planner computes for the same chunk), entFirst[0 .. nEnt],
// entDst as an offset from the lowest destination, entCap (~0 without destinations) and entSeek into the host image h, whose frame
// and entSeek columns are there iff frameBlocks and seekIdx are.  The chunks are numbered in member order.
inline BatchPassSpan batch_pass_fill(const BatchPassEntries& e, u32 chunkBytes, u32 frameBlocks, const BatchPassCols& h)
{
    uintptr_t lo = ~(uintptr_t)0, hi = 0;
    if (e.dsts) for (u32 m = 0; m < e.nEnt; ++m) {
        const size_t i = e.members[m];
        const uintptr_t d = (uintptr_t)e.dsts[i];
        lo = d < lo ? d : lo; hi = d + e.caps[i] > hi ? d + e.caps[i] : hi;
    }
    u32 ck = 0;
    for (u32 m = 0; m < e.nEnt; ++m) {
        const size_t i = e.members[m];
        const u64 S = e.sizes[i];
        h.entFirst[m] = ck;
        if (e.seekIdx) h.entSeek[m] = e.seekIdx[i];
        h.entDst[m] = e.dsts ? (u64)((uintptr_t)e.dsts[i] - lo) : 0;
        h.entCap[m] = e.dsts ? (u64)e.caps[i] : ~(u64)0;
        if (frameBlocks) {
            // what plan_chunk will hand to chunk_frame_word fits it: the highest block index, min(chunks, frameBlocks) - 1, and the
            // longest frame, the entry's first, of min(S, frameBlocks * chunkBytes) bytes
            assert(frameBlocks <= kFrameWordBlocks || S <= (u64)kFrameWordBlocks * chunkBytes);
            assert((S < (u64)frameBlocks * chunkBytes ? S : (u64)frameBlocks * chunkBytes) < kFrameWordLen);
        }
        u32 k = 0;
        for (u64 o = 0; o < S; o += chunkBytes, ++k, ++ck) {      // (no division: an entry of one chunk is the common one)
            const PlanChunk r = plan_chunk((u64)(uintptr_t)e.srcs[i], S, k, chunkBytes, frameBlocks);
            h.from[ck] = r.from; h.len[ck] = r.len;
            if (frameBlocks) h.frame[ck] = r.frameWord;
        }
    }
    h.entFirst[e.nEnt] = ck;
    return BatchPassSpan{ lo, e.dsts ? (u64)(hi - lo) : 0 };
}

// ---- the tables of the calls enqueued from the device ----
// ZSTDMI_compressBatchAsync behind ZSTDMI_CCtx_prepareBatchAsync, the pass's table for n entries of one chunk each:
// from | entDst | entCap (u64) | len | entFirst[n + 1] | verdict (u32) | the byte an ineligible entry reads
struct AsyncTab { size_t atDst, atCap, atLen, atFirst, atVerdict, atDummy, bytes; };
inline AsyncTab async_tab(u32 n)
{
    AsyncTab t;
    t.atDst = (size_t)n * 8; t.atCap = t.atDst + (size_t)n * 8; t.atLen = t.atCap + (size_t)n * 8; t.atFirst = t.atLen + (size_t)n * 4;
    t.atVerdict = t.atFirst + ((size_t)n + 1) * 4; t.atDummy = (t.atVerdict + (size_t)n * 4 + 7) & ~(size_t)7; t.bytes = t.atDummy + 8;
    return t;
}
// The pass's table of a planned call, laid out once for the prepared limits (nEnt entries, nCh chunks):
// from[nCh] | src | size | dst | cap [nEnt] (u64) | len[nCh] | frame[nCh] | first[nEnt + 1] | verdict[nEnt] (u32) | the idle slots' byte
struct AsyncPlanTab { size_t atSrc, atSize, atDst, atCap, atLen, atFrame, atFirst, atVerdict, atDummy, bytes; };
inline AsyncPlanTab async_plan_tab(u32 nEnt, u32 nCh)
{
    AsyncPlanTab t;
    t.atSrc = (size_t)nCh * 8; t.atSize = t.atSrc + (size_t)nEnt * 8; t.atDst = t.atSize + (size_t)nEnt * 8; t.atCap = t.atDst + (size_t)nEnt * 8;
    t.atLen = t.atCap + (size_t)nEnt * 8; t.atFrame = t.atLen + (size_t)nCh * 4; t.atFirst = t.atFrame + (size_t)nCh * 4;
    t.atVerdict = t.atFirst + ((size_t)nEnt + 1) * 4; t.atDummy = (t.atVerdict + (size_t)nEnt * 4 + 7) & ~(size_t)7; t.bytes = t.atDummy + 8;
    return t;
}
// What a pack adds to either prepare (ZSTDMI_compressPackAsync): the placement's columns for nEnt entries of at most F frames each —
// entAt[nEnt] | state[kPackStateWords] (u64) | entRow[nEnt] | rows[2 * nEnt * F] (u32).
// (PackState: the words of `state`, which the placement kernel leaves for the table kernel and the host)
enum PackState : u32 { kPackStateOk = 0, kPackStateTableAt = 1, kPackStateRows = 2, kPackStateWords = 4 };
struct PackAsyncLayout { size_t atState, atRow, atRows, bytes; };
inline PackAsyncLayout pack_async_tab(u32 nEnt, u32 F)
{
    PackAsyncLayout t;
    t.atState = (size_t)nEnt * 8; t.atRow = t.atState + kPackStateWords * 8; t.atRows = t.atRow + (((size_t)nEnt * 4 + 7) & ~(size_t)7);
    t.bytes = t.atRows + (size_t)nEnt * F * 8 + 8;
    return t;
}

} // namespace zmi
