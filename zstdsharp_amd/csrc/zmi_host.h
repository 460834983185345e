// zmi_host.h — what the host files of libzstd_mi355x.so share (zstd_mi355x.hip, zstd_mi355x_dec.hip, dict_train.hip): the prototypes
// of every launch function the kernel files define (each of those files includes this header, so a signature or a default argument is
// stated once and a definition that drifts from it does not compile or link), error codes as return values, device buffers, the
// stage timer and the small helpers around pointers, devices and worker threads.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <assert.h>
#include <vector>
#include <thread>
#include <new>
#include <type_traits>
#include "zmi_common.h"
#include "zmi_frame.h"
#include "zmi_batch_plan.h"
#include "zmi_batch_pass.h"
#include "zmi_dictset.h"
#include "zmi_cdictset.h"
#include "zmi_cuts.h"
#include "../../include/zstd_mi355x.h"

namespace zmi {
// kernels (lz_fast.hip, huf_enc.hip, seq_enc.hip, frame.hip, decode.hip)
// (an indexed dictionary, DictIndexRef: zmi_cdictset.h)
void launch_dict_index(const u8* content, u32 len, u32* table, u32 log, hipStream_t stream);
void launch_dict_index_dual(const u8* content, u32 len, u32* tableLong, u32* tableShort, u32 log, hipStream_t stream);
u32 dict_index_log(u32 len);        // log2 of the buckets for `len` indexed bytes
u32 dict_index_max();               // the most bytes an index covers (the far candidates' reach)
// What the match finder is launched with.  frames (zmi_frame.h): chunkBytes = 64 KiB minus what lies in LDS in front of a block, rounded
// up to whole 4 KiB tiles — the dictionary's tail (prefix / prefixLen: the bytes every chunk sees as history), or, with frameBlocks > 0
// and no dictionary, up to 64 KiB - chunkBytes of the input in front of the block, as far back as its frame reaches; chunkBytes
// < 64 KiB with neither: independent frames of chunkBytes each (ZSTD_c_windowLog 10 .. 15: a frame is its own window), on the same
// instance with an empty history.  independent: the blocks of a frame share no history (frame_blocks_encode).
// chunkLens (optional): a batch of entries, each staged at a chunk boundary: per chunk its length.
// cand / chain / regionList (null: off): workspace of the region parse, 65536 u16 per chunk (twice with the hash chains of the
// level >= 5 search, hcDepth attempts per position) and 1 + nChunks u32.  claimCtr: a zeroable word for the chunk claims (lz_kernel).
// dix (null: off): an indexed dictionary behind full 64 KiB chunks, each a frame of its own (fast finder, or the dual one where dix has
// its two tables; chunkLens allowed; prefix and frames.table are null, and so are cand, chain and regionList below the chain finder).
// The kernel gets a copy (LzArgs::dix).  dist (the chain finder behind dix; else null): the region parse's second plane, 65536 u32 for each
// of lz_region_kernel's at most 256 workgroups: where a position's candidate lies in the dictionary (ZSTDMI_CCtx_setDictIndexChain).
// slots / chunkSlot (null: off; ZSTDMI_compressBatchCDicts, zmi_cdictset.h): a pass behind two or more dictionaries.  The finder's
// set instance then takes the tail (prefix, prefixLen) or the index (dix) per chunk from slots[chunkSlot[c]], and the frame header's
// dictID bytes with them; of prefix / prefixLen / dix the host states only whether there is one (prefixLen != 0, dix != null).
struct LzLaunch {
    u32 finder;
    const u8* src; u64 srcSize; u32 nChunks;
    Seq* seqs; u8* lits; ChunkMeta* meta;
    const u8* prefix; u32 prefixLen;
    FrameLayout frames; bool independent;
    FrameHeaderSpec header;
    u32 minStrideLog;
    u16* cand; u16* chain; u32* regionList; u32 hcDepth;
    u32* dist;
    u32* claimCtr;
    const u32* chunkLens;
    const DictIndexRef* dix;
    const CDictSlot* slots; const u32* chunkSlot;
    hipStream_t stream; StageHook hook;
};
void launch_lz(const LzLaunch& a);
void launch_lz_probe(const u8* src, u64 srcSize, u64 front, u64 groupBytes, u32 nGroups, u32 tilesPerGroup, u32* out, hipStream_t stream);
// frames: a dictionary's entropy tables (dct) serve the first block of every frame
// dictSlots / chunkSlot (null: off), here and in launch_seq_encode: the stage's set instance, which reads dct — and seq_encode the
// header's dictID and the first repcodes — per chunk from dictSlots[chunkSlot[c]]; the arguments they replace are not read
void launch_huf_build(const u8* lits, ChunkMeta* meta, HufTable* tables, u8* slots, u32 nChunks, u32 rawLiterals, const u8* src, const FrameLayout& frames,
                      hipStream_t stream, StageHook hook, const DictCTables* dct = nullptr, const CDictSlot* dictSlots = nullptr, const u32* chunkSlot = nullptr);
void launch_huf_encode(const u8* lits, const ChunkMeta* meta, const HufTable* tables, u8* slots, u8* dst, const u64* offsets, u64 dstCapacity,
                       u32 nChunks, const u8* src, u32 chunkBytes, hipStream_t stream, bool dictEntropy = false);
// carry (null: off; ZSTDMI_CCtx_setEntropyCarry, zmi_carry.h; multi-block frames without dictionary tables only): seq_encode's carry
// instance walks the pass's nGroups carry groups block by block.  tables: the pass's Huffman tables (a block that reuses an earlier
// block's gets a copy in its own entry, and huf_encode must then be launched with dictEntropy = true, the instance that writes
// literals type 3); leaders: for frames.form == kTable, nGroups + 1 chunk indices (carry_leaders_table), else null; rawLiterals: the
// call compresses no literals
struct SeqCarry { HufTable* tables; const u32* leaders; u32 nGroups, rawLiterals; };
void launch_seq_encode(Seq* seqs, ChunkMeta* meta, u8* slots, u32 nChunks, u32 strategy, const FrameHeaderSpec& header, u32 resolveReps,
                       const u32* initReps, const FrameLayout& frames, hipStream_t stream, const DictCTables* dct = nullptr,
                       const CDictSlot* dictSlots = nullptr, const u32* chunkSlot = nullptr, const SeqCarry* carry = nullptr);
// pinned (null: none): kPassPinWords u64 of the context's pinned block: the pass's total and the offsets of up to kPassMarks marked
// chunks (indices into the pass), stored there by the scan itself for the host to read behind its wait
constexpr u32 kPassMarks = 16, kPassPinWords = 1 + kPassMarks;
struct PassMarks { u32 n = 0; u32 chunk[kPassMarks] = {}; };
void launch_scan_sizes(const ChunkMeta* meta, u32 nChunks, u64* offsets, u64* total, hipStream_t stream, u64* pinned = nullptr, const PassMarks& marks = PassMarks());
void launch_gather(const u8* src, u64 srcSize, const u8* slots, const ChunkMeta* meta, const u64* offsets, u8* dst, u64 dstCapacity,
                   u32 nChunks, u32 chunkBytes, hipStream_t stream);
void launch_xxh64(const u8* src, ChunkMeta* meta, u32 nChunks, const FrameLayout& frames, hipStream_t stream, const u32* chunkLens = nullptr);
void launch_batch_stage(const u64* from, const u32* len, u8* stage, u32 nChunks, u32 chunkBytes, hipStream_t stream);
void launch_batch_place(const ChunkMeta* meta, u32 nEntries, const u32* entFirst, const u64* entDst, const u64* entCap, u64 span, u64* offsets, u64* entSize,
                        hipStream_t stream);
// a batch whose descriptors lie in HBM (ZSTDMI_compressBatchAsync, frame.hip).  plan: the caller's four arrays into the pass's table in the
// layout the stages read (one chunk per entry), entDst as an offset from kAsyncBase, and a verdict per entry (AsyncVerdict); an entry
// that runs no pass becomes one byte read from `dummy`.  place: sizes and statuses straight into the caller's column, the empty frame
// (by value) for entries of size 0, the offset kAsyncSpan for every entry that writes nothing.
// (kAsyncBase, kAsyncSpan, AsyncVerdict: zmi_batch_plan.h)
struct AsyncEmptyFrame { u8 bytes[16]; u32 len; };
void launch_batch_plan(const void* const* srcs, const size_t* sizes, void* const* dsts, const size_t* caps, u32 n, u64 bound, u32 emptyLen, const u8* dummy,
                       u64* from, u64* entDst, u64* entCap, u32* len, u32* entFirst, u32* verdict, hipStream_t stream);
void launch_batch_place_async(const ChunkMeta* meta, u32 n, const u64* entDst, const u64* entCap, const u32* verdict, AsyncEmptyFrame empty,
                              u64* offsets, size_t* dstSizes, hipStream_t stream);
// entries of several chunks (ZSTDMI_CCtx_prepareBatchAsyncLimits; the arithmetic is zmi_batch_plan.h's).  The entry table: what the
// plan keeps per entry, and the grid's chunk slots.  plan_entries: verdicts (workSpace_tooSmall by the chunk limit included), the
// entries' first chunks entFirst[0 .. n] by a scan, the caller's arrays copied.  plan_chunks: from / len / frame (null: every chunk a
// frame of its own) for the nLaunch chunk slots, those at or beyond entFirst[n] idle.  place: each entry's frames one behind the other.
struct AsyncEntryTab { u64* src; u64* size; u64* dst; u64* cap; u32* first; u32* verdict; };
void launch_batch_plan_entries(const void* const* srcs, const size_t* sizes, void* const* dsts, const size_t* caps, u32 n, u64 bound, u32 emptyLen,
                               u32 chunkBytes, u32 maxChunks, const AsyncEntryTab& tab, hipStream_t stream);
void launch_batch_plan_chunks(const AsyncEntryTab& tab, u32 n, u32 nLaunch, u32 chunkBytes, u32 frameBlocks, const u8* dummy, u64* from, u32* len, u32* frame,
                              hipStream_t stream);
void launch_batch_place_async_frames(const ChunkMeta* meta, u32 n, u32 nLaunch, const AsyncEntryTab& tab, AsyncEmptyFrame empty, u64* offsets, size_t* dstSizes,
                                     hipStream_t stream);
// a pack of such entries (ZSTDMI_compressPackAsync): one destination, densely packed, one seek table behind the frames.  plan_entries
// without the dst and cap columns (pack_verdict); the placement decides on the device whether frames plus table fit `cap` and writes
// every chunk's final address into offsets (kAsyncSpan for all of them after a failure), the empty frames, the rows, *packSize and
// entryEnds (may be null); the table kernel's grid covers maxRows rows and takes the count and the place from the state.
// PackAsyncTab: context memory the prepare sized: entAt / entRow per entry, rows[2 * maxRows], state[kPackStateWords] (PackState and
// the layout: zmi_batch_pass.h).
struct PackAsyncTab { u64* entAt; u32* entRow; u32* rows; u64* state; };
void launch_pack_plan_entries(const void* const* srcs, const size_t* sizes, u32 n, u64 bound, u32 chunkBytes, u32 maxChunks, const AsyncEntryTab& tab, hipStream_t stream);
void launch_pack_place_async(const ChunkMeta* meta, u32 n, u32 nLaunch, const AsyncEntryTab& tab, const u32* len, u32 frameBlocks, AsyncEmptyFrame empty, u8* dst,
                             u64 cap, const PackAsyncTab& pk, u64* offsets, size_t* packSize, size_t* entryEnds, hipStream_t stream);
void launch_pack_table_async(const PackAsyncTab& pk, u64 maxRows, u8* dst, hipStream_t stream);
void launch_seek_entries(const u64* offsets, const u64* total, u32 nChunks, const FrameLayout& frames, u32* entries, hipStream_t stream);
void launch_seek_table(const u32* entries, u32 n, u8* dst, hipStream_t stream);
// a pack (ZSTDMI_compressPack, frame.hip): a batched pass's seek-table rows per entry (entSeek[e] = the row of entry e's first frame, rows
// at or beyond cap are dropped); the entries' places in the stream (at = exclusive sums of size); their bytes from the arena's slots
// (slot[nEntries + 1]) to dst + at, `longest` = the largest size, nothing at or beyond dst + room
void launch_pack_entries(const ChunkMeta* meta, u32 nEntries, const u32* entFirst, const u32* chunkLens, u32 frameBlocks, const u32* entSeek, u32* entries,
                         u32 cap, hipStream_t stream);
void launch_pack_place(const u64* size, u32 nEntries, u64* at, hipStream_t stream);
void launch_pack_gather(const u8* arena, const u64* slot, const u64* size, const u64* at, u32 nEntries, u64 longest, u8* dst, u64 room, hipStream_t stream);
// long-distance matching (ldm.hip)
size_t ldm_small_bytes(u64 n);
size_t ldm_big_bytes(u64 nSplits);
void launch_ldm_count(const u8* src, u64 n, u64 frameSpan, const LdmLaunch& p, u8* small, hipStream_t stream, const LdmPrefix& pfx);
u32* ldm_total_word(u8* small, u64 n);
// where a pass's splits and their matches lie in `big` afterwards (ZSTDMI_debugLdmPass)
struct LdmRecord { const u32* splitPos = nullptr; const u32* mStart = nullptr; const u32* mLen = nullptr; const u32* mOff = nullptr; u32 nSplits = 0; };
// merge false (ZSTDMI_debugLdmSkipMerge): the stage ends behind ldm_match and the finder's sequence store stays as it is
LdmRecord launch_ldm_rest(const u8* src, u64 n, u32 nChunks, u32 chunkBytes, u64 frameSpan, const LdmLaunch& p, u32 nSplits, u8* small, u8* big,
                          Seq* seqs, u8* lits, ChunkMeta* meta, hipStream_t stream, StageHook hook, const LdmPrefix& pfx, bool merge = true);
// content-defined cuts (content_cuts.hip; the rule: zmi_cuts.h).  small: cut_small_bytes(n) bytes; the count leaves the candidates'
// total in *cut_total_word, the emit writes that many ends in position order, the select 1 + cap words: the pieces, then their ends
size_t cut_small_bytes(u64 n);
u32* cut_total_word(u8* small, u64 n);
void launch_cut_count(const u8* src, u64 n, u32 bits, u8* small, hipStream_t stream);
void launch_cut_emit(const u8* src, u64 n, u32 bits, u8* small, u32* cand, hipStream_t stream);
void launch_cut_select(const u32* cand, u32 nCand, u64 n, const CutRule& rule, u32* out, u32 cap, hipStream_t stream);
// cuts and digests enqueued from the device (content_cuts_async.hip; the selection: zmi_cut_rank.h).  One workspace the
// prepare sizes (cuts_async_layout: include/zstd_mi355x.h states the arithmetic): the count's tiles, the list with room for maxCand
// candidates, per node (maxCand + 2) the successor, two pointer planes, the forced count and the mark, the scan's block sums and bases,
// 256 bytes of state (word 0: the pieces, word 1: the list passed its room), the ends (1 + maxPieces words) and the digests.
constexpr u64 kCutsAsyncMaxCand = 0xFFFFFFF0ull;     // the most candidates a prepare makes room for (node indices are words)
struct CutsAsyncLayout { size_t atSmall, atList, atSucc, atJumpA, atJumpB, atForced, atMark, atSum, atBase, atState, atEnds, atDigests, bytes; };
CutsAsyncLayout cuts_async_layout(u64 bound, u64 maxCand, u64 maxPieces, u32 digestSize);
struct CutRankWs { u32* succ; u32* jumpA; u32* jumpB; u32* forced; u8* mark; u32* blockSum; u32* blockBase; u32* state; };
inline CutRankWs cut_rank_ws(u8* p, const CutsAsyncLayout& L)
{
    return CutRankWs{ (u32*)(p + L.atSucc), (u32*)(p + L.atJumpA), (u32*)(p + L.atJumpB), (u32*)(p + L.atForced), p + L.atMark, (u32*)(p + L.atSum), (u32*)(p + L.atBase), (u32*)(p + L.atState) };
}
// emit: launch_cut_emit that never stores at or beyond `room` and does nothing when the count passed it.  rank: the selection over the
// list of *total candidates -> ends[0] = the pieces, ends[1 ..] their ends (at most cap), state as above.  finish: the caller's arrays
// (all device memory) from the ends, the state and the workspace's digests; maxPieces: the most pieces n allows (the grid)
void launch_cut_emit_bounded(const u8* src, u64 n, u32 bits, u8* small, u32* cand, u32 room, hipStream_t stream);
void launch_cut_rank(const u32* cand, const u32* total, u32 room, u64 n, const CutRule& rule, const CutRankWs& ws, u32* ends, u32 cap, hipStream_t stream);
struct CutsFinishArgs {
    const u32* ends; const u32* state; u32 endsCap; const u8* src; u64 n, maxPieces;
    size_t* sizes; const void** srcs; u64 capacity;
    const u8* digestsWs; u8* digests; u64 digestsCapacity; u32 digestSize;
    size_t* nPieces; size_t* status;
};
void launch_cuts_finish(const CutsFinishArgs& a, hipStream_t stream);
// piece digests (digest.hip; the functions: zmi_digest.h).  Where the pieces of [src, src + srcSize) lie: offs, n + 1 offsets from src
// (device memory, ascending, the last at most srcSize), or — ends not null — launch_cut_select's output, of which the kernel takes the
// count and the ends; n is then the most pieces there can be (the select's cap).  out: n digests side by side (device memory).
struct DigestPieces { const u64* offs; const u32* ends; u64 n; u64 srcSize; };
void launch_digest(unsigned kind, const u8* src, const DigestPieces& tab, u8* out, hipStream_t stream);
// decoder (decode_walk.hip, decode_lit.hip, decode_seq.hip, decode_origin.hip)
// The dictionary of a call as the stage launchers take it (the host's decode_dict, zstd_mi355x_dec.hip): formatted or raw content, the
// whole dictionary and its parsed header (formatted only), the content that is history in front of every frame — a caller may put a
// prefix or a stream's history there —, the dictID, and seqTabs: a DDict's ready-made sequence tables (null for a loaded dictionary).
// slots (null: off): the slot table of the context's DDict set (ZSTD_d_refMultipleDDicts, zmi_dictset.h), nSet records sorted by dictID
// and the current DDict's behind them.  A launcher then starts the stage's set instance, which reads every dictionary argument per
// frame through FrameDesc::dictSlot and gets nulls for the single-dictionary arguments; the other fields describe the current DDict.
struct DecodeDict { bool fmt; const u8* dictFull; const DictInfo* dinfo; const u8* dictContent; u32 dictContentSize, dictID; const u32* seqTabs;
                    const DictSlot* slots; u32 nSet; };
// Run-time flags -> the template arguments of a stage's one entry point (zmi_decode.h): with_flags(f, a, b, ...) calls
// f(std::bool_constant<a>(), std::bool_constant<b>(), ...), and f — a generic lambda, [&](auto set, auto dev) — names the instance as
// kernel<set(), dev()>.  f is instantiated for every combination of the flags: one the family does not have is excluded inside f with
// if constexpr, so that its instance is never compiled.
template <class F> inline void with_flags(F&& f) { f(); }
template <class F, class... Bs> inline void with_flags(F&& f, bool b, Bs... rest)
{
    if (b) with_flags([&](auto... cs) { f(std::true_type(), cs...); }, rest...);
    else   with_flags([&](auto... cs) { f(std::false_type(), cs...); }, rest...);
}
// the status words (kSt*, zmi_common.h) at the start of a call: error key "none" (all ones), everything else zero; and their copy into
// the context's pinned block (PinBuf below), which the host reads behind its wait
void launch_status_reset(u32* status, hipStream_t stream);
void launch_status_mirror(const u32* status, u32* pinned, hipStream_t stream);
size_t decode_walk_workspace_bytes(u64 srcSize);
// pinned (null: none): the context's pinned copy of the status words, which walk_link fills with the words it writes
void launch_frame_walk_count(const u8* src, u64 srcSize, u32 maxFrames, u32* status, u8* walkWs, hipStream_t stream, u32* pinned = nullptr);
void launch_frame_walk_emit(const u8* src, u64 srcSize, FrameDesc* frames, BlockDesc* blocks, u8* walkWs, hipStream_t stream);
void launch_frame_walk_serial(const u8* src, u64 srcSize, FrameDesc* frames, BlockDesc* blocks, u32 maxFrames, u32* status, const DecodeDict& dd, u32 emit, hipStream_t stream);
// open: ZSTDMI_DCtx_setBatchUnsized; caps: batch_scan's instance that holds the entries to the limits in the status words
void launch_batch_walk_count(const u8* src, const BatchEntryIn* in, BatchEntryOut* out, u32 nEntries, const DecodeDict& dd, u64 aloneAbove, u32* status, hipStream_t stream,
                             bool open = false, bool caps = false);
// rooms (not null: the open instance): one u64 per frame, the room its literals have in the scratch
void launch_batch_walk_emit(const u8* src, const BatchEntryIn* in, const BatchEntryOut* out, u32 nEntries, FrameDesc* frames, BlockDesc* blocks, hipStream_t stream,
                            const DecodeDict& dd, u64* rooms = nullptr);
void launch_batch_rescan(const BatchEntryIn* in, BatchEntryOut* out, u32 nEntries, FrameDesc* frames, hipStream_t stream);
void launch_batch_fold(BatchEntryOut* out, u32 nEntries, const u64* keys, hipStream_t stream);
// A batch whose descriptors lie in HBM (ZSTDMI_decompressBatchAsync).  The host knows the number of entries and the
// caller's limits, never the call's frames, blocks or sequences: those stay in the status words.  plan / init / finish stand in for the
// host's loops over the entries and its small copies (decode_walk.hip); every launch_*_d below starts a stage's open instances that
// take their count from the status words, over a grid sized from the limit (capFrames, capBlocks), never on a second stream.
// batch_walk_count / _emit, batch_rescan and batch_fold run one lane or wave per ENTRY and serve as they are.
struct BatchLimitsD { u32 frames, blocks; u64 content, sequences; };
void launch_batch_plan_d(const void* const* srcs, const size_t* sizes, void* const* dsts, const size_t* caps, u32 n, u64 bound, BatchEntryIn* in, u32* verdict, hipStream_t stream);
void launch_batch_init_d(u32* status, const u64* blockKeys, const u64* rooms, u64 dumpOff, const BatchLimitsD& lim, hipStream_t stream);
void launch_batch_finish_d(const BatchEntryOut* out, const u32* verdict, u32 n, size_t* dstSizes, hipStream_t stream);
void launch_block_prepass_d(const u8* src, FrameDesc* frames, BlockDesc* blocks, u32 capFrames, u32 capBlocks, const DecodeDict& dd, u32* status, hipStream_t stream);
void launch_seq_decode_d(const u8* src, const FrameDesc* frames, BlockDesc* blocks, u32 capBlocks, SeqRec* recs, u32* status, const DecodeDict& dd, hipStream_t stream);
void launch_block_offsets_d(FrameDesc* frames, BlockDesc* blocks, u32 capFrames, const DecodeDict& dd, u32* status, hipStream_t stream);
void launch_decode_literals_d(const u8* src, u8* out, u8* scratch, const FrameDesc* frames, const BlockDesc* blocks, u32 capBlocks, u32* status,
                              u8* slowFlags, u32 mode, const DecodeDict& dd, hipStream_t stream);
void launch_place_literals_d(const u8* src, u8* out, const u8* scratch, const FrameDesc* frames, const BlockDesc* blocks, u32 capBlocks,
                             const SeqRec* recs, const u32* status, hipStream_t stream);
void launch_exec_matches_d(const u8* src, u8* out, const FrameDesc* frames, const BlockDesc* blocks, u32 capFrames, const SeqRec* recs, u32* status,
                           const DecodeDict& dd, hipStream_t stream, int wide);
void launch_seek_select(const u8* tab, u64 tableBytes, u32 n, u32 stride, u64 srcSize, u64 offset, u64 length, u64* sum, hipStream_t stream);
void launch_seek_emit(const u8* tab, u32 stride, u32 first, u32 nSel, u64 dFirst, u64 offset, u64 dstBias, u64 edgeBias, u64 slot1, u32 cutFirst, u32 cutLast,
                      BatchEntryIn* out, hipStream_t stream);
void launch_range_check(const BatchEntryIn* in, const BatchEntryOut* out, u32 nEntries, u64* sum, hipStream_t stream);
void launch_range_clip(u8* dst, const u8* edge, ClipJob j0, ClipJob j1, hipStream_t stream);
// many ranges of a seekable stream (decode_ranges.hip)
size_t ranges_ws_bytes(u32 n);
RangesWs ranges_ws(u8* p, u32 n);
void launch_seek_index(const u8* tab, u64 tableBytes, u32 n, u32 stride, u64 srcSize, const RangesWs& ws, hipStream_t stream);
void launch_ranges_select(const RangeIn* in, RangeRec* recs, u32 nRanges, u32 n, const RangesWs& ws, hipStream_t stream);
void launch_ranges_plan(const u8* tab, u32 n, u32 stride, u32 srcDev, const RangesWs& ws, BatchEntryIn* out, hipStream_t stream);
void launch_ranges_alone(const BatchEntryOut* out, u32 nEntries, const RangesWs& ws, hipStream_t stream);
void launch_ranges_gather(const RangeIn* in, const RangeRec* recs, u64* res, u32 nRanges, u32 nSlices, const RangesWs& ws, const BatchEntryOut* out,
                          const u8* arena, hipStream_t stream);
// ranges enqueued from the device over a prepared index (ZSTDMI_decompressRangesAsync)
void launch_ranges_select_d(const unsigned long long* offsets, const size_t* lengths, void* const* dsts, const size_t* caps, u32 nRanges, u64 maxRangeBytes,
                            RangeIn* in, RangeRec* recs, u32 n, const RangesWs& ws, hipStream_t stream);
void launch_ranges_plan_d(const u8* tab, u32 n, u32 stride, const RangesWs& ws, u64 streamOff, u64 arenaOff, u32 maxFrames, u64 maxContent, u64 aloneAbove,
                          u32 nRows, BatchEntryIn* rows, BatchEntryOut* out, hipStream_t stream);
void launch_seq_stats(const Seq* seqs, const u8* lits, const ChunkMeta* meta, u32 nChunks, const u8* src, u32 chunkBytes, u32* stats, hipStream_t stream);
void launch_dict_parse(const u8* dict, u32 dictSize, DictInfo* out, hipStream_t stream);
void launch_dict_ctables(const u8* dict, u32 dictSize, const DictInfo* info, DictCTables* out, hipStream_t stream);
// seqPlane: nBlocks u32 (16-byte aligned, room for a multiple of four), what block_parse and block_link leave for seq_scan to sum;
// pinned (null: none): the context's pinned copy of the status words, which seq_scan fills as the last kernel of the pre-pass
void launch_block_prepass(const u8* src, FrameDesc* frames, BlockDesc* blocks, u32 nFrames, u32 nBlocks, const DecodeDict& dd, u32 earlyLiterals, u32* status, hipStream_t stream,
                          u32* seqPlane, u32* pinned, u32 phantoms = 0, bool open = false);     // phantoms, open: decode_walk.hip block_link_body
// (dd.seqTabs not null: the kernel's instance that copies a DDict's ready-made tables where a block repeats the dictionary's)
// far (here, in launch_exec_matches and in launch_origin_init; null: none): the far plane of a call with a far-capable frame, one u32 per
// sequence record (kRecFar, zmi_common.h); the launcher then starts the stage's far instance
void launch_seq_decode(const u8* src, const FrameDesc* frames, BlockDesc* blocks, u32 nBlocks, SeqRec* recs, u32* status, const DecodeDict& dd, hipStream_t stream,
                       u32* far = nullptr);
// A formatted dictionary's three sequence decoding tables, built once (ZSTD_createDDict): words [0, 1280) are the image seq_decode_kernel
// holds per block in LDS (LL at 0, ML at 512, OF at 1024), words kDictTabLogs + 0 / 1 / 2 the LL / OF / ML table logs (all ones: corrupt)
constexpr u32 kDictTabLogs = 1280, kDictTabWords = 1284;
void launch_dict_seq_tables(const u8* dictFull, const DictInfo* di, u32* tabs, hipStream_t stream);
// reps: the repcodes a frame starts from (dd.dinfo, or a segmented stream's carried triple)
// sizePlane (null: no rescan; never with open): a call with frames without a content size — nFrames u64 (16-byte aligned, room for a multiple
// of four) that block_offsets fills with the frames' regenerated sizes and frame_rescan, launched behind it, sums into their places
void launch_block_offsets(FrameDesc* frames, BlockDesc* blocks, u32 nFrames, const DecodeDict& dd, const DictInfo* reps, u64* sizePlane, u64 dstCapacity, u32* status, hipStream_t stream,
                          bool open = false);
void launch_decode_literals(const u8* src, u8* out, u8* scratch, const FrameDesc* frames, const BlockDesc* blocks, u32 nBlocks, u32* status,
                            u8* slowFlags, u32 mode, const DecodeDict& dd, hipStream_t stream, StageHook hook);
void launch_place_literals(const u8* src, u8* out, const u8* scratch, const FrameDesc* frames, const BlockDesc* blocks, u32 nBlocks,
                           const SeqRec* recs, const u32* status, hipStream_t stream);
// a segmented stream's carried state (decode_stream.hip)
void launch_stream_carry(const BlockDesc* blocks, u32 nBlocks, DictInfo* reps, hipStream_t stream);
// XXH64 with carried state (frame.hip): the decoder's segmented streams and the compressor's single frame across passes and batches.
// xxh_carry_reset: the state of an empty input (host).  launch_xxh_carry_file: the finished hash into the chunk that carries the checksum.
void launch_stream_xxh(XxhCarry* st, const u8* data, u64 n, u32 final, hipStream_t stream);
void launch_xxh_carry_file(const XxhCarry* st, ChunkMeta* chunk, hipStream_t stream);
inline void xxh_carry_reset(XxhCarry* x)
{
    const u64 P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL;
    memset(x, 0, sizeof *x);
    x->acc[0] = P1 + P2; x->acc[1] = P2; x->acc[2] = 0; x->acc[3] = 0 - P1;
}
void launch_exec_matches(const u8* src, u8* out, const FrameDesc* frames, const BlockDesc* blocks, u32 nFrames, const SeqRec* recs, u32* status,
                         const DecodeDict& dd, hipStream_t stream, int wide, const u32* far = nullptr);
void launch_origin_select(FrameDesc* frames, u32 nFrames, u64 minBytes, u32* list, u32 listCap, u64 originCap, u32* status, hipStream_t stream);
void launch_origin_init(const FrameDesc* frames, const BlockDesc* blocks, const u32* list, u32 listCap, u64 maxFrameBytes, const SeqRec* recs, u32* status,
                        u32* origin, const DecodeDict& dd, hipStream_t stream, const u32* far = nullptr);
void launch_origin_jump(const FrameDesc* frames, const u32* list, u32 listCap, u64 maxFrameBytes, u32* status, u32* origin, u32* done, u32 r0, u32 r1, hipStream_t stream);
void launch_origin_gather(const FrameDesc* frames, const u32* list, u32 listCap, u64 maxFrameBytes, const u32* status, const u32* origin, u8* out, const DecodeDict& dd, hipStream_t stream);
// a batch of samples through the compressor, sizes (and sequence statistics) only (zstd_mi355x.hip; the dictionary trainer's inner loop)
size_t compress_samples(ZSTD_CCtx* c, const u8* src, const u64* offs, const size_t* sizes, size_t n, size_t* outSizes, u32* stats);
}

using namespace zmi;

#define ZERR(code) ((size_t)0 - (size_t)(code))
static inline bool isErr(size_t c) { return c > ZERR(kErrMaxCode); }
// No C++ exception may cross the C ABI (the caller is P/Invoke): host-side container growth is the only thing that throws here.
// Host-side tallies of one context (ZSTDMI_debugHostWaits / ZSTDMI_debugDeviceAllocs, and the decoder's with a D behind the name): blocking
// waits its host code made and growths of its device buffers.  Its buffers name it (DevBuf::owner); a wait is counted for the tally this
// thread's ABI call bound (tl_waits: set by cctx_bind / dctx_bind inside guarded(), which puts the caller's back), so that stream_wait and
// dev_read count without an argument.
// beforeFree: what must happen before any of its buffers is freed (cctx_async_drain / dctx_async_drain: the wait behind an enqueued batch)
struct HostTally { long long waits = 0, allocs = 0; void (*beforeFree)(void*) = nullptr; void* self = nullptr; };
static thread_local long long* tl_waits = nullptr;
static thread_local bool tl_guarded = false;
static inline void count_wait() { if (tl_waits) ++*tl_waits; }
template <class F> static size_t guarded(F f)
{
    struct Keep { long long* was = tl_waits; bool in = tl_guarded; Keep() { tl_guarded = true; } ~Keep() { tl_waits = was; tl_guarded = in; } } keep;
    try { return f(); }
    catch (const std::bad_alloc&) { return ZERR(kErrMemoryAllocation); }
    catch (...) { return ZERR(kErrGeneric); }
}

namespace {

constexpr int kMaxStages = 24;

struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    HostTally* owner = nullptr;     // (a context's buffers: see HostTally)
    void drop() { if (!p) return; if (owner && owner->beforeFree) owner->beforeFree(owner->self); (void)hipFree(p); p = nullptr; cap = 0; }
    bool ensure(size_t n)
    {
        if (n <= cap) return true;
        if (owner) owner->allocs++;
        drop();
        size_t want = n + (n >> 3) + 4096;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; if (hipMalloc(&p, n) != hipSuccess) { p = nullptr; return false; } want = n; }
        cap = want; return true;
    }
    void release() { drop(); }
};

// A context's small block of pinned, device-visible host memory: what the host wants of a call — the decoder's status words, the
// compressor's per-pass total and mark offsets — is stored there by a kernel of the call's stream (ordinary vector stores) and read
// behind the call's stream_wait, so that no copy from or to pageable memory, with the staging kernel and the wait of its own that the
// runtime puts behind one, stands in a call.  Made once, at the context's first call that reads it (counted as an allocation), never grown.
struct PinBuf {
    void* p = nullptr;
    HostTally* owner = nullptr;
    bool ensure(size_t n)
    {
        if (p) return true;
        if (owner) owner->allocs++;
        if (hipHostMalloc(&p, n, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
        memset(p, 0, n);
        return true;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; }
};

struct StageTimer {
    bool enabled = false;
    hipEvent_t ev[kMaxStages + 1] = {};
    const char* names[kMaxStages] = {};
    float ms[kMaxStages] = {};
    int n = 0; bool created = false; hipStream_t stream = nullptr;
    static void hook_fn(void* self, const char* name) { StageTimer* t = (StageTimer*)self; t->mark(name, t->stream); }
    StageHook hook() { StageHook h; if (enabled) { h.fn = hook_fn; h.self = this; } return h; }
    void begin(hipStream_t s) { n = 0; stream = s; if (!enabled) return; if (!created) { for (auto& e : ev) (void)hipEventCreate(&e); created = true; } (void)hipEventRecord(ev[0], s); }
    void mark(const char* name, hipStream_t s) { if (!enabled || n >= kMaxStages) return; names[n] = name; (void)hipEventRecord(ev[n + 1], s); n++; }
    void finish() { if (!enabled) return; for (int i = 0; i < n; i++) { float t = 0; (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]); ms[i] = t; } }
    void destroy() { if (created) for (auto& e : ev) (void)hipEventDestroy(e); created = false; }
};

bool is_device_ptr(const void* p)
{
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// a zstd-format dictionary starts with the magic 0xEC30A437 (ZSTD_MAGIC_DICTIONARY); anything else is raw content
bool is_formatted_dictionary(const u8* p, size_t n)
{
    return n >= 8 && ((u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24)) == 0xEC30A437u;
}

// devices the kernels can run on: the leading run of gfx950 agents (device ordinals stay HIP's, so a context's device index means
// the same thing to the caller's runtime; the code objects in this library are gfx950 only)
int device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (; ok < n; ++ok) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, ok) != hipSuccess) { (void)hipGetLastError(); break; }
        if (strncmp(p.gcnArchName, "gfx950", 6) != 0) break;
    }
    return ok;
}

} // namespace

// run f(0 .. n - 1), one host thread each (f(0) on the caller's): a device worker's calls block on its own stream
// (nothing may leave a thread as an exception: -> false, and the caller reports memory_allocation)
template <class F> static bool run_on_workers(size_t n, F f)
{
    std::vector<std::thread> th;
    std::vector<u8> bad(n, 0);
    th.reserve(n);
    auto one = [&f, &bad](size_t i) { try { f(i); } catch (...) { bad[i] = 1; } };
    bool ok = true;
    for (size_t i = 1; i < n; ++i) { try { th.emplace_back(one, i); } catch (...) { ok = false; break; } }
    if (ok) one(0);
    for (auto& t : th) t.join();
    for (size_t i = 0; i < n; ++i) ok = ok && !bad[i];
    return ok;
}

// a copy between any two places (host or device, this device or a peer), enqueued on s
static size_t copy_any(void* dst, const void* src, size_t n, hipStream_t s)
{
    if (!n) return 0;
    if (hipMemcpyAsync(dst, src, n, hipMemcpyDefault, s) != hipSuccess) { (void)hipGetLastError(); return ZERR(kErrGeneric); }
    return 0;
}

// wait for everything enqueued on s -> 0 or generic (the failed wait's error is taken off the runtime's record)
static size_t stream_wait(hipStream_t s)
{
    count_wait();
    if (hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); return ZERR(kErrGeneric); }
    return 0;
}
// device memory read back to the host: the copy, enqueued on s, and the wait for it
static size_t dev_read(void* host, const void* dev, size_t bytes, hipStream_t s)
{
    if (hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return ZERR(kErrGeneric);
    return stream_wait(s);
}

// ---- what ZSTD_CCtx_s and ZSTD_DCtx_s do alike (device, deviceOk, ownStream, stream, workers, dictGen) ----
// make the context's device the current one; the first time, check that it is there and create the context's stream
template <class Ctx> static size_t ctx_bind(Ctx* c)
{
    if (!c) return ZERR(kErrGeneric);
    if (!c->deviceOk) {
        if (device_count() <= c->device) return ZERR(kErrInitMissing);       // no gfx950 device: fail loudly, never fall back
        if (hipSetDevice(c->device) != hipSuccess) return ZERR(kErrInitMissing);
        if (!c->ownStream && hipStreamCreateWithFlags(&c->ownStream, hipStreamNonBlocking) != hipSuccess) return ZERR(kErrMemoryAllocation);
        if (!c->stream) c->stream = c->ownStream;
        c->deviceOk = true;
    } else if (hipSetDevice(c->device) != hipSuccess) return ZERR(kErrInitMissing);
    return 0;
}
template <class Ctx> static size_t ctx_set_device(Ctx* c, int device) { if (!c) return ZERR(kErrGeneric); if (c->deviceOk && device != c->device) return ZERR(kErrStageWrong); c->device = device; return 0; }
template <class Ctx> static size_t ctx_set_stream(Ctx* c, void* st, size_t (*bind)(Ctx*)) { size_t e = bind(c); if (isErr(e)) return e; c->stream = st ? (hipStream_t)st : c->ownStream; return 0; }
// devices: one worker per entry (an ordinal may repeat: several workers share that device); n <= 1 = back to the context's own device
template <class Ctx> static size_t ctx_set_devices(Ctx* c, const int* devices, int n, Ctx* (*create)(void), size_t (*release)(Ctx*))
{
    if (!c || n < 0 || n > 64 || (n && !devices)) return ZERR(kErrParameterOutOfBound);
    for (int i = 0; i < n; ++i) if (devices[i] < 0 || devices[i] >= device_count()) return ZERR(kErrInitMissing);
    for (Ctx* w : c->workers) (void)release(w);
    c->workers.clear();
    if (n <= 1) { if (n == 1) return ctx_set_device(c, devices[0]); return 0; }
    for (int i = 0; i < n; ++i) {
        Ctx* w = create();
        if (!w) return ZERR(kErrMemoryAllocation);
        w->device = devices[i]; w->dictGen = ~(u64)0;
        c->workers.push_back(w);
    }
    return 0;
}
