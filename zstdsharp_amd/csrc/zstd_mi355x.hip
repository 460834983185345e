// zstd_mi355x.hip — the compressor's host side of libzstd_mi355x.so: the compression context, parameters, HBM workspaces, the launch
// sequences of the compress pipeline, the ZSTD_compressStream2 adapter, device workers, and the library's error names and version.
// The decoder's host side is zstd_mi355x_dec.hip; what both share is zmi_host.h.  The C ABI is declared in include/zstd_mi355x.h.
//
// There is no CPU codec in this library: without a usable gfx950 device every compress/decompress call returns
// ZSTD_error_init_missing, loudly.
#include "zmi_cparams.h"
#include "zmi_host.h"
#include "zmi_carry.h"
#include "zmi_digest.h"
#include <memory>
#include <unordered_map>

// ======================================================================================================
// A dictionary as the compressor holds it, on the host and on one device: the fields a context fills from ZSTD_CCtx_loadDictionary and
// cctx_sync_dictionary (described at ZSTD_CCtx_s::own below), or a ZSTD_CDict fills once, whole, at its creation.
struct DictDigest {
    std::vector<u8> dictHost, dictFull, dictWide;
    DevBuf dict, dictFullDev, dictInfoDev, dictCTabDev, dictWideDev, dictIdxDev;
    const u8* dictIdxEnd = nullptr; u32 dictIdxLen = 0, dictIdxLog = 0; bool dictIdxDual = false;
    DictInfo info = {};
    bool dictFormatted = false;
    void release() { dict.release(); dictFullDev.release(); dictInfoDev.release(); dictCTabDev.release(); dictWideDev.release(); dictIdxDev.release(); }
    size_t bytes() const { return dictHost.capacity() + dictFull.capacity() + dictWide.capacity() + dict.cap + dictFullDev.cap + dictInfoDev.cap + dictCTabDev.cap + dictWideDev.cap + dictIdxDev.cap; }
};
// ZSTD_createCDict: a digest built whole on `device` at creation — the staged tail, the content with its index (all three tables), and
// for a formatted dictionary DictInfo and the DictCTables — and never written again: any number of contexts and threads read it without
// a lock.  Its host fields are what it keeps of the caller's bytes: a context that cannot share the device copies makes a private
// upload from them (cctx_adopt_cdict).
struct ZSTD_CDict_s { DictDigest dg; int level = 3; int device = 0; };

struct ZSTD_CCtx_s {
    int level = 3;              // ZSTD_CLEVEL_DEFAULT
    int checksumFlag = 0, contentSizeFlag = 1, dictIDFlag = 1;
    int windowLog = 0, hashLog = 0, chainLog = 0, searchLog = 0, minMatch = 0, targetLength = 0, strategy = 0;
    int ldm = 0, ldmHashLog = 0, ldmMinMatch = 0, ldmBucketSizeLog = 0, ldmHashRateLog = 0;     // ZSTD_c_enableLongDistanceMatching .. (0 = auto / from the window)
    int device = 0; bool deviceOk = false;
    hipStream_t ownStream = nullptr, stream = nullptr;
    DevBuf seqs, lits, meta, tables, slots, offsets, total, cand, probe, stageSrc, stageDst;
    PinBuf pin;                 // what the host reads of a pass: its total and mark offsets (compress_range; launch_scan_sizes)
    DevBuf ldmSmall, ldmBig;    // long-distance matching's workspace (allocated by the first call that runs it)
    LdmRecord ldmRec; u32 ldmRecBase = 0, ldmRecVlo = 0; bool ldmRecOk = false;     // the last pass's stage (ZSTDMI_debugLdmPass)
    bool ldmSkipMerge = false;  // ZSTDMI_debugLdmSkipMerge
    u32 lastChunks = 0;         // chunks of the last pass (debug hook)
    const u8* lastSrc = nullptr; u32 lastChunkBytes = 0;     // its source (debug hook: chunks without sequences keep their literals there)
    u32 passChunks = 16384;     // chunks per pass: 1 GiB of input bounds the HBM workspace to ~4.2 GiB
    // cross-chunk history (row f-1): -1 = by level (on for the strategies above fast, i.e. levels >= 3: 16 KiB at levels 3-4, 32 KiB
    // above; and whenever the caller asks for a windowLog above 16), 0 = off (independent 64 KiB frames), else the bytes of
    // history per block (4 KiB units)
    int historyBytes = -1; u32 frameBytes = 256u << 10;
    u32 parser = 0;                      // ZSTDMI_CCtx_setParser
    // streaming adapter (ZSTD_compressStream2): host-side batching in front of the one-shot engine
    std::vector<u8> sIn, sOut; size_t sOutPos = 0; bool sWrote = false, sEnding = false; size_t sBatch = (size_t)16 << 20;
    StageTimer timer;
    float stageMs[kMaxStages] = {}; const char* stageNames[kMaxStages] = {}; int nStages = 0;
    // dictionary (ZSTD_CCtx_loadDictionary).  dictHost = the history bytes: the last kDictKeep bytes of a raw-content dictionary
    // or of a formatted dictionary's content; host copy + device copy made at the next compression.  A formatted dictionary
    // (dictFull, validated on the device into `info`) also gives the frames their dictID and the first repcodes; its entropy
    // tables are not used (every block carries its own), which any decoder holding the dictionary accepts — unless
    // ZSTDMI_CCtx_setDictEntropy turned them on: then dictCTabDev holds them as compression tables (dict_ctables_kernel, built with
    // the dictionary's upload) and the first block of every frame is coded with them as its previous entropy state.
    // These fields are one DictDigest (above): `own` is what this context loaded and uploaded itself; while a ZSTD_CDict is referenced
    // (cdict, ZSTD_CCtx_refCDict) every reader takes the digest in force from dict_in_force() instead — the CDict's where it can be
    // shared, else `own` filled from the CDict's host bytes (cctx_adopt_cdict).  dictUploads: uploads of `own` (ZSTDMI_debugDictUploads)
    DictDigest own; const ZSTD_CDict_s* cdict = nullptr; bool dictDirty = false; long long dictUploads = 0;
    int dictEntropy = 0;        // ZSTDMI_CCtx_setDictEntropy (sticky)
    // ZSTDMI_CCtx_setEntropyCarry (sticky): the blocks of a multi-block frame are coded in order inside carry groups (zmi_carry.h) and
    // may reuse the Huffman table, the FSE tables and the repcodes of the blocks before them (carry_active says where).
    // lastCarryGroups: groups the carry instance walked in the last call (ZSTDMI_debugLastCarryGroups)
    int entropyCarry = 0; long long lastCarryGroups = 0;
    // ZSTDMI_CCtx_setDictIndex (sticky): the dictionary's content — its last dict_index_max() bytes — stays whole on the device with a
    // hash index over it, built once per upload (lz_fast.hip), and the fast strategy's chunks look candidates up there instead of
    // staging a tail of it.  dictWide = those bytes of a raw-content dictionary (kept at every load, so the switch may come later; a
    // formatted one has them in dictFull); dictIdxEnd / Len / Log = what the last upload indexed (Len 0: nothing).
    // ZSTDMI_CCtx_setDictIndexStrategy (sticky): the highest strategy at which the index is used.  At 2 an upload builds, behind the
    // fast finder's table in dictIdxDev, one table per hash of the dual finder (all three, so the level may change between calls).
    // ZSTDMI_CCtx_setDictIndexChain (sticky): the index also serves what resolves to the chain finder (levels 5 and up); an upload then
    // builds the dual finder's two tables as at strategy 2.  dixDist: the second plane of the chain search's dense chunks (lz_fast.hip),
    // of a context that uses it alone.  lastRegionList: the work list of the last pass's lz_region_kernel, null = none ran (debug hook)
    int dictIndex = 0, dictIndexStrategy = 1, dictIndexChain = 0;
    DevBuf dixDist; const u32* lastRegionList = nullptr;
    u64 dictGen = 0;            // bumped by every ZSTD_CCtx_loadDictionary: device workers copy the dictionary when theirs is older
    // ZSTDMI_CCtx_setDevices: one worker context per listed device (its own stream and workspaces there); a call's frames are
    // dealt to them in contiguous shares (compress_multi).  Empty = the context's own device only.
    std::vector<ZSTD_CCtx_s*> workers;
    DevBuf gatherIn, gatherOut;     // a many-range plan: the ranges of a kind side by side, and their output (compress_plan)
    DevBuf batchStage, batchTab;    // a batch of independent entries: their chunks at chunk boundaries, and the pass's tables (compress_entries)
    int lastBatchAlone = 0;         // entries of the last ZSTDMI_compressBatch that went through the single-call path (debug hook)
    // batched passes of the last compress_entries, and the chunks of those that ran the set instances (ZSTDMI_compressBatchCDicts; debug hooks)
    long long lastBatchPasses = 0, lastBatchSetChunks = 0;
    // ZSTDMI_compressPack: a round's frames in bound-sized slots before they are placed, and its placement table (compress_pack_impl);
    // entries the last pack handed to the single-call path and rows of the table it wrote (debug hooks)
    DevBuf packArena, packTab; int lastPackAlone = 0; long long lastPackFrames = 0;
    // ZSTDMI_compressPackAsync: the placement's columns, rows and state, sized by the async prepares (pack_async_tab)
    DevBuf packAsync;
    // ZSTDMI_CCtx_setSeekTable: one (compressed size, content size) pair per frame, filed on the device by every pass of a call
    // (seekOn: this call files them) at the running index seekCount; compress_device writes the table behind the frames from them
    int seekTable = 0; bool seekOn = false; u32 seekCount = 0;
    DevBuf seekEntries, seekSort;
    // ZSTD_CCtx_refPrefix: the caller's bytes (host or device), referenced until the next ZSTD_compress2 / ZSTDMI_compressDevice has
    // consumed them; a host prefix of the long form is staged into pfxStage inside that call
    const void* pfx = nullptr; size_t pfxSize = 0; DevBuf pfxStage;
    // ZSTDMI_CCtx_setSingleFrame (sticky): a call of more than 64 KiB, and a stream session, is ONE frame.  sfXxh: the content checksum's
    // state, carried from pass to pass and from batch to batch (frame.hip); a session keeps what the switch was when it began
    // (sSingle; and the checksum flag, which its header states), the bytes it has put into its frame (sTotal) and the last kStreamTail of them as the next batch's history (sTail)
    int singleFrame = 0; DevBuf sfXxh; XxhCarry sfXxhHost = {};
    bool sSingle = false; int sChecksum = 0; u64 sTotal = 0; std::vector<u8> sTail;     // (sChecksum: the flag the session's header states)
    // ZSTDMI_CCtx_setSlidingLdm (sticky): under the single frame, long-distance matching's window slides with the frame (sliding_active).
    // A session notes at its beginning whether it runs so and with which windowLog (sSliding, sSlideLog); it then keeps the frame's
    // latest content on the device instead of sTail: sWin holds sWinFill bytes, the last min(sTotal, 2^sSlideLog) of the frame among
    // them, and every batch is appended there (cstream_compress_sliding)
    int slidingLdm = 0;
    // ZSTDMI_CCtx_setFarOffsets (sticky): offsets of 2^29 and more may be written — a referenced prefix's long form up to prefix + source
    // = 2^31, a sliding long-distance window of 2^29 or 2^30 (far_limit, check_single_frame).  Off: every refusal is what it was.
    int farOffsets = 0;
    bool sSliding = false; int sSlideLog = 0; DevBuf sWin; size_t sWinFill = 0;
    // ZSTDMI_CCtx_prepareBatchAsync / ZSTDMI_compressBatchAsync: what the prepare resolved (asyncPrep, valid while cctx_gen() is what it
    // was then; paramGen: bumped by every setter, as dictGen is by every change of the dictionary in force), and the event recorded
    // behind the last enqueued pass (asyncPending: not yet waited for).  cctx_async_drain is the one place that waits for it; every
    // buffer of the context names `tally`, so that no growth or release frees memory an enqueued pass still uses, and counts there.
    HostTally tally; u64 paramGen = 0;
    // ZSTDMI_CCtx_setContentCuts (sticky; 0 = off, else avgLog): the single calls cut their source by content (zmi_cuts.h) and write
    // the pieces as a pack (compress_cut).  cutSmall / cutList / cutEnds: the mark's tile counts, the candidate list and the select's
    // output (content_cuts.hip); lastContentCuts: pieces of the last call that was cut (ZSTDMI_debugLastContentCuts)
    int contentCuts = 0; long long lastContentCuts = 0;
    DevBuf cutSmall, cutList, cutEnds;
    // ZSTDMI_digestPieces / ZSTDMI_contentCutsDigests (digest.hip): the pieces' offsets and their digests on the device
    DevBuf digOffs, digOut;
    // ZSTDMI_CCtx_prepareCutsAsync / ZSTDMI_contentCutsAsync (content_cuts_async.hip): what the prepare resolved and its one
    // workspace, which no other call touches.  Independent of asyncPrep and of every parameter; ZSTDMI_CCtx_setDevice / setDevices drop it.
    struct CutsPrep* cutsPrep = nullptr; DevBuf cutsAsync;
    struct AsyncPrep* asyncPrep = nullptr; hipEvent_t asyncEv = nullptr; bool asyncPending = false;
    ZSTD_CCtx_s();
};
// History per chunk lives in LDS beside the chunk: up to 32 KiB of dictionary in front of 32 KiB chunks, or up to 60 KiB when
// the whole input fits behind it in one chunk (small records, the usual dictionary case).
constexpr size_t kDictKeep = 60u << 10;
static u32 round_tile(size_t n) { return (u32)((n + 4095) & ~(size_t)4095); }
static size_t chunks_of(size_t bytes, u32 chunkBytes) { return (bytes + chunkBytes - 1) / chunkBytes; }     // (not narrowed: entry_batched compares it for any size)
// A referenced CDict's device copies serve a context on the CDict's device that has no device workers (a worker uploads its own copy,
// as of a loaded dictionary); everywhere else the context holds a private upload of the same bytes in `own`.
static bool cdict_shared(const ZSTD_CCtx* c) { return c->cdict && c->cdict->device == c->device && c->workers.size() <= 1; }
// the digest every reader of dictionary state asks: the CDict's while one is shared, else the context's own
static const DictDigest& dict_in_force(const ZSTD_CCtx* c) { return cdict_shared(c) ? c->cdict->dg : c->own; }
// -> bytes of dictionary used as history for an input of srcSize bytes (0 = none)
static u32 dict_prefix_len(const ZSTD_CCtx* c, size_t srcSize)
{
    const size_t have = dict_in_force(c).dictHost.size();
    if (have < 8) return 0;                                  // ZSTD_compress_insertDictionary ignores dictionaries < 8 bytes, U/ZstdCompress.cs:5469-5477
    const size_t wide = have < kDictKeep ? have : kDictKeep;
    if (srcSize <= kChunkSize - round_tile(wide)) return (u32)wide;
    return (u32)(have < (32u << 10) ? have : (32u << 10));
}



// -> content bytes of a dictionary that an index covers (0: one below 8 bytes, which is no dictionary at all); a formatted
// dictionary's content size is known once it has been validated (digest_upload)
static u32 digest_index_len(const DictDigest& g)
{
    const size_t have = g.dictFormatted ? (g.dictFull.empty() ? 0 : g.info.contentSize) : g.dictWide.size();
    if (have < 8) return 0;
    return (u32)(have < dict_index_max() ? have : dict_index_max());
}
// -> content bytes of the dictionary in force that the index covers (0 = no index: switch off, or no dictionary)
static u32 dict_index_len(const ZSTD_CCtx* c) { return c->dictIndex ? digest_index_len(dict_in_force(c)) : 0u; }

static size_t cctx_sync_dictionary(ZSTD_CCtx* c);
// (inside an ABI call's guarded(): the waits of this thread count for this context from here on, see HostTally)
static size_t cctx_bind(ZSTD_CCtx* c) { if (c && tl_guarded) tl_waits = &c->tally.waits; return ctx_bind(c); }
// The lifetime rule of an enqueued batch (ZSTDMI_compressBatchAsync), in one place: wait for the event behind the last enqueued pass.
// Called before anything the pass may still read or write is freed or handed to another stream — by every DevBuf of the context
// before it frees (HostTally::beforeFree: growth and release alike), and by ZSTD_freeCCtx, ZSTDMI_CCtx_setStream,
// ZSTD_CCtx_loadDictionary, ZSTD_CCtx_refCDict and a digest's re-upload directly.  A later call on the same stream is ordered by the stream.
static void cctx_async_drain(ZSTD_CCtx* c)
{
    if (!c->asyncPending) return;
    c->asyncPending = false;
    c->tally.waits++;
    if (hipEventSynchronize(c->asyncEv) != hipSuccess) (void)hipGetLastError();
}
// a blocking copy, counted as the wait it is
static hipError_t host_memcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) { count_wait(); return hipMemcpy(dst, src, n, kind); }
static u64 cctx_gen(const ZSTD_CCtx* c) { return c->paramGen + c->dictGen; }
// a cuts prepare (ZSTDMI_CCtx_prepareCutsAsync): the limits as resolved, the most pieces they allow and where everything lies in cutsAsync
struct CutsPrep { u64 bound; unsigned avgLog, kind; u32 maxCand; u64 maxPieces; u32 digestSize; CutsAsyncLayout lay; };
static void cctx_drop_cuts_prepare(ZSTD_CCtx* c) { delete c->cutsPrep; c->cutsPrep = nullptr; }
ZSTD_CCtx_s::ZSTD_CCtx_s()
{
    tally.self = this; tally.beforeFree = [](void* self) { cctx_async_drain((ZSTD_CCtx_s*)self); };
    for (DevBuf* b : { &seqs, &lits, &meta, &tables, &slots, &offsets, &total, &cand, &probe, &stageSrc, &stageDst, &ldmSmall, &ldmBig, &dixDist, &gatherIn, &gatherOut,
                       &batchStage, &batchTab, &packArena, &packTab, &packAsync, &seekEntries, &seekSort, &pfxStage, &sfXxh, &sWin, &cutSmall, &cutList, &cutEnds, &digOffs, &digOut, &cutsAsync,
                       &own.dict, &own.dictFullDev, &own.dictInfoDev, &own.dictCTabDev, &own.dictWideDev, &own.dictIdxDev }) b->owner = &tally;
    pin.owner = &tally;
}

// The parameters one compression call runs with: the context's sticky ones (ZSTD_compress2, ZSTD_compressStream2) or, for
// ZSTD_compressCCtx, the level alone with default frame parameters and no dictionary (U/ZstdCompress.cs:5751-5776:
// compress_usingDict(NULL) builds its parameters from the level and leaves the context's requested ones untouched).
struct CallParams {
    int level = 3, checksumFlag = 0, contentSizeFlag = 1, dictIDFlag = 1, strategy = 0, targetLength = 0, windowLog = 0, searchLog = 0;
    int minMatch = 0, chainLog = 0;     // accepted by the setters only at the value the kernels implement for the level/strategy in force THEN: checked again per call
    int ldm = 0, ldmHashLog = 0, ldmMinMatch = 0, ldmBucketSizeLog = 0, ldmHashRateLog = 0;     // (ZSTD_compressCCtx: all 0, as the reference's level-only parameters)
    bool useDict = true;
    bool seek = false;                  // append a seek table (ZSTDMI_CCtx_setSeekTable; ZSTD_compressCCtx: never, as it never runs LDM)
    bool dictIndex = false;             // look candidates up in the dictionary's index (ZSTDMI_CCtx_setDictIndex; ZSTD_compressCCtx uses no dictionary)
    int dictIndexStrategy = 1;          // ... at strategies up to this one (ZSTDMI_CCtx_setDictIndexStrategy)
    bool dictIndexChain = false;        // ... and where the call resolves to the chain finder (ZSTDMI_CCtx_setDictIndexChain)
    bool dictEntropy = false;           // code with a formatted dictionary's entropy tables (ZSTDMI_CCtx_setDictEntropy; ZSTD_compressCCtx uses no dictionary)
    bool entropyCarry = false;          // carry entropy tables and repcodes from block to block (ZSTDMI_CCtx_setEntropyCarry; ZSTD_compressCCtx: never, level-only parameters)
    const u8* pfx = nullptr; size_t pfxSize = 0;    // the long form of a referenced prefix (compress_prefixed): device bytes in front of the ONE frame
    bool single = false;                // one frame per call (ZSTDMI_CCtx_setSingleFrame; ZSTD_compressCCtx: never, level-only parameters)
    bool farOffsets = false;            // offsets of 2^29 and more may be written (ZSTDMI_CCtx_setFarOffsets; ZSTD_compressCCtx: never, level-only parameters)
    bool sliding = false;               // ... whose long-distance window slides with it (ZSTDMI_CCtx_setSlidingLdm; takes effect where sliding_active says)
    // a batch of a single-frame stream session (cstream_compress_single): streamAt bytes of the frame lie in front of it (the last
    // kStreamTail of them readable in front of the source), and the batch ends the frame or not
    bool stream = false, streamEnd = false; u64 streamAt = 0;
};
static CallParams sticky_params(const ZSTD_CCtx* c)
{
    CallParams p; p.level = c->cdict ? c->cdict->level : c->level; p.checksumFlag = c->checksumFlag; p.contentSizeFlag = c->contentSizeFlag; p.dictIDFlag = c->dictIDFlag;
    p.strategy = c->strategy; p.targetLength = c->targetLength; p.windowLog = c->windowLog; p.searchLog = c->searchLog; p.minMatch = c->minMatch; p.chainLog = c->chainLog; p.useDict = true;
    p.seek = c->seekTable != 0;
    p.dictEntropy = c->dictEntropy != 0;
    p.entropyCarry = c->entropyCarry != 0;
    p.dictIndex = c->dictIndex != 0; p.dictIndexStrategy = c->dictIndexStrategy; p.dictIndexChain = c->dictIndexChain != 0;
    p.single = c->singleFrame != 0; p.sliding = c->slidingLdm != 0; p.farOffsets = c->farOffsets != 0;
    p.ldm = c->ldm; p.ldmHashLog = c->ldmHashLog; p.ldmMinMatch = c->ldmMinMatch; p.ldmBucketSizeLog = c->ldmBucketSizeLog; p.ldmHashRateLog = c->ldmHashRateLog;
    return p;
}

// What a call resolves to: the reference's cParams for (level, chunk size) with the explicitly set strategy /
// targetLength on top (ZSTD_overrideCParams, U/ZstdCompress.cs:2096-2127), then the parts of them the kernels act on.
// (struct Resolved: zmi_batch_pass.h, beside the batch's group key, which compares it)
static Resolved resolve_call(const CallParams& p, size_t srcSize, u32 chunkBytes)
{
    Resolved r;
    r.cp = get_cparams(p.level, srcSize < chunkBytes ? srcSize : chunkBytes);
    if (p.strategy) r.cp.strategy = (u32)p.strategy;
    if (p.targetLength) r.cp.targetLength = (u32)p.targetLength;
    if (p.searchLog) r.cp.searchLog = (u32)p.searchLog;
    // match finder by strategy (U/ZstdCompress.cs:3397-3417 selects the block compressor the same way): fast; doubleFast -> the
    // dual-hash finder; greedy and everything above it -> dual-hash + lazy deferral (no lazy2 / binary-tree / optimal parsers)
    r.finder = r.cp.strategy <= kStratFast ? 0u : r.cp.strategy == kStratDfast ? 1u : 2u;
    // ZSTD_fast probes two of every targetLength + 2 positions once a step is set (negative levels; U/ZstdFast.cs:101-103,
    // 130-136) but falls back to every position right after each match; the tile finder's counterpart is a floor under its
    // probing stride (a power of two, fixed per 4-16 KiB), set at half the reference's density so that it does not lose more
    // ratio than the reference's own step does (measured against the oracle at levels -5 and -20 in tests/test_gpu_boundary.py)
    r.minStrideLog = 0;
    if (r.cp.strategy == kStratFast && r.cp.targetLength > 5) {
        const u32 gap = (r.cp.targetLength + 2) / 4;
        r.minStrideLog = cp_highbit32(gap); if (r.minStrideLog > 4) r.minStrideLog = 4;
    }
    r.rawLiterals = literals_compression_disabled(r.cp) ? 1u : 0u;
    return r;
}

static bool cctx_workspace(ZSTD_CCtx* c, u32 nChunks)
{
    return c->seqs.ensure((size_t)nChunks * kMaxSeq * sizeof(Seq)) && c->lits.ensure((size_t)nChunks * kLitStride + 64) &&
           c->meta.ensure((size_t)nChunks * sizeof(ChunkMeta)) && c->tables.ensure((size_t)nChunks * sizeof(HufTable)) &&
           c->slots.ensure((size_t)nChunks * kSlotStride + 64) && c->offsets.ensure((size_t)nChunks * sizeof(u64)) &&
           c->total.ensure(64);
}
// the region parse of the fast strategy keeps one candidate position (u16) per input byte between its two steps (lz_fast.hip)
// region parse: candidates (u16 per position of a chunk's 64 KiB image) [+ the hash chains of the level >= 5 finder, same size] + the work list
static size_t cand_plane_bytes(u32 nChunks) { return (size_t)nChunks * kChunkSize * sizeof(u16) + 256; }
// the chain search behind an indexed dictionary: one u32 per position for each of lz_region_kernel's workgroups (at most 256)
static bool cctx_dist_workspace(ZSTD_CCtx* c, u32 nChunks) { return c->dixDist.ensure((size_t)(nChunks < 256 ? nChunks : 256) * kChunkSize * sizeof(u32)); }
static bool cctx_cand_workspace(ZSTD_CCtx* c, u32 nChunks, bool chains) { return c->cand.ensure(cand_plane_bytes(nChunks) * (chains ? 2 : 1) + ((size_t)nChunks + 1) * sizeof(u32)); }

// A digest's host bytes onto the current device, on stream s, waited for: a formatted dictionary is first validated there
// (ZSTD_loadCEntropy's checks are those of ZSTD_loadDEntropy plus the symbol-coverage rules that only matter to an encoder reusing the
// tables) -> dictionary_corrupted, with the digest emptied.  entropy: build its DictCTables; index: the fast finder's table over the
// content's last dict_index_max() bytes; dual: behind it the dual finder's two.  (A context passes its switches, a CDict all three.)
static size_t digest_upload(DictDigest& g, hipStream_t s, bool entropy, bool index, bool dual)
{
    if (g.dictFormatted) {
        const size_t n = g.dictFull.size();
        if (!g.dictFullDev.ensure(n + 64) || !g.dictInfoDev.ensure(sizeof(DictInfo))) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(g.dictFullDev.p, g.dictFull.data(), n, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        launch_dict_parse((const u8*)g.dictFullDev.p, (u32)n, (DictInfo*)g.dictInfoDev.p, s);
        if (isErr(dev_read(&g.info, g.dictInfoDev.p, sizeof(DictInfo), s))) return ZERR(kErrGeneric);
        if (g.info.err) { g.dictFull.clear(); g.dictHost.clear(); g.dictFormatted = false; return ZERR(kErrDictionaryCorrupted); }
        const size_t keep = g.info.contentSize < kDictKeep ? g.info.contentSize : kDictKeep;
        g.dictHost.assign(g.dictFull.end() - (ptrdiff_t)keep, g.dictFull.end());
        if (entropy) {
            if (!g.dictCTabDev.ensure(sizeof(DictCTables))) return ZERR(kErrMemoryAllocation);
            launch_dict_ctables((const u8*)g.dictFullDev.p, (u32)n, (const DictInfo*)g.dictInfoDev.p, (DictCTables*)g.dictCTabDev.p, s);
            if (isErr(stream_wait(s))) return ZERR(kErrGeneric);
        }
    }
    if (!g.dictHost.empty()) {
        if (!g.dict.ensure(g.dictHost.size() + 64)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(g.dict.p, g.dictHost.data(), g.dictHost.size(), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        if (isErr(stream_wait(s))) return ZERR(kErrGeneric);
    }
    g.dictIdxLen = 0;
    if (const u32 ixLen = index ? digest_index_len(g) : 0u) {
        // the content's end on the device, with 64 readable bytes behind it: a formatted dictionary's ends dictFullDev; a raw one goes up whole
        const u8* end = nullptr;
        if (g.dictFormatted) end = (const u8*)g.dictFullDev.p + g.dictFull.size();
        else {
            if (!g.dictWideDev.ensure((size_t)ixLen + 64)) return ZERR(kErrMemoryAllocation);
            if (hipMemcpyAsync(g.dictWideDev.p, g.dictWide.data() + (g.dictWide.size() - ixLen), ixLen, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
            end = (const u8*)g.dictWideDev.p + ixLen;
        }
        const u32 log = dict_index_log(ixLen);
        if (!g.dictIdxDev.ensure((sizeof(u32) << log) * (dual ? 3 : 1))) return ZERR(kErrMemoryAllocation);
        u32* const tables = (u32*)g.dictIdxDev.p;          // fast [| long | short], 1 << log entries each
        launch_dict_index(end - ixLen, ixLen, tables, log, s);
        if (dual) launch_dict_index_dual(end - ixLen, ixLen, tables + ((size_t)1 << log), tables + ((size_t)2 << log), log, s);
        g.dictIdxDual = dual;
        if (isErr(stream_wait(s))) return ZERR(kErrGeneric);
        g.dictIdxEnd = end; g.dictIdxLen = ixLen; g.dictIdxLog = log;
    }
    return 0;
}
// upload a newly loaded dictionary with what the context's switches ask of it (their setters mark it dirty, so a switch turned on
// later builds its tables too).  A shared CDict is complete and on the device already: nothing to do, and nothing is counted.
static size_t cctx_sync_dictionary(ZSTD_CCtx* c)
{
    if (cdict_shared(c) || !c->dictDirty) return 0;
    cctx_async_drain(c);        // (a re-upload writes what an enqueued batch may still read)
    if (c->own.dictFormatted || !c->own.dictHost.empty()) c->dictUploads++;
    const size_t e = digest_upload(c->own, c->stream, c->dictEntropy != 0, c->dictIndex != 0, c->dictIndexStrategy >= 2 || c->dictIndexChain);
    if (isErr(e) && e != ZERR(kErrDictionaryCorrupted)) return e;
    c->dictDirty = false;
    return e;
}

// the dictionary's compression tables for a call, or nullptr: the switch is on and a formatted dictionary is in use (synced before)
static const DictCTables* call_dict_ctables(const ZSTD_CCtx* c, const CallParams& cp)
{
    const DictDigest& g = dict_in_force(c);
    return (cp.dictEntropy && cp.useDict && g.dictFormatted && g.dictCTabDev.p) ? (const DictCTables*)g.dictCTabDev.p : nullptr;
}

// How a range of paramSize bytes is cut into blocks and frames (a function of the parameters, the loaded dictionary and that size):
// bytes of dictionary in front of every chunk, bytes per block, blocks per frame (0 = every block a frame of its own), and what
// the level resolves to for it.
struct Framing { u32 prefixLen, chunkBytes, frameBlocks; Resolved rs; u32 indepWindowLog = 0; bool ldm = false; LdmLaunch ldmP = {};
                 bool dictIndex = false;    // full 64 KiB chunks, each a frame, behind the indexed dictionary (ZSTDMI_CCtx_setDictIndex)
                 bool single = false; u32 singleWindowLog = 0;      // ONE frame across passes; the window its header declares beside (or instead of) the content size, 0 = a single segment
                 u32 slideLog = 0;          // single and ldm: the stage's window is the 2^slideLog bytes in front of a position, wherever a pass or a batch begins (0: off)

                 size_t span() const { return (size_t)chunkBytes * (frameBlocks ? frameBlocks : 1u); } };

// Long-distance matching (ZSTD_c_enableLongDistanceMatching = ZSTD_ps_enable): on for a call of more than one block whose window is
// at least 2^17 (below, frames are no longer than the block finders' own reach and there is nothing for it to find).  The window is
// ZSTD_c_windowLog, or 2^27 (U/ZstdCompress.cs:2166-2171), shrunk to the input as ZSTD_adjustCParams does; the LDM parameters
// left at 0 follow from it as ZSTD_ldm_adjustParameters derives them (U/ZstdLdm.cs:187-212).  ZSTD_ps_auto and ZSTD_ps_disable
// are off: the reference's auto rule (btopt and above with windowLog >= 27) is not adopted, so no level's output changes.
constexpr int kLdmDefaultWindowLog = 27;
constexpr u64 kLdmMaxFrame = (u64)512 << 20;        // every offset stays below 2^29, what the decoder's sequence record packs (kRecOffMax)
// With ZSTDMI_CCtx_setFarOffsets on, what a referenced prefix and its source may span together, and the largest sliding window: ldm.hip's
// positions are 32-bit in the pass's virtual coordinate (prefix or window rounded up to a tile, then the pass of at most 2^31 bytes),
// so 2^30 + 2^31 is the most that stays inside it; a window of 2^31 would not.  Aligned long-distance frames keep kLdmMaxFrame.
constexpr u64 kFarMaxSpan = (u64)1 << 31;
constexpr int kSlideMaxLog = 28, kFarSlideMaxLog = 30;
static int ldm_window_log(const CallParams& cp) { return cp.windowLog ? cp.windowLog : kLdmDefaultWindowLog; }
static bool ldm_active(const CallParams& cp, size_t paramSize) { return cp.ldm == 1 && paramSize > kChunkSize && ldm_window_log(cp) >= 17; }
// the window of a referenced prefix in front of srcSize bytes: ceil_log2(prefixSize + srcSize), at least 17
static u32 prefix_window_log(size_t prefixSize, size_t srcSize)
{
    u32 wl = 17; while (wl < 31 && ((u64)1 << wl) < (u64)prefixSize + srcSize) ++wl;
    return wl;
}
static LdmLaunch ldm_resolve(const CallParams& cp, size_t paramSize)
{
    u32 wl = (u32)ldm_window_log(cp);
    u32 need = 10; while (need < 31 && ((u64)1 << need) < paramSize) ++need;
    if (wl > need) wl = need;
    LdmLaunch p;
    p.minMatch = cp.ldmMinMatch ? (u32)cp.ldmMinMatch : 64u;
    p.hashLog = cp.ldmHashLog ? (u32)cp.ldmHashLog : (wl > 13 ? wl - 7 : 6u);
    p.bucketLog = cp.ldmBucketSizeLog ? (u32)cp.ldmBucketSizeLog : 3u;
    if (p.bucketLog > p.hashLog) p.bucketLog = p.hashLog;
    p.hashRateLog = cp.ldmHashRateLog ? (u32)cp.ldmHashRateLog : (wl > p.hashLog ? wl - p.hashLog : 0u);
    if (p.hashRateLog < kLdmMinHashRateLog) p.hashRateLog = kLdmMinHashRateLog;      // (a derived value; a set one below it was refused)
    return p;
}

// ZSTDMI_CCtx_setSingleFrame: a call of more than one 64 KiB block, and every batch of a stream session, is (part of) ONE frame.
// A stream does not know its size: its parameters are those of the levels' default tier.
constexpr size_t kStreamParamSize = (size_t)1 << 30;
constexpr size_t kStreamTail = (size_t)256 << 10;       // history in front of a batch: more than any finder reaches back (lz_fast.hip: 64 KiB + kFarMax)
constexpr u64 kSingleMax = (u64)2 << 30;
static bool single_active(const CallParams& cp, size_t paramSize) { return cp.single && !cp.pfxSize && (cp.stream || (paramSize > kChunkSize && !ldm_active(cp, paramSize))); }

// bytes per block of a multi-block frame: the fast strategy keeps full 64 KiB blocks (far candidates); the dual-hash finders' blocks
// shrink to 64 KiB minus the hb bytes of history (whole 4 KiB tiles, at most 48 KiB) they carry in front of them in LDS
static u32 history_block_bytes(const Resolved& rf, int hb)
{
    if (rf.finder == 0) return kChunkSize;
    const u32 histB = round_tile((size_t)hb);
    return kChunkSize - (histB > (48u << 10) ? (48u << 10) : histB);
}
// the history of the framings that always have one (LDM windows, one frame per call): the context's, or by strategy
static int history_bytes_or_default(const ZSTD_CCtx* c, const Resolved& rf) { return c->historyBytes > 0 ? c->historyBytes : (rf.cp.strategy == kStratDfast ? (16 << 10) : (32 << 10)); }

static Framing resolve_framing(const ZSTD_CCtx* c, const CallParams& cp, size_t paramSize);
// the content of one frame of the long-distance framing (an aligned window: min(2^windowLog, 512 MiB, a pass))
static size_t ldm_frame_span(const ZSTD_CCtx* c, const CallParams& cp, size_t paramSize)
{
    CallParams plain = cp; plain.single = false; plain.sliding = false;
    return resolve_framing(c, plain, paramSize).span();
}
// ZSTDMI_CCtx_setSlidingLdm takes effect exactly where check_single_frame refuses without it: one frame, ZSTD_ps_enable, and a stream
// session or a call of more than one long-distance frame.  (Everywhere else the switch changes nothing.)
static bool sliding_active(const ZSTD_CCtx* c, const CallParams& cp, size_t paramSize)
{
    if (!cp.sliding || !cp.single || cp.pfxSize || cp.ldm != 1) return false;
    if (cp.stream) return true;
    return ldm_active(cp, paramSize) && paramSize > ldm_frame_span(c, cp, paramSize);
}

static Framing resolve_framing(const ZSTD_CCtx* c, const CallParams& cp, size_t paramSize)
{
    const bool sliding = sliding_active(c, cp, paramSize);
    if (sliding || single_active(cp, paramSize)) {
        // The blocks are the long-distance framing's (below) without its stage: full 64 KiB blocks with far candidates at the fast
        // strategy, 64 KiB - 16/32 KiB blocks behind LDS history above it; every block but the first sees the input in front of it,
        // wherever a pass or a batch begins (zmi_frame.h, kSingle).  The header is the reference's: with wl = ZSTD_c_windowLog, or the level's
        // windowLog for this size, a single segment when the content fits 2^wl, else a window descriptor for 2^wl beside the content
        // size (no finder reaches 2^18 back, and a wl below 18 was refused: check_single_frame).
        Framing f; f.prefixLen = 0; f.single = true;
        const Resolved rf = resolve_call(cp, paramSize, (u32)1 << 31);
        const u32 chunkBytes = history_block_bytes(rf, history_bytes_or_default(c, rf));
        // With a sliding long-distance window (sliding_active) the blocks, the finders and the header's rules are the same; wl is the
        // stage's window (ZSTD_c_windowLog, or 27), its parameters follow from it as they do for the aligned windows, and the stage
        // lets no offset exceed it (ldm.hip, WIN).
        const u32 wl = sliding ? (u32)ldm_window_log(cp) : cp.windowLog ? (u32)cp.windowLog : rf.cp.windowLog;
        f.singleWindowLog = (cp.stream || (u64)paramSize > ((u64)1 << wl)) ? wl : 0u;
        f.chunkBytes = chunkBytes; f.frameBlocks = 0x7FFFFFFFu; f.rs = rf;      // (frameBlocks: "blocks share a frame"; a block's place is counted in bytes: zmi_frame.h, kSingle)
        if (sliding) { f.ldm = true; f.slideLog = wl; f.ldmP = ldm_resolve(cp, paramSize); }
        return f;
    }
    if (cp.pfxSize || ldm_active(cp, paramSize)) {
        // Under LDM a frame is a window: min(2^windowLog, 512 MiB, the pass) of content (ldm.hip matches never leave their frame, so
        // no offset exceeds what the frame declares).  Blocks and history are those the level's windowLog > 16 path picks: full
        // 64 KiB blocks with far candidates at the fast strategy, 64 KiB - 16/32 KiB blocks behind LDS history above it.
        // Behind a referenced prefix (the long form, compress_prefixed) the window is prefix + source, at least 2^17, and the whole
        // source is ONE frame of those blocks.
        Framing f; f.prefixLen = 0; f.indepWindowLog = 0; f.ldm = true;
        u32 wl = (u32)ldm_window_log(cp);
        if (cp.pfxSize) {
            wl = prefix_window_log(cp.pfxSize, paramSize);
            CallParams q = cp; q.windowLog = (int)wl;
            f.ldmP = ldm_resolve(q, cp.pfxSize + paramSize);
        } else f.ldmP = ldm_resolve(cp, paramSize);
        const u64 win = ((u64)1 << wl) < kLdmMaxFrame ? ((u64)1 << wl) : kLdmMaxFrame;
        const Resolved rf = resolve_call(cp, paramSize < win ? paramSize : (size_t)win, (u32)(win < ((u64)1 << 31) ? win : ((u64)1 << 31)));
        const u32 chunkBytes = history_block_bytes(rf, history_bytes_or_default(c, rf));
        u32 frameBlocks = cp.pfxSize ? (u32)((paramSize + chunkBytes - 1) / chunkBytes) : (u32)(win / chunkBytes);
        if (frameBlocks > c->passChunks) frameBlocks = c->passChunks;
        if (frameBlocks < 2) frameBlocks = 2;
        f.chunkBytes = chunkBytes; f.frameBlocks = frameBlocks; f.rs = rf;
        return f;
    }
    // An indexed dictionary at the fast strategy — with ZSTDMI_CCtx_setDictIndexStrategy(2) at doubleFast, with
    // ZSTDMI_CCtx_setDictIndexChain(1) at everything above, the chain finder (whatever the other setting says): nothing of it is
    // staged, so a chunk is a whole 64 KiB block and every chunk a single-segment frame behind the dictionary (ZSTD_c_windowLog
    // 10 .. 15 keeps its own framing: a window below the block)
    if (cp.useDict && cp.dictIndex && dict_index_len(c) && !(cp.windowLog >= 10 && cp.windowLog < (int)kChunkLog)) {
        const Resolved rx = resolve_call(cp, paramSize, kChunkSize);
        if (rx.finder == 0 || (rx.finder == 1 && cp.dictIndexStrategy >= 2) || (rx.finder == 2 && cp.dictIndexChain)) { Framing f; f.prefixLen = 0; f.chunkBytes = kChunkSize; f.frameBlocks = 0; f.rs = rx; f.dictIndex = true; return f; }
    }
    const u32 prefixLen = cp.useDict ? dict_prefix_len(c, paramSize) : 0u;
    u32 chunkBytes = kChunkSize - round_tile(prefixLen);
    // ZSTD_c_windowLog 10 .. 15: independent frames of 1 << windowLog bytes (the reference cuts blocks at the window size and lets
    // no offset exceed it, U/ZstdCompress.cs:4690-4712, U/ZstdCompressInternal.cs:787-813; a frame that IS its own window does both)
    u32 indepWindowLog = 0;
    if (cp.windowLog >= 10 && cp.windowLog < (int)kChunkLog && chunkBytes > (1u << cp.windowLog)) { chunkBytes = 1u << cp.windowLog; indepWindowLog = (u32)cp.windowLog; }
    Resolved rs = resolve_call(cp, paramSize, chunkBytes);
    // Cross-chunk history (the window the block loop carries, U/ZstdCompress.cs:4705-4807): blocks of 64 KiB - hist
    // bytes, each with the hist bytes in front of it as match-only history in LDS, frameBlocks of them to a frame (so a
    // match never reaches out of its frame and frames stay independent units for the decoder and for sharding).  Without a
    // dictionary only (a dictionary's tail takes the same place in LDS).
    u32 frameBlocks = 0;
    // a frame never declares more than the window the caller asked for (its content size is its window)
    const u32 frameBytes = (cp.windowLog >= (int)kChunkLog && cp.windowLog < 31 && ((u64)1 << cp.windowLog) < c->frameBytes) ? (1u << cp.windowLog) : c->frameBytes;
    if (prefixLen == 0 && paramSize > kChunkSize && chunkBytes == kChunkSize && frameBytes > kChunkSize) {
        int hb = c->historyBytes;
        // by level: the doubleFast levels (3-4; 3 is the library's default level) stage 16 KiB of history per 48 KiB block (one
        // third more staging and hashing for three quarters of what 32 KiB buy), greedy and above 32 KiB per 32 KiB block
        if (hb < 0) hb = (rs.cp.strategy > kStratFast || cp.windowLog > (int)kChunkLog) ? (rs.cp.strategy == kStratDfast ? (16 << 10) : (32 << 10)) : 0;
        if (hb > 0) {
            // what the level resolves to at the frame's size decides the form: the fast strategy keeps full 64 KiB blocks and
            // finds far matches through its table (candidates in front of the block are verified against global memory, up to
            // 188 KiB back); the dual-hash finders' 16-bit tables cannot hold far positions, so their blocks shrink to
            // 64 KiB - hist and carry the hist bytes in front of them in LDS
            const Resolved rf = resolve_call(cp, paramSize < frameBytes ? paramSize : frameBytes, frameBytes);
            chunkBytes = history_block_bytes(rf, hb);
            frameBlocks = frameBytes / chunkBytes; if (frameBlocks < 2) frameBlocks = 2;
            rs = rf;
        }
    }
    // Small calls at the fast strategy (64 KiB < size <= kSmallCall, everything left to the level): a call of 10 MiB is 160 chunks on
    // 256 CUs, and what it waits for is ONE chunk's serial chains — the tANS states of seq_encode and, on the way back, of seq_decode
    // (~270 ns a sequence, 1.0 of a 2.4 ms round trip), then the Huffman streams.  Frames stay 64 KiB (match execution is ordered per
    // frame) but are cut into four blocks of 16 KiB, each behind the frame's earlier blocks in LDS (the history form of the dual-hash
    // levels): same window, four times as many chains a quarter as long, for a block header, a Huffman table and the unknown-repcode
    // start per 16 KiB (text: + 1.5 % of size).  The finder restages the history per block — on a chip that a call this size leaves idle.
    constexpr size_t kSmallCall = (size_t)32 << 20;
    if (!frameBlocks && prefixLen == 0 && chunkBytes == kChunkSize && c->historyBytes < 0 && cp.windowLog == 0 && rs.finder == 0 && rs.minStrideLog == 0 &&
        paramSize > kChunkSize && paramSize <= kSmallCall) {
        chunkBytes = 16u << 10; frameBlocks = kChunkSize / chunkBytes;
    }
    // ZSTD_c_windowLog 10 .. 15 (continued): the blocks of 1 << windowLog bytes are independent of each other but share frames of 64 KiB
    // with a window descriptor of exactly that windowLog — a frame per block would cost 13 bytes per KiB on incompressible input, more
    // than ZSTD_compressBound grants (the reference spends a 3-byte block header per window)
    if (indepWindowLog && paramSize > chunkBytes) frameBlocks = kChunkSize / chunkBytes; else indepWindowLog = 0;
    Framing f; f.prefixLen = prefixLen; f.chunkBytes = chunkBytes; f.frameBlocks = frameBlocks; f.rs = rs; f.indepWindowLog = indepWindowLog;
    return f;
}

// What either async prepare resolved: the parameters and the framing of an entry of exactly `bound` bytes (ZSTDMI_CCtx_prepareBatchAsync:
// one chunk, one single-block frame), the empty frame under those parameters, and the generation it holds for.  No device pointer is
// kept: the launch state is derived again per call (launch_state, host arithmetic), and the buffers, which only ever grow, are asked
// where they are.  maxChunks: the chunks one call may hold (one chunk per entry: maxEntries).  planned (entries of several chunks, or
// a chunk limit below maxEntries): the call cuts the entries into chunks on the device (zmi_batch_plan.h).
struct AsyncPrep { u64 gen; u32 maxEntries; size_t bound; CallParams cp; Framing fr; AsyncEmptyFrame empty; u32 maxChunks; bool planned; };

// What the kernels of a pass are launched with for a framing: derived in one place for the single call (compress_range) and the
// batch (compress_entries), whose bytes must be the same.
struct LaunchState {
    bool regionParse, hcChains, independent; u32 hcDepth, strategy;
    FrameHeaderSpec header;             // of every frame the call writes
    u32 initReps[3];                // the repcodes in front of every frame: a formatted dictionary's, or the format's
    const DictCTables* dct;         // a formatted dictionary's entropy tables (ZSTDMI_CCtx_setDictEntropy), or null
    const u8* prefix;               // the dictionary's tail in front of every chunk (fr.prefixLen bytes), or null
    DictIndexRef dix;               // the indexed dictionary (fr.dictIndex)
};
static LaunchState launch_state(const ZSTD_CCtx* c, const CallParams& cp, const Framing& fr)
{
    const Resolved& rs = fr.rs;
    LaunchState L;
    L.independent = fr.indepWindowLog != 0;       // (no history between the blocks of a frame)
    // (not the far-candidate finder; behind an indexed dictionary the chain finder alone has one)
    assert(!fr.dictIndex || (!fr.prefixLen && !fr.frameBlocks && fr.chunkBytes == kChunkSize && (rs.finder < 2 || cp.dictIndexChain)));
    L.regionParse = rs.minStrideLog == 0 && !(rs.finder == 0 && fr.frameBlocks && fr.chunkBytes >= kChunkSize) && (!fr.dictIndex || rs.finder == 2) && c->parser == 0;
    L.hcChains = L.regionParse && rs.finder >= 2;
    // attempts per position of the level >= 5 search: the reference's 1 << searchLog (U/ZstdLazy.cs:641-642), between 4 and 32; the
    // greedy and lazy strategies (levels 5-7) stop at 8 unless ZSTD_c_searchLog asks for more: measured on text, 32 attempts
    // instead of 8 cost twice the time for 1 % of size
    L.hcDepth = rs.cp.searchLog < 2 ? 4u : rs.cp.searchLog > 5 ? 32u : 1u << rs.cp.searchLog;
    if (L.hcDepth > 8 && rs.cp.strategy <= 4 && cp.searchLog == 0) L.hcDepth = 8;
    L.strategy = rs.cp.strategy < kStratGreedy ? rs.cp.strategy : (u32)kStratGreedy;      // ZSTD_selectEncodingType's < lazy heuristic is the one seq_encode holds (U/ZstdCompressSequences.cs:400-469): levels whose strategy is lazy or above get greedy's constants
    // a formatted dictionary: its dictID in every frame header (unless ZSTD_c_dictIDFlag = 0), its repcodes in front of every frame.
    // The window: one frame per call states its own beside (or instead of) the content size, frames of independent blocks the
    // block's; a stream's header never carries a content size
    const DictDigest& g = dict_in_force(c);
    const bool fmtDict = cp.useDict && g.dictFormatted;
    L.header.dictID = fmtDict ? g.info.dictID : 0u;
    L.header.dictIdBytes = (u8)(cp.dictIDFlag ? dict_id_bytes(L.header.dictID) : 0u);
    L.header.checksum = cp.checksumFlag ? 1 : 0;
    L.header.noContentSize = (cp.contentSizeFlag && !cp.stream) ? 0 : 1;
    L.header.windowLog = (u8)(fr.single ? fr.singleWindowLog : fr.indepWindowLog);
    const u32 plainReps[3] = { 1, 4, 8 };
    for (int i = 0; i < 3; ++i) L.initReps[i] = fmtDict ? g.info.rep[i] : plainReps[i];
    L.dct = call_dict_ctables(c, cp);
    L.prefix = fr.prefixLen ? (const u8*)g.dict.p + (g.dictHost.size() - fr.prefixLen) : nullptr;
    {
        const u32* const tables = (const u32*)g.dictIdxDev.p;
        const bool dual = g.dictIdxDual && tables;
        L.dix = DictIndexRef{ g.dictIdxEnd, g.dictIdxLen, tables, g.dictIdxLog, dual ? tables + ((size_t)1 << g.dictIdxLog) : nullptr, dual ? tables + ((size_t)2 << g.dictIdxLog) : nullptr };
    }
    return L;
}
// the finder's launch for a pass of nChunks chunks (the candidate planes lie where a workspace for planeChunks chunks puts them:
// candidates | hash chains | work list, cctx_cand_workspace)
static LzLaunch pass_lz(ZSTD_CCtx* c, const LaunchState& L, const Framing& fr, const u8* src, u64 srcSize, u32 nChunks, u32 planeChunks, const FrameLayout& frames, const u32* chunkLens)
{
    LzLaunch a = {};
    a.finder = fr.rs.finder; a.src = src; a.srcSize = srcSize; a.nChunks = nChunks;
    a.seqs = (Seq*)c->seqs.p; a.lits = (u8*)c->lits.p; a.meta = (ChunkMeta*)c->meta.p;
    a.prefix = L.prefix; a.prefixLen = fr.prefixLen;
    a.frames = frames; a.independent = L.independent; a.header = L.header; a.minStrideLog = fr.rs.minStrideLog;
    u8* const planes = (u8*)c->cand.p;
    a.cand = L.regionParse ? (u16*)planes : nullptr;
    a.chain = L.hcChains ? (u16*)(planes + cand_plane_bytes(planeChunks)) : nullptr;
    a.regionList = L.regionParse ? (u32*)(planes + cand_plane_bytes(planeChunks) * (L.hcChains ? 2 : 1)) : nullptr;
    a.hcDepth = L.hcDepth;
    a.dist = (L.regionParse && fr.dictIndex) ? (u32*)c->dixDist.p : nullptr;
    c->lastRegionList = (L.regionParse && (fr.rs.finder == 2 || (fr.rs.finder == 0 && !fr.prefixLen && fr.chunkBytes >= kChunkSize))) ? a.regionList : nullptr;
    a.claimCtr = (u32*)((u64*)c->total.p + 4);      // (the claim counter: a word of `total`'s 64 bytes)
    a.chunkLens = chunkLens; a.dix = fr.dictIndex ? &L.dix : nullptr;
    a.stream = c->stream; a.hook = c->timer.hook();
    return a;
}
// ZSTDMI_CCtx_setEntropyCarry takes effect in a pass whose chunks share frames and see no dictionary: not where every chunk is a frame
// of its own, not where the blocks of a frame are independent windows (ZSTD_c_windowLog 10 .. 15), not behind a loaded dictionary or
// a CDict of any kind (such calls write what they wrote, byte for byte)
static bool carry_active(const ZSTD_CCtx* c, const CallParams& cp, const Framing& fr, const LaunchState& ls)
{
    if (!cp.entropyCarry || !fr.frameBlocks || ls.independent || ls.dct || fr.prefixLen || fr.dictIndex) return false;
    const DictDigest& g = dict_in_force(c);
    return !(cp.useDict && (g.dictFormatted || !g.dictHost.empty()));
}
// the workspace of a pass of nCh chunks: the stages' buffers, the candidate planes of a region parse, the distance plane of its
// chain search behind an indexed dictionary.  staged_workspace: with the staging buffer and the table of a staged pass (below)
static bool pass_workspace(ZSTD_CCtx* c, const LaunchState& ls, const Framing& fr, u32 nCh)
{
    return cctx_workspace(c, nCh) && (!ls.regionParse || cctx_cand_workspace(c, nCh, ls.hcChains)) && (!ls.regionParse || !fr.dictIndex || cctx_dist_workspace(c, nCh));
}
static bool staged_workspace(ZSTD_CCtx* c, const LaunchState& ls, const Framing& fr, u32 nCh, size_t tabBytes)
{
    return pass_workspace(c, ls, fr, nCh) && c->batchStage.ensure((u64)nCh * fr.chunkBytes + 64) && c->batchTab.ensure(tabBytes);
}

// ---- the staged pass: the table form of the pipeline over c->batchStage, stated once for compress_entries, compress_batch_async_impl
// and compress_pack_async_impl, whose bytes must be the same.  staged_encode: batch_stage -> lz -> huf_build -> [xxh64] -> seq_encode,
// which leaves every chunk's size in its ChunkMeta; the caller's own placement kernel then fills `offsets`; staged_write: huf_encode ->
// gather, to base + offsets[chunk] below base + span.  The marks are compress_entries' stage times; an async call has the timer off.
struct StagedPass {
    u32 nCh, cb; FrameLayout frames;        // chunk slots of cb bytes in the staging buffer and each one's place in its frame
    const u64* dFrom; const u32* dLen;      // (device) where each chunk is staged from, and its length
    const DictCTables* dct;                 // a dictionary's entropy tables; in a set pass: those of any slot ("some slot has tables")
    const CDictSlot* dSlots; const u32* dChunkSlot;     // a set pass (two or more CDicts): the slot table and each chunk's slot, else null
    const SeqCarry* carry;                  // carried entropy state, else null
    bool checksum;
};
// (multi-block frames: each chunk's place from the table dFrame; else every chunk a frame)
static StagedPass staged_pass(u32 nCh, const Framing& fr, const u64* dFrom, const u32* dLen, const u32* dFrame, const DictCTables* dct, bool checksum)
{
    const FrameLayout frames = dFrame ? layout_table(fr.chunkBytes, fr.frameBlocks, dFrame) : layout_arith(fr.chunkBytes, 0, (u64)nCh * fr.chunkBytes);
    return StagedPass{ nCh, fr.chunkBytes, frames, dFrom, dLen, dct, nullptr, nullptr, nullptr, checksum };
}
static void staged_encode(ZSTD_CCtx* c, const LaunchState& ls, const Framing& fr, const StagedPass& p)
{
    hipStream_t s = c->stream;
    const u8* stage = (const u8*)c->batchStage.p; Seq* seqs = (Seq*)c->seqs.p; u8* lits = (u8*)c->lits.p; ChunkMeta* meta = (ChunkMeta*)c->meta.p; u8* slots = (u8*)c->slots.p;
    launch_batch_stage(p.dFrom, p.dLen, (u8*)c->batchStage.p, p.nCh, p.cb, s);      c->timer.mark("batch_stage", s);
    LzLaunch lz = pass_lz(c, ls, fr, stage, (u64)p.nCh * p.cb, p.nCh, p.nCh, p.frames, p.dLen);
    // (a set pass: the finder's set instance — behind staged tails or behind indexes — takes each chunk's dictionary from its slot)
    assert(!p.dSlots || fr.prefixLen || fr.dictIndex);
    if (p.dSlots) { lz.slots = p.dSlots; lz.chunkSlot = p.dChunkSlot; lz.prefix = nullptr; }
    launch_lz(lz);
    launch_huf_build(lits, meta, (HufTable*)c->tables.p, slots, p.nCh, fr.rs.rawLiterals, stage, p.frames, s, c->timer.hook(), p.dct, p.dSlots, p.dChunkSlot);
    if (p.checksum) { launch_xxh64(stage, meta, p.nCh, p.frames, s, p.dLen);        c->timer.mark("xxh64", s); }
    launch_seq_encode(seqs, meta, slots, p.nCh, ls.strategy, ls.header, 1, ls.initReps, p.frames, s, p.dct, p.dSlots, p.dChunkSlot, p.carry);      c->timer.mark("seq_encode", s);
}
// (the literals' tables are in force — huf_encode's dictEntropy — behind a dictionary's tables and in a carry pass)
static void staged_write(ZSTD_CCtx* c, const StagedPass& p, u8* base, u64 span)
{
    hipStream_t s = c->stream;
    const u8* stage = (const u8*)c->batchStage.p; const ChunkMeta* meta = (const ChunkMeta*)c->meta.p; u8* slots = (u8*)c->slots.p; const u64* offsets = (const u64*)c->offsets.p;
    launch_huf_encode((const u8*)c->lits.p, meta, (const HufTable*)c->tables.p, slots, base, offsets, span, p.nCh, stage, p.cb, s, p.dct || p.carry);      c->timer.mark("huf_encode", s);
    launch_gather(stage, (u64)p.nCh * p.cb, slots, meta, offsets, base, span, p.nCh, p.cb, s);      c->timer.mark("gather", s);
}
// a pass is over: its stage times into the call's, which are sums over its passes (inputs above 1 GiB take several)
static void add_stage_times(ZSTD_CCtx* c, bool& first)
{
    c->timer.finish(); c->nStages = c->timer.n;
    for (int i = 0; i < c->timer.n; i++) { c->stageMs[i] = (first ? 0.f : c->stageMs[i]) + c->timer.ms[i]; c->stageNames[i] = c->timer.names[i]; }
    first = false;
}

// ZSTD_writeEpilogue on an empty frame: header (FCS=0, single segment) + empty raw last block [+ checksum] -> its 9 .. 13 bytes into f
static size_t empty_frame_write(const CallParams& cp, u8* f)
{
    FrameHeaderSpec h = {}; h.checksum = cp.checksumFlag ? 1 : 0; h.noContentSize = cp.contentSizeFlag ? 0 : 1;
    if (h.noContentSize && cp.windowLog >= 10) h.windowLog = (u8)cp.windowLog;     // (the window descriptor states the caller's window)
    size_t n = frame_header_write(h, 0, f);
    f[n++] = 1; f[n++] = 0; f[n++] = 0;
    if (cp.checksumFlag) { f[n++] = 0x99; f[n++] = 0xE9; f[n++] = 0xD8; f[n++] = 0x51; }   // XXH64("") low 32 bits = 0x51D8E999
    return n;
}
// the compress pipeline over device-resident buffers: one range of the input with one set of parameters (see compress_device)
// paramSize: the size the parameters are resolved for — the whole range's, of which [d_src, d_src + srcSize) may be a frame-aligned
// part (a device worker's share of the range, compress_multi): what is written for a stretch of frames depends on nothing else
// markAt / marks (optional): input offsets (multiples of the frame span, ascending) whose place in the output is wanted -> marks[i]
static size_t compress_range(ZSTD_CCtx* c, const CallParams& cp, u8* d_dst, size_t dstCapacity, const u8* d_src, size_t srcSize, size_t paramSize, bool& first,
                             const std::vector<size_t>* markAt = nullptr, std::vector<u64>* marks = nullptr)
{
    hipStream_t s = c->stream;
    c->lastRegionList = nullptr;
    if (srcSize == 0) {     // (empty_frame_write)
        u8 f[18 + 3 + 4]; const size_t n = empty_frame_write(cp, f);
        if (dstCapacity < n) return ZERR(kErrDstSizeTooSmall);
        if (hipMemcpyAsync(d_dst, f, n, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        count_wait(); (void)hipStreamSynchronize(s);       // (deliberately not stream_wait: a failed wait is ignored here)
        return n;
    }
    if (cp.useDict) { const size_t e = cctx_sync_dictionary(c); if (isErr(e)) return e; }
    const Framing fr = resolve_framing(c, cp, paramSize);
    const u32 chunkBytes = fr.chunkBytes, frameBlocks = fr.frameBlocks;
    const LaunchState ls = launch_state(c, cp, fr);
    const Resolved rs = fr.rs;
    // one frame: where this range lies in it (a one-shot call IS the frame; a stream's batch continues it) and how long it is
    const u64 sfAt = cp.stream ? cp.streamAt : 0u, sfTotal = cp.stream ? (cp.streamEnd ? cp.streamAt + srcSize : ~(u64)0) : (u64)srcSize;
    if (fr.single && cp.checksumFlag) {
        if (!c->sfXxh.ensure(sizeof(XxhCarry))) return ZERR(kErrMemoryAllocation);
        if (sfAt == 0) {
            xxh_carry_reset(&c->sfXxhHost);
            if (hipMemcpyAsync(c->sfXxh.p, &c->sfXxhHost, sizeof(XxhCarry), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        }
    }
    const DictCTables* const dct = ls.dct;
    const u64 totalChunks = (srcSize + chunkBytes - 1) / chunkBytes;
    u32 passChunks = (u32)(totalChunks < c->passChunks ? totalChunks : c->passChunks);
    if (fr.ldm) { const u32 fit = (u32)(((u64)1 << 31) / chunkBytes), most = fr.slideLog ? fit : whole_frame_chunks(fit, frameBlocks); if (passChunks > most) passChunks = most; }    // (ldm.hip: u32 positions in a pass; a sliding window adds at most 2^30 in front, a prefix at most 2^30 + a tile: window + pass stay below 2^32)
    if (frameBlocks && !fr.single && passChunks < totalChunks) { passChunks = whole_frame_chunks(passChunks, frameBlocks); if (!passChunks) passChunks = frameBlocks; }     // frames never straddle passes
    // carried entropy state: a one-shot call's passes of the one frame are whole carry groups, so that the bytes do not depend on
    // ZSTDMI_CCtx_setPassChunks (a stream's batch ends a group where it ends)
    const bool carry = carry_active(c, cp, fr, ls);
    if (carry && fr.single && passChunks < totalChunks) passChunks = carry_pass_chunks(passChunks);
    if (!pass_workspace(c, ls, fr, passChunks)) return ZERR(kErrMemoryAllocation);
    size_t produced = 0;
    for (u64 c0 = 0; c0 < totalChunks; c0 += passChunks) {
        const u32 nChunks = (u32)((totalChunks - c0) < passChunks ? (totalChunks - c0) : passChunks);
        const u8* src = d_src + c0 * chunkBytes;
        const u64 n = (srcSize - c0 * chunkBytes) < (u64)nChunks * chunkBytes ? (srcSize - c0 * chunkBytes) : (u64)nChunks * chunkBytes;
        Seq* seqs = (Seq*)c->seqs.p; u8* lits = (u8*)c->lits.p; ChunkMeta* meta = (ChunkMeta*)c->meta.p;
        HufTable* tables = (HufTable*)c->tables.p; u8* slots = (u8*)c->slots.p; u64* offsets = (u64*)c->offsets.p; u64* total = (u64*)c->total.p;
        // (one frame: the pass's first block lies frames.at bytes into it; everything the kernels knew from a chunk's index in the pass comes from there)
        const FrameLayout frames = fr.single ? layout_single(chunkBytes, frameBlocks, sfAt + c0 * chunkBytes, sfTotal) : layout_arith(chunkBytes, frameBlocks, n);
        c->timer.begin(s);
        launch_lz(pass_lz(c, ls, fr, src, n, nChunks, passChunks, frames, nullptr));
        if (fr.ldm) {       // long-distance matches into the finder's sequence store (ldm.hip); the splits are counted first to size the workspace
            const u64 span = (u64)frameBlocks * chunkBytes;
            // a referenced prefix: splits over prefix and source as one window in the virtual coordinate (ldm.hip), nL = its end
            LdmPrefix lp;
            if (fr.slideLog) {
                // a sliding window: what the frame holds in front of this pass, up to 2^slideLog bytes of it, takes the prefix's place.
                // It lies in front of src (the caller's own input; a session's device window) and is read there.  The first pass has
                // nothing in front of it and runs the same instances, for the distance bound: it may be longer than the window.
                const u64 keep = frames.at < ((u64)1 << fr.slideLog) ? frames.at : ((u64)1 << fr.slideLog);
                lp.pre = src - keep; lp.base = (u32)((keep + kLdmPrefixAlign - 1) / kLdmPrefixAlign * kLdmPrefixAlign); lp.vlo = lp.base - (u32)keep;
                lp.maxDist = 1u << fr.slideLog;
            } else if (cp.pfxSize) { lp.pre = cp.pfx; lp.base = (u32)((cp.pfxSize + kLdmPrefixAlign - 1) / kLdmPrefixAlign * kLdmPrefixAlign); lp.vlo = lp.base - (u32)cp.pfxSize; }
            const u64 nL = lp.base + n;
            if (!c->ldmSmall.ensure(ldm_small_bytes(nL))) return ZERR(kErrMemoryAllocation);
            launch_ldm_count(src, nL, span, fr.ldmP, (u8*)c->ldmSmall.p, s, lp);
            u32 nSplits = 0;
            if (isErr(dev_read(&nSplits, ldm_total_word((u8*)c->ldmSmall.p, nL), sizeof(u32), s))) return ZERR(kErrGeneric);
            c->timer.mark("ldm_count", s);
            c->ldmRec = LdmRecord(); c->ldmRecBase = lp.base; c->ldmRecVlo = lp.vlo; c->ldmRecOk = true;
            if (nSplits) {
                if (!c->ldmBig.ensure(ldm_big_bytes(nSplits))) return ZERR(kErrMemoryAllocation);
                c->ldmRec = launch_ldm_rest(src, nL, nChunks, chunkBytes, span, fr.ldmP, nSplits, (u8*)c->ldmSmall.p, (u8*)c->ldmBig.p, seqs, lits, meta, s, c->timer.hook(), lp,
                                            !c->ldmSkipMerge);
            }
        } else c->ldmRecOk = false;
        launch_huf_build(lits, meta, tables, slots, nChunks, rs.rawLiterals, src, frames, s, c->timer.hook(), dct);
        if (cp.checksumFlag && fr.single) {
            // XXH64 does not merge: the whole content is one serial chain, carried from pass to pass (and from batch to batch); the
            // pass that ends the frame files the hash with its last block
            const bool ends = frames.at + n == sfTotal;
            launch_stream_xxh((XxhCarry*)c->sfXxh.p, src, n, ends ? 1u : 0u, s);
            if (ends) launch_xxh_carry_file((const XxhCarry*)c->sfXxh.p, meta + (nChunks - 1), s);
            c->timer.mark("xxh64", s);
        } else if (cp.checksumFlag) { launch_xxh64(src, meta, nChunks, frames, s);             c->timer.mark("xxh64", s); }
        SeqCarry sc = { tables, nullptr, 0, rs.rawLiterals };
        if (carry) { sc.nGroups = fr.single ? carry_groups_single(nChunks, frames.at, chunkBytes) : carry_groups_arith(nChunks, frameBlocks); c->lastCarryGroups += sc.nGroups; }
        launch_seq_encode(seqs, meta, slots, nChunks, ls.strategy, ls.header, 1, ls.initReps, frames, s, dct, nullptr, nullptr, carry ? &sc : nullptr);   c->timer.mark("seq_encode", s);
        // What the host wants of the pass — its total, and the output offsets of the chunks that start at the marked inputs — is stored
        // in the context's pinned block by the scan itself (markIdx: which of markAt fall into this pass, at most kPassMarks of them; a
        // pass with more marks reads them back one by one as it always did)
        PassMarks pm; size_t markIdx[kPassMarks]; bool marksPinned = true;
        if (markAt) for (size_t i = 0; i < markAt->size(); ++i) {
            const u64 ck = (*markAt)[i] / chunkBytes;
            if (ck < c0 || ck >= c0 + nChunks) continue;
            if (pm.n == kPassMarks) { marksPinned = false; pm.n = 0; break; }
            markIdx[pm.n] = i; pm.chunk[pm.n++] = (u32)(ck - c0);
        }
        if (!c->pin.ensure(kPassPinWords * sizeof(u64))) return ZERR(kErrMemoryAllocation);
        u64* const pinned = (u64*)c->pin.p;
        launch_scan_sizes(meta, nChunks, offsets, total, s, pinned, pm);           c->timer.mark("scan", s);
        if (c->seekOn) {        // the pass's frames into the call's seek table
            const u32 nFrames = (nChunks + (frameBlocks ? frameBlocks : 1u) - 1) / (frameBlocks ? frameBlocks : 1u);
            if (((size_t)c->seekCount + nFrames) * 8 > c->seekEntries.cap) return ZERR(kErrGeneric);
            launch_seek_entries(offsets, total, nChunks, frames, (u32*)c->seekEntries.p + 2 * (size_t)c->seekCount, s);
            c->seekCount += nFrames;
        }
        const size_t room = dstCapacity > produced ? dstCapacity - produced : 0;
        // the literals section (most of the output) is encoded straight into its final place; gather moves the rest
        launch_huf_encode(lits, meta, tables, slots, d_dst + produced, offsets, room, nChunks, src, chunkBytes, s, dct != nullptr || carry);   c->timer.mark("huf_encode", s);
        launch_gather(src, n, slots, meta, offsets, d_dst + produced, room, nChunks, chunkBytes, s);      c->timer.mark("gather", s);
        if (markAt && !marksPinned) for (size_t i = 0; i < markAt->size(); ++i) {
            const u64 ck = (*markAt)[i] / chunkBytes;
            if (ck >= c0 && ck < c0 + nChunks && hipMemcpyAsync(&(*marks)[i], offsets + (ck - c0), sizeof(u64), hipMemcpyDeviceToHost, s) != hipSuccess) return ZERR(kErrGeneric);
        }
        if (isErr(stream_wait(s))) return ZERR(kErrGeneric);
        const u64 passTotal = pinned[0];
        for (u32 k = 0; k < pm.n; ++k) (*marks)[markIdx[k]] = pinned[1 + k];
        if (markAt) for (size_t i = 0; i < markAt->size(); ++i) { const u64 ck = (*markAt)[i] / chunkBytes; if (ck >= c0 && ck < c0 + nChunks) (*marks)[i] += produced; }
        add_stage_times(c, first);
        if (passTotal > room) return ZERR(kErrDstSizeTooSmall);
        produced += (size_t)passTotal;
        c->lastChunks = nChunks; c->lastSrc = src; c->lastChunkBytes = chunkBytes;
    }
    return produced;
}

// Input the match finder gets nothing out of (BASELINE's Zipf bytes, random or already compressed data): the history, smaller blocks
// and deeper search of the levels >= 3 only cost there — Zipf at level 5 came out 0.8 % LARGER than at level 1 (a frame header share
// and a Huffman table per 32 KiB instead of per 64 KiB) at an eighth of the speed, and in a mixed input such stretches took a third
// of the match finder's time.  So a call of 4 MiB or more that leaves strategy, window and history to the level is first looked at
// in groups of 16 frames (~4 MiB): lz_probe_kernel counts, in eight 4 KiB tiles per group, the positions that repeat an earlier one of
// their tile or of the 60 KiB in front of it (text: several hundred per tile; Zipf bytes: a handful; an eighth of the input is read).
// Runs of groups below 32 per tile — the whole call, or at least 8 MiB of it — are compressed as level 1 would (its finder,
// independent 64 KiB frames: the same bytes level 1 writes for them), the rest by the level's own path; a group boundary is a frame
// boundary of both.  The decision is a function of the data alone: probe (device, per group) -> plan (host) -> ranges.
constexpr u32 kProbeTiles = 8;
constexpr size_t kMinRunBytes = (size_t)8 << 20;     // a stretch without matches becomes a range of its own from this length on
struct PlanRange { size_t off, len; bool sparse; };

// does the call get probed, and in groups of how many bytes?  (0 = no probe: one range, the call's own parameters)
static size_t probe_group_bytes(ZSTD_CCtx* c, const CallParams& cp, size_t srcSize, size_t& err)
{
    err = 0;
    // (a caller-set targetLength keeps the level's own path: at the fast strategy it means raw literals, which the sparse ranges must not inherit)
    if (!(srcSize >= (4u << 20) && c->historyBytes < 0 && cp.strategy == 0 && cp.windowLog == 0 && cp.searchLog == 0 && cp.targetLength == 0)) return 0;
    if (cp.pfxSize || ldm_active(cp, srcSize)) return 0;          // (one range: LDM frames are windows)
    if (cp.useDict) { err = cctx_sync_dictionary(c); if (isErr(err)) return 0; err = 0; }
    if (cp.useDict && dict_prefix_len(c, srcSize)) return 0;
    if (resolve_call(cp, srcSize, kChunkSize).cp.strategy <= kStratFast) return 0;
    CallParams framed = cp; framed.single = false;      // (one frame or not, the probe looks at the groups it looks at today)
    const Framing fr = resolve_framing(c, framed, srcSize);
    return (size_t)16 * (fr.frameBlocks ? fr.span() : (size_t)kChunkSize * 4);      // a multiple of 64 KiB
}
// counts of the groups of [d_src, d_src + len); `front` = bytes of the input readable in front of d_src (a worker's share of a call)
static size_t probe_run(ZSTD_CCtx* c, const u8* d_src, size_t len, size_t front, size_t group, u32* counts)
{
    const u32 nGroups = (u32)((len + group - 1) / group);
    if (!c->probe.ensure((size_t)nGroups * sizeof(u32))) return ZERR(kErrMemoryAllocation);
    launch_lz_probe(d_src, len, front, group, nGroups, kProbeTiles, (u32*)c->probe.p, c->stream);
    if (isErr(dev_read(counts, c->probe.p, (size_t)nGroups * sizeof(u32), c->stream))) return ZERR(kErrGeneric);
    return 0;
}
static void plan_ranges(const std::vector<u32>& counts, size_t group, size_t srcSize, std::vector<PlanRange>& out)
{
    const u32 nGroups = (u32)counts.size();
    // a range is a pass of its own: a stretch without matches counts if it is the whole call or at least kMinRunBytes long (round 2
    // asked for 64 MiB, because the passes of a many-range plan ran one after the other and none filled the chip: the mixed bench
    // input's 12.8 MiB pieces took 1.7 x the time as ranges of their own; now the ranges of a kind are compressed as one pass, compress_plan)
    std::vector<u8> sp(nGroups);
    for (u32 g = 0; g < nGroups; ++g) sp[g] = counts[g] < kProbeTiles * 32;
    const u32 minRun = (u32)((kMinRunBytes + group - 1) / group);
    for (u32 g = 0; g < nGroups; ) {
        u32 e = g + 1;
        while (e < nGroups && sp[e] == sp[g]) ++e;
        if (sp[g] && e - g < minRun && !(g == 0 && e == nGroups)) for (u32 k = g; k < e; ++k) sp[k] = 0;
        g = e;
    }
    for (u32 g = 0; g < nGroups; ) {
        const bool sparse = sp[g] != 0;
        u32 e = g + 1;
        while (e < nGroups && (sp[e] != 0) == sparse) ++e;
        PlanRange r; r.off = (size_t)g * group; r.len = (e == nGroups ? srcSize : (size_t)e * group) - r.off; r.sparse = sparse;
        out.push_back(r);
        g = e;
    }
}
// LDM together with a dictionary: the dictionary's framing (a prefix in front of independent 64 KiB frames) cannot hold a window-sized frame
static size_t check_ldm_dict(const ZSTD_CCtx* c, const CallParams& cp, size_t srcSize)
{
    if (ldm_active(cp, srcSize) && cp.useDict && (dict_in_force(c).dictFormatted || dict_in_force(c).dictHost.size() >= 8)) return ZERR(kErrParameterUnsupported);
    return 0;
}
// ZSTDMI_CCtx_setSingleFrame with what one frame across passes cannot be: refused at the call, before a byte is read.  (Calls of at
// most 64 KiB are one frame with or without the switch, and a referenced prefix writes one frame anyway: nothing to refuse.)
static size_t check_single_frame(const ZSTD_CCtx* c, const CallParams& cp, size_t srcSize)
{
    if (!cp.single || cp.pfxSize || (!cp.stream && srcSize <= kChunkSize)) return 0;
    if ((u64)srcSize > kSingleMax) return ZERR(kErrParameterUnsupported);
    if (cp.seek || c->workers.size() > 1) return ZERR(kErrParameterUnsupported);       // (frames are the seek table's and the workers' unit)
    if (cp.windowLog >= 10 && cp.windowLog < 18) return ZERR(kErrParameterUnsupported); // (the finders reach up to 2^18 back)
    if (cp.useDict && (dict_in_force(c).dictFormatted || dict_in_force(c).dictHost.size() >= 8)) return ZERR(kErrParameterUnsupported);   // (a dictionary's framing: a prefix in front of independent blocks)
    if (cp.stream ? cp.ldm == 1 : ldm_active(cp, srcSize)) {       // one LDM frame is one frame already (bytes unchanged); more than one is not,
        if (cp.stream || srcSize > ldm_frame_span(c, cp, srcSize)) {  // unless the window slides (ZSTDMI_CCtx_setSlidingLdm): up to 2^28 (what a sequence record of the decoder packs), with ZSTDMI_CCtx_setFarOffsets up to 2^30
            if (!cp.sliding || ldm_window_log(cp) > (cp.farOffsets ? kFarSlideMaxLog : kSlideMaxLog)) return ZERR(kErrParameterUnsupported);
        }
    }
    return 0;
}
static size_t check_call_params(const CallParams& cp)
{
    if (cp.minMatch || cp.chainLog) {       // set under another level or strategy than the call runs with: refuse, never ignore
        const CParams lv = get_cparams(cp.level, kChunkSize);
        if (cp.minMatch && cp.minMatch != (int)kernel_min_match(cp.strategy ? (u32)cp.strategy : lv.strategy)) return ZERR(kErrParameterUnsupported);
        if (cp.chainLog && cp.chainLog != (int)lv.chainLog) return ZERR(kErrParameterUnsupported);
    }
    return 0;
}

static size_t compress_multi(ZSTD_CCtx* c, const CallParams& cp, void* dst, size_t dstCapacity, const void* src, size_t srcSize);
// a single call under ZSTDMI_CCtx_setContentCuts (defined behind the pack, whose rounds it runs)
static size_t compress_cut(ZSTD_CCtx* c, const CallParams& cp, void* dst, size_t dstCapacity, const void* src, size_t srcSize, bool deviceCall);

// A plan of several ranges (a mixed input: stretches the level's finder is for, stretches without matches) as it stands is a run of
// small passes — a handful of kernels over a few hundred chunks each, none of which fills the chip; side by side on several
// streams they only queue for the CUs (the finders hold a CU's LDS alone; measured: slower than one after the other).  So the
// ranges of a KIND are gathered into one contiguous buffer and compressed as ONE pass sequence per kind (range lengths are whole
// probe groups, i.e. whole frames of either framing; the call's tail is the last range of its kind), each range's place in that
// output is read back with the pass (marks), and the pieces are copied into the caller's buffer in the order of the input.  Two
// pass sequences instead of one per range; the bytes are those of the ranges one after the other.  paramSize: the whole call's.
static size_t compress_plan(ZSTD_CCtx* c, const CallParams& cp, const std::vector<PlanRange>& plan, size_t paramSize, u8* d_dst, size_t dstCapacity, const u8* d_src, bool& first)
{
    const size_t R = plan.size();
    CallParams cpSparse = cp; cpSparse.level = 1;
    size_t len[2] = {0, 0}, cnt[2] = {0, 0};
    for (const PlanRange& r : plan) { len[r.sparse] += r.len; cnt[r.sparse]++; }
    // the kinds' inputs, contiguous (a kind with one range is read where it lies)
    size_t inAt[2] = {0, len[0] + 256};
    const size_t inNeed = (cnt[0] > 1 ? len[0] + 256 : 0) + (cnt[1] > 1 ? len[1] + 256 : 0);
    if (inNeed && !c->gatherIn.ensure(inAt[1] + len[1] + 256)) return ZERR(kErrMemoryAllocation);
    size_t bound[2], outAt[2] = {0, 0};
    for (int k = 0; k < 2; ++k) bound[k] = len[k] ? ((ZSTD_compressBound(len[k]) + (len[k] >> 12) + 4096) & ~(size_t)255) : 0;
    outAt[1] = bound[0];
    if (!c->gatherOut.ensure(bound[0] + bound[1] + 256)) return ZERR(kErrMemoryAllocation);
    std::vector<size_t> markAt[2]; std::vector<u64> marks[2];
    { size_t fill[2] = {0, 0};
      for (const PlanRange& r : plan) {
          const int k = r.sparse;
          markAt[k].push_back(fill[k]);
          if (cnt[k] > 1 && hipMemcpyAsync((u8*)c->gatherIn.p + inAt[k] + fill[k], d_src + r.off, r.len, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
          fill[k] += r.len;
      } }
    size_t got[2] = {0, 0};
    u32 seekAt[3] = { c->seekCount, c->seekCount, c->seekCount };      // where each kind's seek-table entries begin (and where they end)
    for (int k = 0; k < 2; ++k) {
        seekAt[k] = c->seekCount;
        if (!len[k]) continue;
        marks[k].assign(markAt[k].size(), 0);
        const u8* in = (const u8*)c->gatherIn.p + inAt[k];
        if (cnt[k] == 1) for (const PlanRange& r : plan) if ((int)r.sparse == k) in = d_src + r.off;
        const size_t n = compress_range(c, k ? cpSparse : cp, (u8*)c->gatherOut.p + outAt[k], bound[k], in, len[k], paramSize, first, &markAt[k], &marks[k]);
        if (isErr(n)) return n;
        got[k] = n;
    }
    seekAt[2] = c->seekCount;
    if (c->seekOn && seekAt[2] > seekAt[0]) {
        // the seek-table entries were filed kind by kind: into the order of the input, range by range (a range starts at a frame of its
        // kind's framing, so its first entry is its start in the kind's input over that framing's span)
        const size_t bytes = (size_t)(seekAt[2] - seekAt[0]) * 8;
        u8* const ent = (u8*)c->seekEntries.p + (size_t)seekAt[0] * 8;
        if (!c->seekSort.ensure(bytes)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(c->seekSort.p, ent, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
        const size_t span[2] = { resolve_framing(c, cp, paramSize).span(), resolve_framing(c, cpSparse, paramSize).span() };
        const size_t kindEnd[2] = { (size_t)(seekAt[1] - seekAt[0]), (size_t)(seekAt[2] - seekAt[0]) };
        size_t at = 0, seenK[2] = {0, 0};
        for (size_t r = 0; r < R; ++r) {
            const int k = plan[r].sparse;
            const size_t i = seenK[k]++;
            const size_t base = k ? kindEnd[0] : 0;
            const size_t lo = base + markAt[k][i] / span[k], hi = i + 1 < markAt[k].size() ? base + markAt[k][i + 1] / span[k] : kindEnd[k];
            if (hi > lo && hipMemcpyAsync(ent + at * 8, (const u8*)c->seekSort.p + lo * 8, (hi - lo) * 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
            at += hi - lo;
        }
    }
    if (got[0] + got[1] > dstCapacity) return ZERR(kErrDstSizeTooSmall);
    size_t pos = 0, seen[2] = {0, 0};
    for (size_t r = 0; r < R; ++r) {
        const int k = plan[r].sparse;
        const size_t i = seen[k]++;
        const u64 lo = marks[k][i], hi = i + 1 < marks[k].size() ? marks[k][i + 1] : got[k];
        if (hipMemcpyAsync(d_dst + pos, (const u8*)c->gatherOut.p + outAt[k] + lo, (size_t)(hi - lo), hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
        pos += (size_t)(hi - lo);
    }
    if (isErr(stream_wait(c->stream))) return ZERR(kErrGeneric);
    c->lastChunks = 0;
    return pos;
}

static size_t compress_frames(ZSTD_CCtx* c, const CallParams& cp, u8* d_dst, size_t dstCapacity, const u8* d_src, size_t srcSize)
{
    bool first = true;
    { const size_t e = check_call_params(cp); if (isErr(e)) return e; }
    { const size_t e = check_ldm_dict(c, cp, srcSize); if (isErr(e)) return e; }
    { const size_t e = check_single_frame(c, cp, srcSize); if (isErr(e)) return e; }
    size_t err = 0;
    const size_t group = probe_group_bytes(c, cp, srcSize, err);
    if (isErr(err)) return err;
    if (!group) return compress_range(c, cp, d_dst, dstCapacity, d_src, srcSize, srcSize, first);
    std::vector<u32> counts((srcSize + group - 1) / group);
    { const size_t e = probe_run(c, d_src, srcSize, 0, group, counts.data()); if (isErr(e)) return e; }
    std::vector<PlanRange> plan;
    plan_ranges(counts, group, srcSize, plan);
    if (plan.size() == 1) { CallParams one = cp; if (plan[0].sparse) one.level = 1; return compress_range(c, one, d_dst, dstCapacity, d_src, srcSize, srcSize, first); }
    // one frame is not cut into ranges: a mixed input takes the level's own path as a whole (its stretches without matches cost the
    // level's finder instead of level 1's)
    if (single_active(cp, srcSize)) return compress_range(c, cp, d_dst, dstCapacity, d_src, srcSize, srcSize, first);
    return compress_plan(c, cp, plan, srcSize, d_dst, dstCapacity, d_src, first);
}

// Seek table (the zstd seekable format: a skippable frame behind the last frame).  Frames a call can write: the smallest framing is a
// frame per 4 KiB of content (a 60 KiB dictionary in front of 4 KiB chunks); windows below 64 KiB share 64 KiB frames; every pass
// and every range of a plan ends on a frame boundary except the call's tail.  So a call of srcSize bytes writes at most
// srcSize / 4096 + 1 frames (the + 1: the tail's partial frame, or the one frame of an empty input), each an 8-byte entry, behind
// an 8-byte skippable header and in front of the 9-byte footer.
static size_t seek_max_frames(size_t srcSize) { return srcSize / 4096 + 1; }
static size_t seek_table_bound(size_t srcSize) { return 17 + 8 * seek_max_frames(srcSize); }

// one call over device-resident buffers: the frames and, when the call asks for it, the seek table behind them
static size_t compress_device(ZSTD_CCtx* c, const CallParams& cp, u8* d_dst, size_t dstCapacity, const u8* d_src, size_t srcSize)
{
    if (!cp.seek) return compress_frames(c, cp, d_dst, dstCapacity, d_src, srcSize);
    if (!c->seekEntries.ensure(seek_max_frames(srcSize) * 8)) return ZERR(kErrMemoryAllocation);
    struct On { ZSTD_CCtx* c; ~On() { c->seekOn = false; } } on{c};
    c->seekOn = true; c->seekCount = 0;
    const size_t r = compress_frames(c, cp, d_dst, dstCapacity, d_src, srcSize);
    if (isErr(r)) return r;
    hipStream_t s = c->stream;
    if (srcSize == 0) {         // the one empty frame: the host wrote it and knows its size
        const u32 e[2] = { (u32)r, 0 };
        if (hipMemcpyAsync(c->seekEntries.p, e, sizeof e, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        if (isErr(stream_wait(s))) return ZERR(kErrGeneric);
        c->seekCount = 1;
    }
    const size_t tableBytes = 17 + 8 * (size_t)c->seekCount;
    if (tableBytes > dstCapacity - r) return ZERR(kErrDstSizeTooSmall);
    launch_seek_table((const u32*)c->seekEntries.p, c->seekCount, d_dst + r, s);
    if (isErr(stream_wait(s))) return ZERR(kErrGeneric);
    return r + tableBytes;
}


// ======================================================================================================
extern "C" {

ZSTD_CCtx* ZSTD_createCCtx(void) { return new (std::nothrow) ZSTD_CCtx_s(); }

size_t ZSTD_freeCCtx(ZSTD_CCtx* c)
{
    if (!c) return 0;
    for (ZSTD_CCtx* w : c->workers) (void)ZSTD_freeCCtx(w);
    c->workers.clear();
    if (tl_waits == &c->tally.waits) tl_waits = nullptr;
    if (c->deviceOk) {
        (void)hipSetDevice(c->device);
        cctx_async_drain(c);        // (an enqueued batch may run on a stream that is not the context's own)
        if (c->asyncEv) (void)hipEventDestroy(c->asyncEv);
        if (c->ownStream) (void)hipStreamSynchronize(c->ownStream);
        c->seqs.release(); c->lits.release(); c->meta.release(); c->tables.release(); c->slots.release(); c->cand.release(); c->lastRegionList = nullptr; c->dixDist.release(); c->probe.release();
        c->gatherIn.release(); c->gatherOut.release(); c->batchStage.release(); c->batchTab.release(); c->packArena.release(); c->packTab.release(); c->packAsync.release(); c->ldmSmall.release(); c->ldmBig.release(); c->offsets.release(); c->total.release(); c->seekEntries.release(); c->seekSort.release(); c->stageSrc.release(); c->stageDst.release(); c->pfxStage.release(); c->sfXxh.release(); c->sWin.release(); c->cutSmall.release(); c->cutList.release(); c->cutEnds.release(); c->digOffs.release(); c->digOut.release(); c->cutsAsync.release(); c->own.release(); c->pin.release();
        c->timer.destroy();
        if (c->ownStream) (void)hipStreamDestroy(c->ownStream);
    }
    delete c->asyncPrep;
    cctx_drop_cuts_prepare(c);
    delete c;
    return 0;
}

int ZSTD_minCLevel(void) { return -(1 << 17); }
int ZSTD_maxCLevel(void) { return 22; }
int ZSTD_defaultCLevel(void) { return 3; }

size_t ZSTD_CCtx_setParameter(ZSTD_CCtx* c, int param, int value)
{
    if (!c) return ZERR(kErrGeneric);
    c->paramGen++;
    switch (param) {
    case ZSTD_c_compressionLevel:           // clamped, 0 means default (U/ZstdCompress.cs:886-905)
        if (value < ZSTD_minCLevel()) value = ZSTD_minCLevel();
        if (value > ZSTD_maxCLevel()) value = ZSTD_maxCLevel();
        c->level = value == 0 ? 3 : value;
        return c->level >= 0 ? (size_t)c->level : 0;        /* a size_t cannot carry a negative level (U/ZstdCompress.cs:899-905) */
    case ZSTD_c_checksumFlag:    if (value < 0 || value > 1) return ZERR(kErrParameterOutOfBound); c->checksumFlag = value; return (size_t)value;
    case ZSTD_c_contentSizeFlag: if (value < 0 || value > 1) return ZERR(kErrParameterOutOfBound);   /* 0: window descriptor instead of the content size */
                                 c->contentSizeFlag = value; return (size_t)value;
    case ZSTD_c_dictIDFlag:      if (value < 0 || value > 1) return ZERR(kErrParameterOutOfBound); c->dictIDFlag = value; return (size_t)value;
    case ZSTD_c_nbWorkers:       if (value != 0) return ZERR(kErrParameterUnsupported); return 0;   /* as U/ZstdCompress.cs:1064-1072 */
    case ZSTD_c_windowLog:       if (value != 0 && (value < 10 || value > 31)) return ZERR(kErrParameterOutOfBound);
                                 c->windowLog = value; return (size_t)value;            /* 10 .. 15: frames of 1 << windowLog bytes; 17+: frames of at most that */
    // Match-finder parameters (bounds: ZSTD_cParam_getBounds, U/ZstdCompress.cs:444-700).  0 = "from the level".  A value the
    // kernels implement is accepted and stored; any other value within bounds is parameter_unsupported, never silently ignored.
    case ZSTD_c_strategy:        // every strategy maps onto one of the three finders (resolve_call)
        if (value < 0 || value > 9) return ZERR(kErrParameterOutOfBound);
        c->strategy = value; return (size_t)value;
    case ZSTD_c_targetLength:    // fast strategy: acceleration (the probing stride) and, when > 0, raw literals; the other strategies' finders have no
                                 // counterpart of it (accepted and unused there, as the reference's greedy/lazy levels 5-12 ignore it: U/ZstdLazy.cs)
        if (value < 0 || value > (1 << 17)) return ZERR(kErrParameterOutOfBound);
        c->targetLength = value; return (size_t)value;
    case ZSTD_c_hashLog:         // the LDS tables have 2^13 buckets whatever the level's row says
        if (value != 0 && (value < 6 || value > 30)) return ZERR(kErrParameterOutOfBound);
        if (value != 0 && value != (int)kKernelHashLog) return ZERR(kErrParameterUnsupported);
        c->hashLog = value; return (size_t)value;
    case ZSTD_c_minMatch: {      // width of the finder's hash: 6 (fast), 5 (the others)
        if (value != 0 && (value < 3 || value > 7)) return ZERR(kErrParameterOutOfBound);
        const CParams cp = get_cparams(c->level, kChunkSize);
        if (value != 0 && value != (int)kernel_min_match(c->strategy ? (u32)c->strategy : cp.strategy)) return ZERR(kErrParameterUnsupported);
        c->minMatch = value; return (size_t)value; }
    case ZSTD_c_chainLog: {      // the chain table covers the finder's whole 64 KiB window: only the level's own value is accepted
        if (value != 0 && (value < 6 || value > 30)) return ZERR(kErrParameterOutOfBound);
        const CParams cp = get_cparams(c->level, kChunkSize);
        if (value != 0 && value != (int)cp.chainLog) return ZERR(kErrParameterUnsupported);
        c->chainLog = value; return (size_t)value; }
    case ZSTD_c_searchLog:       // attempts per position of the greedy/lazy search = 1 << searchLog (used from 2 to 5: 4 .. 32 attempts)
        if (value != 0 && (value < 1 || value > 30)) return ZERR(kErrParameterOutOfBound);
        c->searchLog = value; return (size_t)value;
    // Long-distance matching (ldm.hip; bounds: ZSTD_cParam_getBounds, U/ZstdCompress.cs:560-595).  0 = from the window.
    case ZSTD_c_enableLongDistanceMatching:     // ZSTD_ps_auto (0) and ZSTD_ps_disable (2): off; ZSTD_ps_enable (1): on
        if (value < 0 || value > 2) return ZERR(kErrParameterOutOfBound);
        c->ldm = value; return (size_t)value;
    case ZSTD_c_ldmHashLog:
        if (value != 0 && (value < 6 || value > 30)) return ZERR(kErrParameterOutOfBound);
        c->ldmHashLog = value; return (size_t)value;
    case ZSTD_c_ldmMinMatch:
        if (value != 0 && (value < 4 || value > 4096)) return ZERR(kErrParameterOutOfBound);
        c->ldmMinMatch = value; return (size_t)value;
    case ZSTD_c_ldmBucketSizeLog:
        if (value != 0 && (value < 1 || value > 8)) return ZERR(kErrParameterOutOfBound);
        c->ldmBucketSizeLog = value; return (size_t)value;
    case ZSTD_c_ldmHashRateLog:                 // 1 .. kLdmMinHashRateLog - 1: a split every 2 .. 16 bytes, more than the workspace holds
        if (value < 0 || value > 25) return ZERR(kErrParameterOutOfBound);
        if (value != 0 && value < (int)kLdmMinHashRateLog) return ZERR(kErrParameterUnsupported);
        c->ldmHashRateLog = value; return (size_t)value;
    default: return ZERR(kErrParameterUnsupported);
    }
}

size_t ZSTD_CCtx_getParameter(const ZSTD_CCtx* c, int param, int* value)
{
    if (!c || !value) return ZERR(kErrGeneric);
    switch (param) {
    case ZSTD_c_compressionLevel: *value = c->level; return 0;
    case ZSTD_c_checksumFlag: *value = c->checksumFlag; return 0;
    case ZSTD_c_contentSizeFlag: *value = c->contentSizeFlag; return 0;
    case ZSTD_c_dictIDFlag: *value = c->dictIDFlag; return 0;
    case ZSTD_c_nbWorkers: *value = 0; return 0;
    case ZSTD_c_windowLog: *value = c->windowLog; return 0;
    case ZSTD_c_hashLog: *value = c->hashLog; return 0;            // the requested values, 0 = from the level (U/ZstdCompress.cs:1100-1150)
    case ZSTD_c_chainLog: *value = c->chainLog; return 0;
    case ZSTD_c_searchLog: *value = c->searchLog; return 0;
    case ZSTD_c_minMatch: *value = c->minMatch; return 0;
    case ZSTD_c_targetLength: *value = c->targetLength; return 0;
    case ZSTD_c_strategy: *value = c->strategy; return 0;
    case ZSTD_c_enableLongDistanceMatching: *value = c->ldm; return 0;
    case ZSTD_c_ldmHashLog: *value = c->ldmHashLog; return 0;
    case ZSTD_c_ldmMinMatch: *value = c->ldmMinMatch; return 0;
    case ZSTD_c_ldmBucketSizeLog: *value = c->ldmBucketSizeLog; return 0;
    case ZSTD_c_ldmHashRateLog: *value = c->ldmHashRateLog; return 0;
    default: return ZERR(kErrParameterUnsupported);
    }
}

// ZSTD_compress_insertDictionary, U/ZstdCompress.cs:5465-5503: without the magic the bytes are raw content
// (ZSTD_loadDictionaryContent, :5126-5237) and the frames carry no dictID, exactly as the reference writes them; with it, a
// formatted dictionary (ZSTD_loadZstdDictionary, :5402-5463).
static size_t ZSTD_CCtx_loadDictionary_impl(ZSTD_CCtx* c, const void* dict, size_t dictSize)
{
    if (!c) return ZERR(kErrGeneric);
    if (!c->sIn.empty() || c->sEnding) return ZERR(kErrStageWrong);        /* not in the middle of a streaming frame session, U/ZstdCompress.cs:1273 */
    if (tl_guarded) tl_waits = &c->tally.waits;
    c->dictGen++;
    if (c->deviceOk && hipSetDevice(c->device) == hipSuccess) cctx_async_drain(c);
    c->pfx = nullptr; c->pfxSize = 0;       // (a pending prefix is cancelled: ZSTD_clearAllDicts)
    c->cdict = nullptr;                     // (and a referenced CDict)
    c->own.dictFormatted = false; c->own.dictFull.clear(); c->own.dictWide.clear();
    if (dict == nullptr || dictSize == 0) { c->own.dictHost.clear(); c->dictDirty = true; return 0; }          /* "no dictionary" */
    if (dictSize > (size_t)1 << 30) return ZERR(kErrParameterUnsupported);
    u8 head[8] = {};
    const bool dev = is_device_ptr(dict);
    if (dev) { if (host_memcpy(head, dict, dictSize < 8 ? dictSize : 8, hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric); }
    else memcpy(head, dict, dictSize < 8 ? dictSize : 8);
    if (is_formatted_dictionary(head, dictSize)) {
        // ZSTD_loadZstdDictionary, U/ZstdCompress.cs:5402-5463: dictID + repcodes + content are used (see ZSTD_CCtx_s::dictHost)
        std::vector<u8> full(dictSize);
        if (dev) { if (host_memcpy(full.data(), dict, dictSize, hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric); }
        else memcpy(full.data(), dict, dictSize);
        c->own.dictFull.swap(full); c->own.dictHost.clear(); c->own.dictFormatted = true; c->dictDirty = true;
        if (!isErr(cctx_bind(c))) return cctx_sync_dictionary(c);          // validated now when a device is there, else at first use
        return 0;
    }
    const size_t keep = dictSize < kDictKeep ? dictSize : kDictKeep;
    std::vector<u8> h(dictSize < 8 ? dictSize : keep);
    const u8* tail = (const u8*)dict + (dictSize - h.size());
    if (dev) { if (host_memcpy(h.data(), tail, h.size(), hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric); }
    else memcpy(h.data(), tail, h.size());
    c->own.dictHost.swap(h);
    if (dictSize >= 8) {        // what an index would cover (ZSTDMI_CCtx_setDictIndex, before or after this load)
        std::vector<u8> wide(dictSize < dict_index_max() ? dictSize : dict_index_max());
        const u8* from = (const u8*)dict + (dictSize - wide.size());
        if (dev) { if (host_memcpy(wide.data(), from, wide.size(), hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric); }
        else memcpy(wide.data(), from, wide.size());
        c->own.dictWide.swap(wide);
    }
    c->dictDirty = true;
    return 0;
}

size_t ZSTD_compressBound(size_t n) { return n + (n >> 8) + (n < (128u << 10) ? (((128u << 10) - n) >> 11) : 0); }

static size_t ZSTDMI_compressDevice_impl(ZSTD_CCtx* c, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize)
{
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    c->lastRegionList = nullptr; c->lastCarryGroups = 0;
    if (srcSize && !d_src) return ZERR(kErrSrcSizeWrong);
    if (!d_dst && dstCapacity) return ZERR(kErrDstBufferNull);
    if (!d_dst) return ZERR(kErrDstSizeTooSmall);
    if (c->workers.size() > 1 && c->seekTable) return ZERR(kErrParameterUnsupported);       // (the workers' shares have no common table)
    { const size_t e2 = check_single_frame(c, sticky_params(c), srcSize); if (isErr(e2)) return e2; }
    if (c->workers.size() > 1 && srcSize) return compress_multi(c, sticky_params(c), d_dst, dstCapacity, d_src, srcSize);
    return compress_device(c, sticky_params(c), (u8*)d_dst, dstCapacity, (const u8*)d_src, srcSize);
}

static size_t compress_any(ZSTD_CCtx* c, const CallParams& cp, void* dst, size_t dstCapacity, const void* src, size_t srcSize)
{
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    c->lastRegionList = nullptr;        // (ZSTDMI_debugLastRegionChunks speaks of this call from here on)
    c->lastCarryGroups = 0;             // (and ZSTDMI_debugLastCarryGroups)
    if (srcSize && !src) return ZERR(kErrSrcSizeWrong);
    if (!dst) return ZERR(kErrDstSizeTooSmall);
    if (c->workers.size() > 1 && cp.seek) return ZERR(kErrParameterUnsupported);
    { const size_t e2 = check_single_frame(c, cp, srcSize); if (isErr(e2)) return e2; }
    if (c->workers.size() > 1 && srcSize) return compress_multi(c, cp, dst, dstCapacity, src, srcSize);
    const bool srcDev = srcSize ? is_device_ptr(src) : true, dstDev = is_device_ptr(dst);
    const u8* d_src = (const u8*)src; u8* d_dst = (u8*)dst;
    size_t devCap = dstCapacity;
    if (!srcDev) {
        if (!c->stageSrc.ensure(srcSize + 64)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(c->stageSrc.p, src, srcSize, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
        d_src = (const u8*)c->stageSrc.p;
    }
    if (!dstDev) {
        const size_t worst = ZSTD_compressBound(srcSize) + 32 + (cp.seek ? seek_table_bound(srcSize) : 0);
        devCap = dstCapacity < worst ? dstCapacity : worst;
        if (!c->stageDst.ensure(devCap + 64)) return ZERR(kErrMemoryAllocation);
        d_dst = (u8*)c->stageDst.p;
    }
    const size_t r = compress_device(c, cp, d_dst, devCap, d_src, srcSize);
    if (isErr(r)) return r;
    if (!dstDev) {
        if (hipMemcpyAsync(dst, d_dst, r, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return ZERR(kErrGeneric);
        count_wait();
        if (hipStreamSynchronize(c->stream) != hipSuccess) return ZERR(kErrGeneric);      // (deliberately not stream_wait: no hipGetLastError behind this wait)
    }
    return r;
}

// ZSTD_CCtx_refPrefix (U/ZstdCompress.cs:1723-1765): raw content in front of ONE frame, referenced and used once.
// The call with a pending prefix.  Under 8 bytes: ignored (U/ZstdCompress.cs:5465-5503).  Short form — the prefix rounded up to 4 KiB
// and the source fit one 64 KiB block —: the path of ZSTD_CCtx_loadDictionary(the same raw bytes), which writes one frame with the
// prefix's last 60 KiB as LDS history.  Long form: one frame of the LDM framing's blocks whose long-distance stage indexes prefix and
// source as one window (ldm.hip); the block finders see no prefix.  What the long form cannot do is refused before a byte is read.
static size_t compress_prefixed(ZSTD_CCtx* c, void* dst, size_t dstCapacity, const void* src, size_t srcSize, bool deviceCall)
{
    const void* const pfx = c->pfx; const size_t pfxSize = c->pfxSize;
    c->pfx = nullptr; c->pfxSize = 0;       // consumed, whatever this call returns (the reference consumes it at frame start)
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    c->lastRegionList = nullptr; c->lastCarryGroups = 0;
    CallParams cp = sticky_params(c);
    auto plain = [&]() { return deviceCall ? ZSTDMI_compressDevice_impl(c, dst, dstCapacity, src, srcSize) : compress_any(c, cp, dst, dstCapacity, src, srcSize); };
    if (pfxSize < 8) return plain();
    if (cp.seek || c->workers.size() > 1) return ZERR(kErrParameterUnsupported);
    if (srcSize && !src) return ZERR(kErrSrcSizeWrong);
    if (!dst) return dstCapacity && deviceCall ? ZERR(kErrDstBufferNull) : ZERR(kErrDstSizeTooSmall);
    if (srcSize == 0) return plain();       // (the empty frame holds no match)
    if (pfxSize <= kChunkSize && (size_t)round_tile(pfxSize) + srcSize <= kChunkSize) {
        const size_t keep = pfxSize < kDictKeep ? pfxSize : kDictKeep;
        std::vector<u8> h(keep);
        if (host_memcpy(h.data(), (const u8*)pfx + (pfxSize - keep), keep, hipMemcpyDefault) != hipSuccess) { (void)hipGetLastError(); return ZERR(kErrGeneric); }
        c->own.dictHost.swap(h); c->own.dictFormatted = false; c->dictDirty = true; c->dictGen++;
        const size_t r = plain();
        c->own.dictHost.clear(); c->dictDirty = true; c->dictGen++;
        return r;
    }
    { const size_t e2 = check_call_params(cp); if (isErr(e2)) return e2; }
    if (cp.ldm == ZSTD_ps_disable || !cp.contentSizeFlag) return ZERR(kErrParameterUnsupported);
    if ((u64)pfxSize + srcSize > (cp.farOffsets ? kFarMaxSpan : kLdmMaxFrame)) return ZERR(kErrParameterUnsupported);       // (offsets of 2^29 and more: only with ZSTDMI_CCtx_setFarOffsets)
    if (cp.windowLog && cp.windowLog < 31 && ((u64)1 << cp.windowLog) < (u64)pfxSize + srcSize) return ZERR(kErrParameterUnsupported);
    cp.pfxSize = pfxSize;
    { const Framing fr = resolve_framing(c, cp, srcSize); if ((srcSize + fr.chunkBytes - 1) / fr.chunkBytes > c->passChunks) return ZERR(kErrParameterUnsupported); }
    if (is_device_ptr(pfx)) cp.pfx = (const u8*)pfx;
    else {
        if (!c->pfxStage.ensure(pfxSize + 64)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(c->pfxStage.p, pfx, pfxSize, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
        cp.pfx = (const u8*)c->pfxStage.p;
    }
    if (deviceCall) return compress_device(c, cp, (u8*)dst, dstCapacity, (const u8*)src, srcSize);
    return compress_any(c, cp, dst, dstCapacity, src, srcSize);
}
static size_t ZSTD_CCtx_refPrefix_impl(ZSTD_CCtx* c, const void* prefix, size_t prefixSize)
{
    if (!c) return ZERR(kErrGeneric);
    if (!c->sIn.empty() || c->sEnding) return ZERR(kErrStageWrong);
    if (prefix && prefixSize > (size_t)1 << 30) return ZERR(kErrParameterUnsupported);
    // ZSTD_clearAllDicts: a loaded dictionary, a referenced CDict and an earlier prefix are gone
    c->cdict = nullptr;
    c->dictGen++; c->own.dictFormatted = false; c->own.dictFull.clear(); c->own.dictHost.clear(); c->own.dictWide.clear(); c->dictDirty = true;
    c->pfx = nullptr; c->pfxSize = 0;
    if (prefix && prefixSize) { c->pfx = prefix; c->pfxSize = prefixSize; }
    return 0;
}

// ---------------- digested dictionaries (ZSTD_createCDict, U/ZstdCompress.cs:5984-6110; ZSTD_CCtx_refCDict, :1700) ----------------
// a dictionary's bytes (host memory) into a digest's host fields, as ZSTD_CCtx_loadDictionary files them
static void digest_set_bytes(DictDigest& g, const u8* b, size_t n)
{
    g.dictFormatted = false; g.dictFull.clear(); g.dictWide.clear(); g.dictHost.clear(); g.info = DictInfo{};
    if (!n) return;
    if (is_formatted_dictionary(b, n)) { g.dictFull.assign(b, b + n); g.dictFormatted = true; return; }
    const size_t keep = n < 8 ? n : (n < kDictKeep ? n : kDictKeep);
    g.dictHost.assign(b + (n - keep), b + n);
    if (n >= 8) { const size_t wide = n < dict_index_max() ? n : dict_index_max(); g.dictWide.assign(b + (n - wide), b + n); }
}
static ZSTD_CDict* create_cdict(const void* dict, size_t dictSize, int level, int device)
{
    if ((dictSize && !dict) || dictSize > (size_t)1 << 30) return nullptr;
    if (device < 0 || device_count() <= device) return nullptr;       // no gfx950 device: no digest
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    ZSTD_CDict_s* cd = new (std::nothrow) ZSTD_CDict_s();
    if (!cd) return nullptr;
    if (level < ZSTD_minCLevel()) level = ZSTD_minCLevel();
    if (level > ZSTD_maxCLevel()) level = ZSTD_maxCLevel();
    cd->level = level == 0 ? 3 : level; cd->device = device;            // (0 means the default level, U/ZstdCompress.cs:5991)
    bool ok = true;
    hipStream_t s = nullptr;
    try {       // (host containers may throw: nothing of a half-made CDict is left behind)
        std::vector<u8> bytes(dictSize);
        if (dictSize && host_memcpy(bytes.data(), dict, dictSize, hipMemcpyDefault) != hipSuccess) { (void)hipGetLastError(); ok = false; }
        if (ok) digest_set_bytes(cd->dg, bytes.data(), dictSize);
        // whole, on a stream of its own, waited for: every table any switch of a context can ask for
        if (ok && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); s = nullptr; ok = false; }
        if (ok) ok = !isErr(digest_upload(cd->dg, s, true, true, true)) && !isErr(stream_wait(s));
    } catch (...) { ok = false; }
    if (s) (void)hipStreamDestroy(s);
    if (!ok) { cd->dg.release(); delete cd; return nullptr; }
    return cd;
}
ZSTD_CDict* ZSTDMI_createCDictOnDevice(const void* dict, size_t dictSize, int compressionLevel, int device) { return create_cdict(dict, dictSize, compressionLevel, device); }
ZSTD_CDict* ZSTD_createCDict(const void* dict, size_t dictSize, int compressionLevel) { return ZSTDMI_createCDictOnDevice(dict, dictSize, compressionLevel, 0); }
size_t ZSTD_freeCDict(ZSTD_CDict* cd)
{
    if (!cd) return 0;
    if (hipSetDevice(cd->device) == hipSuccess) cd->dg.release(); else (void)hipGetLastError();
    delete cd;
    return 0;
}
size_t ZSTD_sizeof_CDict(const ZSTD_CDict* cd) { return cd ? sizeof(*cd) + cd->dg.bytes() : 0; }
unsigned ZSTD_getDictID_fromCDict(const ZSTD_CDict* cd) { return (cd && cd->dg.dictFormatted) ? cd->dg.info.dictID : 0u; }

// The context's own digest follows its reference: empty while the CDict's device copies are shared, a private copy of the CDict's host
// bytes (uploaded by the next call, exactly as after ZSTD_CCtx_loadDictionary) while they cannot be.  Touches no device.
static void cctx_adopt_cdict(ZSTD_CCtx* c)
{
    c->dictGen++; c->dictDirty = true;
    DictDigest& g = c->own;
    g.dictFormatted = false; g.dictFull.clear(); g.dictHost.clear(); g.dictWide.clear();
    if (!c->cdict || cdict_shared(c)) return;
    const DictDigest& from = c->cdict->dg;
    g.dictFormatted = from.dictFormatted; g.dictFull = from.dictFull; g.dictHost = from.dictHost; g.dictWide = from.dictWide; g.info = from.info;
}
size_t ZSTD_CCtx_refCDict(ZSTD_CCtx* c, const ZSTD_CDict* cdict)
{
    if (!c) return ZERR(kErrGeneric);
    if (!c->sIn.empty() || c->sEnding) return ZERR(kErrStageWrong);
    return guarded([&]() -> size_t {
        cctx_async_drain(c);
        c->pfx = nullptr; c->pfxSize = 0;       // ZSTD_clearAllDicts: a loaded dictionary and a pending prefix are gone
        c->cdict = cdict;
        cctx_adopt_cdict(c);
        return 0;
    });
}
// run() with `cdict` in force as after ZSTD_CCtx_refCDict (null: no dictionary at all); then the context's own dictionary or reference
// is back.  Where the CDict cannot be shared, its host fields stand in for the context's and are uploaded again by their next use.
extern "C++" { template <class F> static size_t under_cdict(ZSTD_CCtx* c, const ZSTD_CDict_s* cdict, F run)
{
    const ZSTD_CDict_s* const was = c->cdict;
    c->cdict = cdict;
    if (cdict_shared(c)) {
        size_t r;
        try { r = run(); } catch (...) { c->cdict = was; throw; }      // (the entry point's guarded() names the error)
        c->cdict = was;
        return r;
    }
    DictDigest& g = c->own;
    std::vector<u8> h, f, w; const bool fmt = g.dictFormatted; const DictInfo info = g.info;
    h.swap(g.dictHost); f.swap(g.dictFull); w.swap(g.dictWide);
    size_t r;
    try { cctx_adopt_cdict(c); r = run(); }
    catch (...) { r = ZERR(kErrMemoryAllocation); }
    g.dictHost.swap(h); g.dictFull.swap(f); g.dictWide.swap(w); g.dictFormatted = fmt; g.info = info;
    c->cdict = was; c->dictDirty = true; c->dictGen++;
    return r;
} }
size_t ZSTD_compress_usingCDict(ZSTD_CCtx* c, void* dst, size_t dstCapacity, const void* src, size_t srcSize, const ZSTD_CDict* cdict)
{
    if (!c || !cdict) return ZERR(kErrGeneric);
    // the CDict's level, default frame parameters, the context's four dictionary switches; the context's own dictionary or reference
    // steps aside for the call (where the CDict cannot be shared, its host fields do, and are uploaded again by their next use)
    CallParams p; p.level = cdict->level; p.useDict = true;
    p.dictEntropy = c->dictEntropy != 0; p.dictIndex = c->dictIndex != 0; p.dictIndexStrategy = c->dictIndexStrategy; p.dictIndexChain = c->dictIndexChain != 0;
    return guarded([&]() -> size_t { return under_cdict(c, cdict, [&] { return c->contentCuts ? compress_cut(c, p, dst, dstCapacity, src, srcSize, false)
                                                                                              : compress_any(c, p, dst, dstCapacity, src, srcSize); }); });
}
long long ZSTDMI_debugDictUploads(const ZSTD_CCtx* c)
{
    if (!c) return -1;
    long long n = c->dictUploads;
    for (const ZSTD_CCtx* w : c->workers) n += w->dictUploads;
    return n;
}

size_t ZSTDMI_compressDevice(ZSTD_CCtx* c, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize)
{
    if (c && c->contentCuts) return guarded([&] { return compress_cut(c, sticky_params(c), d_dst, dstCapacity, d_src, srcSize, true); });     // (a pending prefix: refused there, and stays pending)
    if (c && c->pfx) return guarded([&] { return compress_prefixed(c, d_dst, dstCapacity, d_src, srcSize, true); });
    return guarded([&] { return ZSTDMI_compressDevice_impl(c, d_dst, dstCapacity, d_src, srcSize); });
}
size_t ZSTD_compress2(ZSTD_CCtx* c, void* dst, size_t dstCapacity, const void* src, size_t srcSize)
{
    if (!c) return ZERR(kErrGeneric);
    if (c->contentCuts) return guarded([&] { return compress_cut(c, sticky_params(c), dst, dstCapacity, src, srcSize, false); });
    if (c->pfx) return guarded([&] { return compress_prefixed(c, dst, dstCapacity, src, srcSize, false); });
    return guarded([&] { return compress_any(c, sticky_params(c), dst, dstCapacity, src, srcSize); });
}
size_t ZSTD_CCtx_refPrefix(ZSTD_CCtx* c, const void* prefix, size_t prefixSize) { return guarded([&] { return ZSTD_CCtx_refPrefix_impl(c, prefix, prefixSize); }); }

size_t ZSTD_compressCCtx(ZSTD_CCtx* c, void* dst, size_t dstCapacity, const void* src, size_t srcSize, int level)
{
    if (!c) return ZERR(kErrGeneric);
    // ZSTD_compressCCtx = ZSTD_compress_usingDict(dict = NULL, level) (U/ZstdCompress.cs:5751-5776): the level alone, default
    // frame parameters (content size, no checksum), NO dictionary even if one is loaded; the context's sticky parameters and
    // its dictionary stay as they are for later ZSTD_compress2 calls.
    CallParams p; p.level = level == 0 ? 3 : (level < ZSTD_minCLevel() ? ZSTD_minCLevel() : level > ZSTD_maxCLevel() ? ZSTD_maxCLevel() : level);
    p.useDict = false;
    return guarded([&] { return compress_any(c, p, dst, dstCapacity, src, srcSize); });
}

/* S/CompressionStream.cs:41, S/DecompressionStream.cs:41 size their buffers with these (U/ZstdCompress.cs:6241-6249,
 * U/ZstdDecompress.cs:2096-2104): one block in, one compressed block + header + checksum out */
size_t ZSTD_CStreamInSize(void)  { return (size_t)1 << 17; }
size_t ZSTD_CStreamOutSize(void) { return ZSTD_compressBound((size_t)1 << 17) + 3 + 4; }
size_t ZSTD_DStreamInSize(void)  { return ((size_t)1 << 17) + 3; }
size_t ZSTD_DStreamOutSize(void) { return (size_t)1 << 17; }

// ---------------- several devices behind one context (SURVEY.md section 8 e; ZSTDMI_*_setDevices) ----------------
// north_star: "chunks partition naturally across the 8 GPUs of one node".  Frames are the independent unit (a match never leaves its
// frame), so a call's frames are dealt to the device workers in contiguous shares: every worker stages its share on its own device,
// compresses it with the kernels above on its own stream, from a host thread of its own, and the shares' outputs are copied into the
// caller's buffer one behind the other.  What is written does not depend on the number of workers: shares are cut on frame
// boundaries (on probe-group boundaries when the sparse-input probe runs), parameters are resolved for the whole range, and the probe's
// plan is made once over all shares' counts.  No collective: the only exchange is the final copy (device to host, or peer to peer).
static size_t compress_multi(ZSTD_CCtx* c, const CallParams& cp, void* dst, size_t dstCapacity, const void* src, size_t srcSize)
{
    { const size_t e = check_call_params(cp); if (isErr(e)) return e; }
    { const size_t e = check_ldm_dict(c, cp, srcSize); if (isErr(e)) return e; }
    const size_t W = c->workers.size();
    for (ZSTD_CCtx* w : c->workers) { w->lastRegionList = nullptr; w->lastCarryGroups = 0; }
    bool ok = true;
    // the workers run with the parent's settings and dictionary
    if (cp.useDict) { const size_t e = cctx_sync_dictionary(c); if (isErr(e)) return e; }
    for (ZSTD_CCtx* w : c->workers) {
        w->historyBytes = c->historyBytes; w->frameBytes = c->frameBytes; w->parser = c->parser; w->passChunks = c->passChunks; w->timer.enabled = c->timer.enabled;
        w->dictEntropy = c->dictEntropy;        // (before the dictionary: a worker builds the tables when it uploads its copy)
        w->entropyCarry = c->entropyCarry;
        w->farOffsets = c->farOffsets;
        w->dictIndex = c->dictIndex; w->dictIndexStrategy = c->dictIndexStrategy; w->dictIndexChain = c->dictIndexChain;       // (and the index, as far up the strategies as the parent's)
        if (w->dictGen != c->dictGen) {
            w->own.dictHost = c->own.dictHost; w->own.dictFull = c->own.dictFull; w->own.dictWide = c->own.dictWide; w->own.dictFormatted = c->own.dictFormatted; w->own.info = c->own.info; w->dictDirty = true; w->dictGen = c->dictGen;
        }
    }
    size_t err = 0;
    ZSTD_CCtx* const w0 = c->workers[0];
    { const size_t e = cctx_bind(w0); if (isErr(e)) return e; }
    if (cp.useDict) { const size_t e = cctx_sync_dictionary(w0); if (isErr(e)) return e; }
    const size_t group = probe_group_bytes(w0, cp, srcSize, err);
    if (isErr(err)) return err;
    // shares: whole probe groups, or whole frames of the one range
    const size_t unit = group ? group : resolve_framing(w0, cp, srcSize).span();
    const size_t nUnits = (srcSize + unit - 1) / unit;
    std::vector<size_t> lo(W + 1);
    for (size_t i = 0; i <= W; ++i) { const size_t u = nUnits * i / W; lo[i] = u * unit < srcSize ? u * unit : srcSize; }
    lo[W] = srcSize;
    std::vector<size_t> res(W, 0), front(W, 0);
    std::vector<u32> counts(group ? (srcSize + group - 1) / group : 0);
    // phase A: every worker stages its share (with the probe's 60 KiB window in front of it) and, if the call is probed, counts its groups
    ok = run_on_workers(W, [&](size_t i) {
        ZSTD_CCtx* w = c->workers[i];
        size_t e = cctx_bind(w); if (isErr(e)) { res[i] = e; return; }
        const size_t n = lo[i + 1] - lo[i];
        if (!n) return;
        front[i] = group ? (lo[i] < (60u << 10) ? lo[i] : (60u << 10)) : 0;
        if (!w->stageSrc.ensure(front[i] + n + 64) || !w->stageDst.ensure(ZSTD_compressBound(n) + (n / unit + 2) * 64 + 64)) { res[i] = ZERR(kErrMemoryAllocation); return; }
        e = copy_any(w->stageSrc.p, (const u8*)src + lo[i] - front[i], front[i] + n, w->stream); if (isErr(e)) { res[i] = e; return; }
        if (group) { e = probe_run(w, (const u8*)w->stageSrc.p + front[i], n, front[i], group, counts.data() + lo[i] / group); if (isErr(e)) res[i] = e; }
    });
    if (!ok) return ZERR(kErrMemoryAllocation);
    for (size_t i = 0; i < W; ++i) if (isErr(res[i])) return res[i];
    std::vector<PlanRange> plan;
    if (group) plan_ranges(counts, group, srcSize, plan);
    else { PlanRange r; r.off = 0; r.len = srcSize; r.sparse = false; plan.push_back(r); }
    CallParams cpSparse = cp; cpSparse.level = 1;
    // phase B: every worker compresses what the plan's ranges hold of its share (parameters resolved for the whole call, as one device does)
    std::vector<size_t> produced(W, 0);
    ok = run_on_workers(W, [&](size_t i) {
        ZSTD_CCtx* w = c->workers[i];
        if (isErr(cctx_bind(w))) return;
        bool first = true;
        std::vector<PlanRange> part;
        for (const PlanRange& r : plan) {
            const size_t a = r.off > lo[i] ? r.off : lo[i], b = (r.off + r.len) < lo[i + 1] ? (r.off + r.len) : lo[i + 1];
            if (a < b) { PlanRange q; q.off = a - lo[i]; q.len = b - a; q.sparse = r.sparse; part.push_back(q); }
        }
        if (part.empty()) return;
        const u8* base = (const u8*)w->stageSrc.p + front[i];
        size_t n;
        if (part.size() == 1) n = compress_range(w, part[0].sparse ? cpSparse : cp, (u8*)w->stageDst.p, w->stageDst.cap, base + part[0].off, part[0].len, srcSize, first);
        else n = compress_plan(w, cp, part, srcSize, (u8*)w->stageDst.p, w->stageDst.cap, base, first);
        if (isErr(n)) { res[i] = n; return; }
        produced[i] = n;
    });
    if (!ok) return ZERR(kErrMemoryAllocation);
    for (size_t i = 0; i < W; ++i) if (isErr(res[i])) return res[i];
    size_t total = 0;
    for (size_t i = 0; i < W; ++i) total += produced[i];
    if (total > dstCapacity) return ZERR(kErrDstSizeTooSmall);
    // the shares, one behind the other, into the caller's buffer (host: device-to-host copies side by side; device: peer copies)
    std::vector<size_t> at(W, 0);
    for (size_t i = 1; i < W; ++i) at[i] = at[i - 1] + produced[i - 1];
    ok = run_on_workers(W, [&](size_t i) {
        ZSTD_CCtx* w = c->workers[i];
        if (isErr(cctx_bind(w))) return;
        size_t e = copy_any((u8*)dst + at[i], w->stageDst.p, produced[i], w->stream);
        if (!isErr(e)) e = stream_wait(w->stream);
        if (isErr(e)) res[i] = e;
    });
    if (!ok) return ZERR(kErrMemoryAllocation);
    for (size_t i = 0; i < W; ++i) if (isErr(res[i])) return res[i];
    // stage times: the first worker's (every worker runs the same sequence over its share)
    c->nStages = w0->nStages;
    for (int i = 0; i < w0->nStages; i++) { c->stageMs[i] = w0->stageMs[i]; c->stageNames[i] = w0->stageNames[i]; }
    c->lastChunks = 0;
    (void)cctx_bind(c);
    return total;
}

// ---------------- errors ----------------
unsigned ZSTD_isError(size_t code) { return isErr(code); }
const char* ZSTD_getErrorName(size_t code)
{
    if (!isErr(code)) return "No error detected";
    switch ((u32)(0 - code)) {          // strings as U/ErrorPrivate.cs:35-180
    case kErrGeneric: return "Error (generic)";
    case kErrPrefixUnknown: return "Unknown frame descriptor";
    case kErrVersionUnsupported: return "Version not supported";
    case kErrFrameParameterUnsupported: return "Unsupported frame parameter";
    case kErrWindowTooLarge: return "Frame requires too much memory for decoding";
    case kErrCorruption: return "Corrupted block detected";
    case kErrChecksumWrong: return "Restored data doesn't match checksum";
    case kErrParameterUnsupported: return "Unsupported parameter";
    case kErrParameterOutOfBound: return "Parameter is out of bound";
    case kErrInitMissing: return "Context should be init first";
    case kErrMemoryAllocation: return "Allocation error : not enough memory";
    case kErrWorkSpaceTooSmall: return "workSpace buffer is not large enough";
    case kErrStageWrong: return "Operation not authorized at current processing stage";
    case kErrTableLogTooLarge: return "tableLog requires too much memory : unsupported";
    case kErrMaxSymbolValueTooLarge: return "Unsupported max Symbol Value : too large";
    case kErrMaxSymbolValueTooSmall: return "Specified maxSymbolValue is too small";
    case kErrDictionaryCorrupted: return "Dictionary is corrupted";
    case kErrDictionaryWrong: return "Dictionary mismatch";
    case 34: return "Cannot create Dictionary from provided samples";
    case kErrDstSizeTooSmall: return "Destination buffer is too small";
    case kErrSrcSizeWrong: return "Src size is incorrect";
    case kErrDstBufferNull: return "Operation on NULL destination buffer";
    case 100: return "Frame index is too large";
    case 102: return "An I/O error occurred when reading/seeking";
    case 104: return "Destination buffer is wrong";
    case 105: return "Source buffer is wrong";
    default: return "Unspecified error code";
    }
}
/* S/ThrowHelper.cs:18-24 (EnsureZdictSuccess) -> U/Zdict.cs:11-19: the dictionary builder's error helpers are the common ones */
unsigned ZDICT_isError(size_t code) { return isErr(code); }
const char* ZDICT_getErrorName(size_t code) { return ZSTD_getErrorName(code); }
unsigned ZSTD_versionNumber(void) { return 10501; }
const char* ZSTD_versionString(void) { return "1.5.1"; }

// ---------------- streaming adapters on the batched engine ----------------
// ZSTD_compressStream2 (S/Compressor.cs:108-116 <- S/CompressionStream.cs:130-190; U/ZstdCompress.cs:6632-6861).
// Input is buffered on the host until a batch (16 MiB) is full or the caller flushes/ends; each batch goes through the
// one-shot pipeline and comes back as complete, independent 64 KiB frames, so a flush point is a frame boundary and the
// concatenation of everything emitted is one ordinary multi-frame zstd stream.  Return value as the reference's: for
// e_flush / e_end the number of bytes still to be flushed (0 = done), for e_continue a non-zero hint.
static size_t cstream_drain(ZSTD_CCtx* c, ZSTD_outBuffer* o)
{
    const size_t avail = c->sOut.size() - c->sOutPos, room = o->size - o->pos;
    const size_t n = avail < room ? avail : room;
    if (n) { memcpy((u8*)o->dst + o->pos, c->sOut.data() + c->sOutPos, n); o->pos += n; c->sOutPos += n; }
    if (c->sOutPos == c->sOut.size()) { c->sOut.clear(); c->sOutPos = 0; }
    return c->sOut.size() - c->sOutPos;
}
static size_t cstream_compress(ZSTD_CCtx* c, size_t n)      // first n buffered bytes -> appended to sOut
{
    const size_t cap = ZSTD_compressBound(n), at = c->sOut.size();
    c->sOut.resize(at + cap);
    const size_t r = ZSTD_compress2(c, c->sOut.data() + at, cap, c->sIn.data(), n);
    if (isErr(r)) { c->sOut.resize(at); return r; }
    c->sOut.resize(at + r);
    c->sIn.erase(c->sIn.begin(), c->sIn.begin() + (ptrdiff_t)n);
    return 0;
}
// A batch of a single-frame session (ZSTDMI_CCtx_setSingleFrame): the first n buffered bytes continue the session's ONE frame.  The last
// kStreamTail bytes the frame already holds go up in front of the batch, so its first block has its history where every other
// block finds it: in front of itself.  The first batch writes the header (a window descriptor, no content size), the batch of
// ZSTD_e_end sets Last_Block and appends the checksum.
static size_t cstream_compress_single(ZSTD_CCtx* c, size_t n, bool ending)
{
    CallParams cp = sticky_params(c);
    cp.single = true; cp.stream = true; cp.streamAt = c->sTotal; cp.streamEnd = ending; cp.seek = false; cp.checksumFlag = c->sChecksum;
    cp.sliding = false;     // (a session that did not begin with a sliding window has none: the refusal stands)
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    e = check_call_params(cp); if (isErr(e)) return e;
    e = check_single_frame(c, cp, n); if (isErr(e)) return e;
    if (c->sTotal + n > kSingleMax) return ZERR(kErrParameterUnsupported);
    const size_t tail = c->sTail.size(), pad = (256 - tail % 256) % 256;       // (the batch itself begins 256-byte aligned)
    const size_t cap = ZSTD_compressBound(n) + 32;
    if (!c->stageSrc.ensure(pad + tail + n + 64) || !c->stageDst.ensure(cap + 64)) return ZERR(kErrMemoryAllocation);
    u8* const d_src = (u8*)c->stageSrc.p + pad + tail;
    if (tail && hipMemcpyAsync(d_src - tail, c->sTail.data(), tail, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
    if (hipMemcpyAsync(d_src, c->sIn.data(), n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
    bool first = true;
    c->lastCarryGroups = 0;
    const size_t r = compress_range(c, cp, (u8*)c->stageDst.p, cap, d_src, n, kStreamParamSize, first);
    if (isErr(r)) return r;
    const size_t at = c->sOut.size();
    c->sOut.resize(at + r);
    if (isErr(dev_read(c->sOut.data() + at, c->stageDst.p, r, c->stream))) { c->sOut.resize(at); return ZERR(kErrGeneric); }
    c->sTail.insert(c->sTail.end(), c->sIn.begin(), c->sIn.begin() + (ptrdiff_t)n);
    if (c->sTail.size() > kStreamTail) c->sTail.erase(c->sTail.begin(), c->sTail.end() - (ptrdiff_t)kStreamTail);
    c->sTotal += n;
    c->sIn.erase(c->sIn.begin(), c->sIn.begin() + (ptrdiff_t)n);
    return 0;
}
// The same for a session whose long-distance window slides (ZSTDMI_CCtx_setSlidingLdm; sSliding): the frame's latest content stays on
// the device, in sWin, and a batch is appended to it, so that the 2^sSlideLog bytes in front of the batch (the stage's window, and the
// finders' history with them) lie in front of it where compress_range reads them.  sWin holds the window, one batch and kSlideSlack
// bytes more.  When the next batch does not fit, the window's bytes are moved to the front: a left shift by more than kSlideSlack, done
// as device-to-device copies of at most the shift's length each, front to back on the one stream, so that no copy overlaps itself
// (at most 2^sSlideLog / kSlideSlack + 1 of them, and only once per kSlideSlack bytes of input).  A batch is at most sBatch bytes:
// more is cut, which a session without the switch does not do.
constexpr size_t kSlideSlack = (size_t)4 << 20;
static CallParams sliding_session_params(const ZSTD_CCtx* c)
{
    CallParams cp = sticky_params(c);
    cp.single = true; cp.stream = true; cp.seek = false; cp.checksumFlag = c->sChecksum;
    cp.sliding = true; cp.ldm = 1; cp.windowLog = c->sSlideLog;         // (what the session noted when it began)
    return cp;
}
static size_t cstream_compress_sliding(ZSTD_CCtx* c, size_t n, bool ending)
{
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    const size_t win = (size_t)1 << c->sSlideLog, room = win + c->sBatch + kSlideSlack;
    while (n) {
        const size_t m = n < c->sBatch ? n : c->sBatch;
        CallParams cp = sliding_session_params(c);
        cp.streamAt = c->sTotal; cp.streamEnd = ending && m == n;
        e = check_call_params(cp); if (isErr(e)) return e;
        e = check_single_frame(c, cp, m); if (isErr(e)) return e;
        if (c->sTotal + m > kSingleMax) return ZERR(kErrParameterUnsupported);
        const size_t cap = ZSTD_compressBound(m) + 32;
        if (c->sTotal == 0) { c->sWinFill = 0; if (!c->sWin.ensure(room + 64)) return ZERR(kErrMemoryAllocation); }      // (allocated by the session's first batch)
        if (!c->sWin.p || c->sWin.cap < room + 64) return ZERR(kErrGeneric);
        if (!c->stageDst.ensure(cap + 64)) return ZERR(kErrMemoryAllocation);
        u8* const w = (u8*)c->sWin.p;
        if (c->sWinFill + m > room) {       // roll: the last `win` bytes to the front (sWinFill > win + kSlideSlack here)
            const size_t shift = c->sWinFill - win;
            for (size_t at = 0; at < win; at += shift) {
                const size_t len = win - at < shift ? win - at : shift;
                if (hipMemcpyAsync(w + at, w + at + shift, len, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
            }
            c->sWinFill = win;
        }
        u8* const d_src = w + c->sWinFill;
        if (hipMemcpyAsync(d_src, c->sIn.data(), m, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
        bool first = true;
        c->lastCarryGroups = 0;
        const size_t r = compress_range(c, cp, (u8*)c->stageDst.p, cap, d_src, m, kStreamParamSize, first);
        if (isErr(r)) return r;
        const size_t at = c->sOut.size();
        c->sOut.resize(at + r);
        if (isErr(dev_read(c->sOut.data() + at, c->stageDst.p, r, c->stream))) { c->sOut.resize(at); return ZERR(kErrGeneric); }
        c->sWinFill += m; c->sTotal += m;
        c->sIn.erase(c->sIn.begin(), c->sIn.begin() + (ptrdiff_t)m);
        n -= m;
    }
    return 0;
}
// ZSTD_e_end with nothing buffered behind earlier batches: an empty raw last block, and the checksum of what the frame holds
static size_t cstream_end_single(ZSTD_CCtx* c)
{
    u8 f[7] = { 1, 0, 0 }; size_t n = 3;
    if (c->sChecksum) {
        size_t e = cctx_bind(c); if (isErr(e)) return e;
        u32 h = 0;
        launch_stream_xxh((XxhCarry*)c->sfXxh.p, (const u8*)c->sfXxh.p, 0, 1, c->stream);
        if (isErr(dev_read(&h, (const u8*)c->sfXxh.p + offsetof(XxhCarry, hash), sizeof h, c->stream))) return ZERR(kErrGeneric);
        for (u32 i = 0; i < 4; ++i) f[n++] = (u8)(h >> (8 * i));
    }
    c->sOut.insert(c->sOut.end(), f, f + n);
    return 0;
}
static size_t ZSTD_compressStream2_impl(ZSTD_CCtx* c, ZSTD_outBuffer* output, ZSTD_inBuffer* input, int endOp)
{
    if (!c || !output || !input) return ZERR(kErrGeneric);
    if (output->pos > output->size) return ZERR(104);          // dstBuffer_wrong
    if (input->pos > input->size) return ZERR(105);            // srcBuffer_wrong
    if ((unsigned)endOp > 2) return ZERR(kErrParameterOutOfBound);
    if (c->seekTable) return ZERR(kErrParameterUnsupported);   // (a table per batch of the session would not be one table of the stream)
    if (c->contentCuts) return ZERR(kErrParameterUnsupported); // (cuts would have to carry across the session's batches)
    if (c->pfx) return ZERR(kErrParameterUnsupported);         // (a referenced prefix stands in front of ONE frame; a session writes one per batch)
    if (input->size > input->pos && !input->src) return ZERR(kErrSrcSizeWrong);
    if (output->size > output->pos && !output->dst) return ZERR(kErrDstBufferNull);
    if (cstream_drain(c, output)) return c->sOut.size() - c->sOutPos;       // output full: nothing consumed this time
    if (!c->sWrote && !c->sEnding && c->sIn.empty()) { c->sSingle = c->singleFrame != 0; c->sChecksum = c->checksumFlag; c->sTotal = 0; c->sTail.clear();      // a session begins
        c->sSliding = c->sSingle && c->slidingLdm && c->ldm == 1; c->sSlideLog = c->windowLog ? c->windowLog : kLdmDefaultWindowLog; c->sWinFill = 0; }
    if (c->sSingle && !c->sEnding) {    // what one frame per session cannot be: refused before anything is taken
        CallParams cp = sticky_params(c); cp.single = true; cp.stream = true; cp.seek = false; cp.sliding = false;
        if (c->sSliding) cp = sliding_session_params(c);
        const size_t e = check_single_frame(c, cp, 0); if (isErr(e)) return e;
    }
    if (!c->sEnding) {
        const size_t n = input->size - input->pos;
        if (n) { c->sIn.insert(c->sIn.end(), (const u8*)input->src + input->pos, (const u8*)input->src + input->size); input->pos = input->size; c->sWrote = true; }
        size_t e = 0;
        if (endOp == 0) {                                      // ZSTD_e_continue: whole chunks only, so that frames stay 64 KiB
            if (c->sIn.size() >= c->sBatch) { const size_t whole = c->sIn.size() / kChunkSize * kChunkSize; e = c->sSliding ? cstream_compress_sliding(c, whole, false) : c->sSingle ? cstream_compress_single(c, whole, false) : cstream_compress(c, whole); }
        } else {
            if (!c->sIn.empty()) e = c->sSliding ? cstream_compress_sliding(c, c->sIn.size(), endOp == 2) : c->sSingle ? cstream_compress_single(c, c->sIn.size(), endOp == 2) : cstream_compress(c, c->sIn.size());     // (ZSTD_e_flush ends a block, not the frame)
            else if (endOp == 2 && c->sSingle && c->sTotal) e = cstream_end_single(c);
            else if (endOp == 2 && !c->sWrote) {               // ZSTD_e_end on an empty stream: the empty frame (U/ZstdCompress.cs:5598-5656)
                u8 tmp[16]; const size_t r = ZSTD_compress2(c, tmp, sizeof tmp, tmp, 0);
                if (isErr(r)) e = r; else c->sOut.insert(c->sOut.end(), tmp, tmp + r);
            }
            if (endOp == 2) c->sEnding = true;
        }
        if (isErr(e)) return e;
    }
    const size_t left = cstream_drain(c, output);
    if (c->sEnding && left == 0) { c->sEnding = false; c->sWrote = false; c->sTotal = 0; c->sTail.clear();      // frame session closed; the context may start another
        if (c->sSliding) { c->sSliding = false; c->sWinFill = 0; if (c->deviceOk && !isErr(cctx_bind(c))) c->sWin.release(); } }       // (and its device window goes with it)
    if (endOp == 0) return left ? left : (c->sBatch > c->sIn.size() ? c->sBatch - c->sIn.size() : 1);
    return left;
}

// ---------------- extensions ----------------
int ZSTDMI_deviceCount(void) { return device_count(); }
// (a referenced CDict is shared or copied by where the context runs: cctx_adopt_cdict)
size_t ZSTDMI_CCtx_setDevice(ZSTD_CCtx* c, int device) { if (c) { c->paramGen++; cctx_drop_cuts_prepare(c); } const size_t e = ctx_set_device(c, device); if (c && c->cdict) (void)guarded([&]() -> size_t { cctx_adopt_cdict(c); return 0; }); return e; }
size_t ZSTDMI_CCtx_setDevices(ZSTD_CCtx* c, const int* devices, int n)
{
    if (c) { c->paramGen++; cctx_drop_cuts_prepare(c); }
    const size_t e = ctx_set_devices(c, devices, n, ZSTD_createCCtx, ZSTD_freeCCtx);
    if (c && c->cdict) (void)guarded([&]() -> size_t { cctx_adopt_cdict(c); return 0; });
    return e;
}
size_t ZSTDMI_CCtx_setStream(ZSTD_CCtx* c, void* st)
{
    if (c && (st ? (hipStream_t)st : c->ownStream) != c->stream) cctx_async_drain(c);     // (the new stream is not ordered behind an enqueued batch)
    return ctx_set_stream(c, st, cctx_bind);
}
size_t ZSTDMI_CCtx_setPassChunks(ZSTD_CCtx* c, unsigned chunks) { if (!c || chunks == 0 || chunks > (1u << 20)) return ZERR(kErrParameterOutOfBound); c->passChunks = chunks; c->paramGen++; return 0; }
// bytes: 0 = independent 64 KiB frames; > 0 = cross-chunk history of that many bytes per block (rounded to 4 KiB, at most 48 KiB);
// < 0 = by level.  frameBytes: content of one multi-block frame (64 KiB .. 16 MiB), 0 = keep.
size_t ZSTDMI_CCtx_setHistory(ZSTD_CCtx* c, int bytes, unsigned frameBytes)
{
    if (!c || bytes > (48 << 10) || (frameBytes && (frameBytes < kChunkSize || frameBytes > (16u << 20)))) return ZERR(kErrParameterOutOfBound);
    c->historyBytes = bytes; if (frameBytes) c->frameBytes = frameBytes; c->paramGen++; return 0;
}
size_t ZSTDMI_CCtx_setSeekTable(ZSTD_CCtx* c, unsigned mode) { if (!c) return ZERR(kErrGeneric); if (mode > 1) return ZERR(kErrParameterOutOfBound); c->seekTable = (int)mode; c->paramGen++; return 0; }
// (no device is touched; what the switch cannot be combined with is refused by the call that would have to do it: check_single_frame)
size_t ZSTDMI_CCtx_setSingleFrame(ZSTD_CCtx* c, unsigned mode) { if (!c) return ZERR(kErrGeneric); if (mode > 1) return ZERR(kErrParameterOutOfBound); c->singleFrame = (int)mode; c->paramGen++; return 0; }
// (no device is touched; where the switch takes effect: sliding_active, and what it cannot be combined with: check_single_frame)
size_t ZSTDMI_CCtx_setFarOffsets(ZSTD_CCtx* c, unsigned mode) { if (!c) return ZERR(kErrGeneric); if (mode > 1) return ZERR(kErrParameterOutOfBound); c->farOffsets = (int)mode; c->paramGen++; return 0; }
size_t ZSTDMI_CCtx_setSlidingLdm(ZSTD_CCtx* c, unsigned mode) { if (!c) return ZERR(kErrGeneric); if (mode > 1) return ZERR(kErrParameterOutOfBound); c->slidingLdm = (int)mode; c->paramGen++; return 0; }
size_t ZSTDMI_seekTableBound(size_t srcSize) { return seek_table_bound(srcSize); }
// (no device is touched: a loaded formatted dictionary is marked for another upload, which builds — or no longer builds — its tables)
size_t ZSTDMI_CCtx_setDictEntropy(ZSTD_CCtx* c, unsigned mode)
{
    if (!c) return ZERR(kErrGeneric);
    if (mode > 1) return ZERR(kErrParameterOutOfBound);
    if (c->dictEntropy != (int)mode && c->own.dictFormatted) { c->dictDirty = true; c->dictGen++; }
    c->dictEntropy = (int)mode; c->paramGen++;
    return 0;
}
// (no device is touched: the switch is read by the next call, carry_active)
size_t ZSTDMI_CCtx_setEntropyCarry(ZSTD_CCtx* c, unsigned mode) { if (!c) return ZERR(kErrGeneric); if (mode > 1) return ZERR(kErrParameterOutOfBound); c->entropyCarry = (int)mode; c->paramGen++; return 0; }
long long ZSTDMI_debugLastCarryGroups(const ZSTD_CCtx* c)
{
    if (!c) return -1;
    if (c->workers.size() <= 1) return c->lastCarryGroups;
    long long n = 0;
    for (const ZSTD_CCtx* w : c->workers) n += w->lastCarryGroups;
    return n;
}
// (no device is touched: a loaded dictionary is marked for another upload, which builds — or no longer builds — its index)
size_t ZSTDMI_CCtx_setDictIndex(ZSTD_CCtx* c, unsigned mode)
{
    if (!c) return ZERR(kErrGeneric);
    if (mode > 1) return ZERR(kErrParameterOutOfBound);
    if (c->dictIndex != (int)mode && (c->own.dictFormatted || !c->own.dictWide.empty())) { c->dictDirty = true; c->dictGen++; }
    c->dictIndex = (int)mode; c->paramGen++;
    return 0;
}
// (no device is touched: with the index on, a loaded dictionary is marked for another upload, which builds — or no longer builds —
//  the dual finder's two tables; with it off nothing changes until it is turned on, and that setter marks the dictionary itself)
size_t ZSTDMI_CCtx_setDictIndexStrategy(ZSTD_CCtx* c, unsigned maxStrategy)
{
    if (!c) return ZERR(kErrGeneric);
    if (maxStrategy < 1 || maxStrategy > 2) return ZERR(kErrParameterOutOfBound);
    if (c->dictIndexStrategy != (int)maxStrategy && c->dictIndex && (c->own.dictFormatted || !c->own.dictWide.empty())) { c->dictDirty = true; c->dictGen++; }
    c->dictIndexStrategy = (int)maxStrategy; c->paramGen++;
    return 0;
}
// (no device is touched: with the index on, a loaded dictionary is marked for another upload, which builds — or, where
//  ZSTDMI_CCtx_setDictIndexStrategy does not ask for them either, no longer builds — the two tables the chain finder's search probes)
size_t ZSTDMI_CCtx_setDictIndexChain(ZSTD_CCtx* c, unsigned mode)
{
    if (!c) return ZERR(kErrGeneric);
    if (mode > 1) return ZERR(kErrParameterOutOfBound);
    if (c->dictIndexChain != (int)mode && c->dictIndex && (c->own.dictFormatted || !c->own.dictWide.empty())) { c->dictDirty = true; c->dictGen++; }
    c->dictIndexChain = (int)mode; c->paramGen++;
    return 0;
}
// chunks the last pass of the last compress call handed to lz_region_kernel: its work list's count, read back here
long long ZSTDMI_debugLastRegionChunks(const ZSTD_CCtx* c)
{
    if (!c) return -1;
    const ZSTD_CCtx* const w = c->workers.size() > 1 ? c->workers.back() : c;
    if (!w->lastRegionList || !w->deviceOk) return 0;
    int before = 0;
    if (hipGetDevice(&before) != hipSuccess || hipSetDevice(w->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    u32 count = 0;
    if (hipStreamSynchronize(w->stream) != hipSuccess || host_memcpy(&count, w->lastRegionList, sizeof count, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); count = 0; }
    (void)hipSetDevice(before);         // (a hook leaves the caller's current device where it was)
    return (long long)count;
}
long long ZSTDMI_debugDictIndexed(const ZSTD_CCtx* c) { return c ? (long long)dict_index_len(c) : -1; }
size_t ZSTDMI_CCtx_setParser(ZSTD_CCtx* c, unsigned mode) { if (!c || mode > 1) return ZERR(kErrParameterOutOfBound); c->parser = mode; c->paramGen++; return 0; }
size_t ZSTDMI_CCtx_setProfiling(ZSTD_CCtx* c, int en) { if (!c) return ZERR(kErrGeneric); c->timer.enabled = en != 0; return 0; }
int ZSTDMI_CCtx_getStageTimes(const ZSTD_CCtx* c, float* ms, const char** names, int cap)
{
    if (!c) return 0;
    int n = c->nStages < cap ? c->nStages : cap;
    for (int i = 0; i < n; i++) { if (ms) ms[i] = c->stageMs[i]; if (names) names[i] = c->stageNames[i]; }
    return n;
}

size_t ZSTDMI_debugLdmPass(ZSTD_CCtx* c, unsigned* pos, unsigned* mStart, unsigned* mLen, unsigned* mOff, size_t cap, size_t* nSplits, unsigned* base, unsigned* vlo)
{
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    if (!nSplits || !base || !vlo) return ZERR(kErrGeneric);
    if (c->workers.size() > 1 || !c->lastChunks || !c->ldmRecOk) return ZERR(kErrParameterUnsupported);
    const LdmRecord& r = c->ldmRec;
    *nSplits = r.nSplits; *base = c->ldmRecBase; *vlo = c->ldmRecVlo;
    const size_t k = r.nSplits < cap ? r.nSplits : cap;
    const struct { unsigned* to; const u32* from; } rows[4] = { { pos, r.splitPos }, { mStart, r.mStart }, { mLen, r.mLen }, { mOff, r.mOff } };
    for (const auto& row : rows)
        if (k && row.to && host_memcpy(row.to, row.from, k * sizeof(u32), hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric);
    // what lies in front of the pass is searched by no block: ldm_match writes nothing for those splits (they are candidates only)
    if (k && c->ldmRecBase) {
        std::vector<u32> p(k);
        if (host_memcpy(p.data(), r.splitPos, k * sizeof(u32), hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric);
        const size_t front = (size_t)(std::lower_bound(p.begin(), p.end(), c->ldmRecBase) - p.begin());
        for (unsigned* col : { mStart, mLen, mOff }) if (col) std::fill(col, col + front, 0u);
    }
    return 0;
}
size_t ZSTDMI_debugLdmSkipMerge(ZSTD_CCtx* c, int on) { if (!c) return ZERR(kErrGeneric); c->ldmSkipMerge = on != 0; return 0; }

size_t ZSTDMI_debugGetChunk(ZSTD_CCtx* c, size_t chunkIdx, ZSTDMI_Seq* seqs, size_t seqCap, size_t* nbSeq, void* lits, size_t litCap, size_t* litSize)
{
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    if (chunkIdx >= c->lastChunks) return ZERR(kErrParameterOutOfBound);
    ChunkMeta m;
    if (host_memcpy(&m, (ChunkMeta*)c->meta.p + chunkIdx, sizeof m, hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric);
    *nbSeq = m.nbSeq; *litSize = m.litSize;
    const size_t ns = m.nbSeq < seqCap ? m.nbSeq : seqCap, nl = m.litSize < litCap ? m.litSize : litCap;
    if (ns && host_memcpy(seqs, (Seq*)c->seqs.p + chunkIdx * kMaxSeq, ns * sizeof(Seq), hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric);
    const u8* litDev = m.litFromSrc ? c->lastSrc + chunkIdx * (size_t)c->lastChunkBytes : (const u8*)c->lits.p + chunkIdx * kLitStride;
    if (nl && (!litDev || host_memcpy(lits, litDev, nl, hipMemcpyDeviceToHost) != hipSuccess)) return ZERR(kErrGeneric);
    return 0;
}

// one caller-supplied seqStore through huf_build / huf_encode / seq_encode.  resolveReps 0: offBase holds repcodes already, as the block
// codes them; 1: offBase is distance + 3 throughout and seq_encode resolves it against `reps`, as behind the match finders.  Either way
// the record is chunk 0 of the context's last call afterwards (ZSTDMI_debugGetChunk reads the codes seq_encode left), raw verdict or not.
static size_t debug_entropy_block(ZSTD_CCtx* c, void* dst, size_t dstCapacity, const ZSTDMI_Seq* seqs, size_t nbSeq,
                                  const void* lits, size_t litSize, size_t srcSize, u32 resolveReps, const u32* reps)
{
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    if (nbSeq > kMaxSeq || litSize > kChunkSize || srcSize > kChunkSize) return ZERR(kErrParameterOutOfBound);
    if (!cctx_workspace(c, 1)) return ZERR(kErrMemoryAllocation);
    hipStream_t s = c->stream;
    ChunkMeta m = {}; m.srcSize = (u32)srcSize; m.nbSeq = (u32)nbSeq; m.litSize = (u32)litSize;
    m.fhSize = frame_header_bytes(FrameHeaderSpec{}, srcSize);
    if (nbSeq) (void)hipMemcpyAsync(c->seqs.p, seqs, nbSeq * sizeof(Seq), hipMemcpyHostToDevice, s);
    if (litSize) (void)hipMemcpyAsync(c->lits.p, lits, litSize, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(c->meta.p, &m, sizeof m, hipMemcpyHostToDevice, s);
    launch_huf_build((u8*)c->lits.p, (ChunkMeta*)c->meta.p, (HufTable*)c->tables.p, (u8*)c->slots.p, 1, 0, nullptr, layout_arith(0, 0, 0), s, StageHook());
    launch_huf_encode((u8*)c->lits.p, (ChunkMeta*)c->meta.p, (HufTable*)c->tables.p, (u8*)c->slots.p, nullptr, nullptr, 0, 1, nullptr, 0, s);
    { const Resolved rs = resolve_call(sticky_params(c), srcSize, kChunkSize);
      launch_seq_encode((Seq*)c->seqs.p, (ChunkMeta*)c->meta.p, (u8*)c->slots.p, 1, rs.cp.strategy < kStratGreedy ? rs.cp.strategy : (u32)kStratGreedy, FrameHeaderSpec{}, resolveReps, reps, layout_arith(kChunkSize, 0, 0), s); }
    if (isErr(dev_read(&m, c->meta.p, sizeof m, s))) return ZERR(kErrGeneric);
    c->lastChunks = 1;
    if (m.blockType != 2) return 0;
    if (m.bodySize > dstCapacity) return ZERR(kErrDstSizeTooSmall);
    if (host_memcpy(dst, (u8*)c->slots.p + m.fhSize + 3, m.bodySize, hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric);
    return m.bodySize;
}
size_t ZSTDMI_debugEntropyBlock(ZSTD_CCtx* c, void* dst, size_t dstCapacity, const ZSTDMI_Seq* seqs, size_t nbSeq,
                                const void* lits, size_t litSize, size_t srcSize)
{
    const u32 plainReps[3] = { 1, 4, 8 };
    return debug_entropy_block(c, dst, dstCapacity, seqs, nbSeq, lits, litSize, srcSize, 0, plainReps);
}
size_t ZSTDMI_debugEntropyBlockRaw(ZSTD_CCtx* c, void* dst, size_t dstCapacity, const ZSTDMI_Seq* seqs, size_t nbSeq,
                                   const void* lits, size_t litSize, size_t srcSize, const unsigned rep[3])
{
    if (!rep) return ZERR(kErrGeneric);
    for (size_t i = 0; i < nbSeq && i < kMaxSeq; ++i) if (seqs[i].offBase < 4) return ZERR(kErrParameterOutOfBound);     // (distance + 3, distance >= 1)
    const u32 reps[3] = { rep[0], rep[1], rep[2] };
    return debug_entropy_block(c, dst, dstCapacity, seqs, nbSeq, lits, litSize, srcSize, 1, reps);
}

size_t ZSTDMI_debugPoisonedChunk(ZSTD_CCtx* c, unsigned nbSeq, unsigned litSize, unsigned srcSize, unsigned fill)
{
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    hipStream_t s = c->stream;
    // (with ZSTDMI_CCtx_setDictEntropy on and a formatted dictionary loaded, the instances that read its tables run)
    e = cctx_sync_dictionary(c); if (isErr(e)) return e;
    const DictCTables* const dct = call_dict_ctables(c, sticky_params(c));
    // (with ZSTDMI_CCtx_setEntropyCarry on, and no such tables, the record is filed twice, as the two blocks of one frame in the
    //  pipeline's order, and seq_encode's carry instance codes the second behind what the first left: the answer is the second's)
    const bool carry = c->entropyCarry && !dct;
    const u32 nRec = carry ? 2u : 1u;
    if (!cctx_workspace(c, nRec)) return ZERR(kErrMemoryAllocation);
    const u32 blockSize = srcSize < kChunkSize ? srcSize : kChunkSize;
    ChunkMeta m = {}; m.srcSize = srcSize; m.nbSeq = nbSeq; m.litSize = litSize; m.fhSize = frame_header_bytes(FrameHeaderSpec{}, blockSize);
    (void)hipMemsetAsync(c->seqs.p, (int)(fill & 0xFF), (size_t)nRec * kMaxSeq * sizeof(Seq), s);
    (void)hipMemsetAsync(c->lits.p, (int)(fill & 0xFF), (size_t)nRec * kLitStride, s);
    for (u32 r = 0; r < nRec; ++r) (void)hipMemcpyAsync((ChunkMeta*)c->meta.p + r, &m, sizeof m, hipMemcpyHostToDevice, s);
    const FrameLayout frames = carry ? layout_arith(kChunkSize, 2, (u64)kChunkSize + blockSize) : layout_arith(kChunkSize, 0, blockSize);
    const u32 plainReps[3] = { 1, 4, 8 };
    const SeqCarry sc = { (HufTable*)c->tables.p, nullptr, 1, 0 };
    launch_huf_build((u8*)c->lits.p, (ChunkMeta*)c->meta.p, (HufTable*)c->tables.p, (u8*)c->slots.p, nRec, 0, (const u8*)c->lits.p, layout_arith(kChunkSize, 0, 0), s, StageHook(), dct);
    if (!carry) launch_huf_encode((u8*)c->lits.p, (ChunkMeta*)c->meta.p, (HufTable*)c->tables.p, (u8*)c->slots.p, nullptr, nullptr, 0, 1, (const u8*)c->lits.p, kChunkSize, s, dct != nullptr);
    launch_seq_encode((Seq*)c->seqs.p, (ChunkMeta*)c->meta.p, (u8*)c->slots.p, nRec, 1, FrameHeaderSpec{}, 1, plainReps, frames, s, dct, nullptr, nullptr, carry ? &sc : nullptr);
    if (carry) launch_huf_encode((u8*)c->lits.p, (ChunkMeta*)c->meta.p, (HufTable*)c->tables.p, (u8*)c->slots.p, nullptr, nullptr, 0, nRec, (const u8*)c->lits.p, kChunkSize, s, true);
    if (isErr(dev_read(&m, (ChunkMeta*)c->meta.p + (nRec - 1), sizeof m, s))) return ZERR(kErrGeneric);
    c->lastChunks = 0;
    return m.outSize;
}

// ---------------- entry points whose host-side containers may throw: guarded (see guarded()) ----------------
size_t ZSTD_CCtx_loadDictionary(ZSTD_CCtx* c, const void* dict, size_t dictSize) { return guarded([&] { return ZSTD_CCtx_loadDictionary_impl(c, dict, dictSize); }); }
size_t ZSTD_compressStream2(ZSTD_CCtx* c, ZSTD_outBuffer* output, ZSTD_inBuffer* input, int endOp) { return guarded([&] { return ZSTD_compressStream2_impl(c, output, input, endOp); }); }

} // extern "C"

// ---- a batch of independent entries, each compressed as the single call would compress it alone (ZSTDMI_compressBatch; the
// dictionary trainer's inner loop, dict_train.hip) ----
// Entries of one framing class (same dictionary prefix, chunk size, blocks per frame and resolved parameters) go through the pipeline
// together (staged_encode): each chunk of an entry is staged at its own chunk boundary (batch_stage_kernel) and the finder and the checksum take its
// length from a per-chunk table (chunkLens).  Where every chunk is a frame of its own, what is written for it depends on nothing
// beside it.  Multi-block frames behind LDS history (the small-call 16 KiB cut of levels 1-2, the 48 / 32 KiB blocks of the dual-hash
// and chain finders) take a second column (chunkFrames): the block's index inside its frame and the frame's content size, which the
// single call derives from its total size; all chunks of an entry but the last are full, so a block's history lies in front of it in
// the staging buffer as it does in the entry.
// compress_entries (below) is the sequence of the steps that follow: batch_classify sorts the entries into groups and the alone
// list, a group is cut into passes (batch_pass_cut), batch_pass_image lays out and fills a pass's table (behind per-entry CDicts with
// batch_slot_table's slots), batch_pass_run runs it, batch_alone_tail takes the rest.  The host decisions among them — the group key,
// the cut, the table's layout and its fill — are zmi_batch_pass.h's, which tests/host/batch_plan_harness.cpp holds to account.
//
// entry_batched -> does an entry of S bytes (S > 0, framed as fr) share a batched pass?  One rule for compress_entries, which sorts
// its entries by it, and for ZSTDMI_compressPack, which cuts its rounds by it.
// An entry the class model does not cover — empty, windows below 64 KiB above one window, LDM above one block, more than one block under
// ZSTDMI_CCtx_setSingleFrame (one frame per entry: a framing of its own), the fast strategy's
// full 64 KiB blocks with far candidates (no per-chunk tables in that kernel), the sparse-input probe and multi-block frames of
// 4 MiB and more, more chunks than a pass, several device workers — is compressed alone afterwards, in entry order, by the
// single-call path, and counted in `alone` (batch_alone_tail).
static bool entry_batched(ZSTD_CCtx* c, const CallParams& cp, size_t S, const Framing& fr, u32 passLimit, bool dct, bool stats)
{
    bool batched = S && !fr.indepWindowLog && !fr.ldm && !fr.single && c->workers.size() <= 1 && chunks_of(S, fr.chunkBytes) <= passLimit;
    // multi-block frames: the blocks behind LDS history (chunks below 64 KiB; the full 64 KiB blocks with far candidates have no
    // table form, launch_lz), below 4 MiB and of at most 256 chunks (a block index and a frame size that fit chunk_frame_word);
    // with a dictionary's entropy tables (huf_tree_kernel<true> finds a frame's first block in the arithmetic form alone), or with sizes
    // only and statistics (the trainer's finalize step), as before: alone
    if (batched && fr.frameBlocks)
        batched = S < (4u << 20) && chunks_of(S, fr.chunkBytes) <= 256 && fr.chunkBytes < kChunkSize && !dct && !stats;
    if (batched && S >= (4u << 20)) { size_t err = 0; if (probe_group_bytes(c, cp, S, err) || isErr(err)) batched = false; }
    return batched;
}
static u32 batch_pass_limit(const ZSTD_CCtx* c) { return c->passChunks < 16384 ? c->passChunks : 16384; }

// What the steps of one compress_entries call share: its arguments, the per-entry CDicts, and the vectors every pass fills anew.
// srcs[i]: device pointers.  dsts / caps: device pointers and their capacities, or null (sizes only).  outSizes[i] = the compressed
// size of entry i (or its error).  d_stats (optional, device, 377 u32): seq_stats_kernel's counts of the batched chunks are added.
// seekIdx (optional; ZSTDMI_compressPack): the row of c->seekEntries (seekCap rows) at which entry i's frames are filed, one
// (compressed size, content size) pair per frame, by every pass from its ChunkMeta (pack_entries_kernel).
// cdicts (optional; ZSTDMI_compressBatchCDicts): entry i is compressed behind cdicts[i] (null: without a dictionary) as after
// ZSTD_CCtx_refCDict, all of them shareable by this context (on its device, no workers) — or a single one that is not, of which the
// context holds its private upload (compress_batch_cdicts_impl).  `cp` then holds the context's parameters without
// a reference; what the call runs with is resolved per distinct CDict, because its level is: CallParams here, LaunchState per pass.
// For the length of a resolve or a launch the CDict is the context's reference (c->cdict), which is put back at the end.
struct BatchCall {
    ZSTD_CCtx* c; const CallParams& cp; const u8* const* srcs; const size_t* sizes; size_t n; u8* const* dsts; const size_t* caps; size_t* outSizes;
    u32* d_stats; const u32* seekIdx; u32 seekCap; const ZSTD_CDict_s* const* cdicts;
    const ZSTD_CDict_s* was;
    // per-entry CDicts: the distinct ones, each entry's index among them, and the parameters each of them makes of the context's
    std::vector<const void*> dicts; std::vector<u32> slotOf; std::vector<CallParams> cps; std::vector<size_t> slotErr;
    // a pass's table on the host, its sizes as they come back, and the slot table of a pass behind per-entry CDicts
    std::vector<u8> tab; std::vector<u64> got;
    std::vector<u32> chunkSlot, used; std::vector<CDictSlot> slotTab; std::vector<u8> slotDone;
    ~BatchCall() { c->cdict = was; }
    // the parameters entry i runs with; with per-entry CDicts its CDict becomes the reference in force
    const CallParams& params_of(size_t i)
    {
        if (!cdicts) return cp;
        c->cdict = (const ZSTD_CDict_s*)dicts[slotOf[i]];
        return cps[slotOf[i]];
    }
    size_t assign_cdicts()
    {
        const int bad = cdict_slots_assign((const void* const*)cdicts, n, dicts, slotOf);
        if (bad) return bad == 1 ? ZERR(kErrParameterUnsupported) : ZERR(kErrMemoryAllocation);
        for (const void* d : dicts) {
            CallParams q = cp;
            if (d) q.level = ((const ZSTD_CDict_s*)d)->level; else q.useDict = false;
            cps.push_back(q); slotErr.push_back(check_call_params(q));       // (what every single call behind this CDict would answer)
        }
        return 0;
    }
};
// Entries share a group, and so a pass, by same_group (zmi_batch_pass.h).  tail (per-entry CDicts): each member's prefixLen
struct BatchGroup { Framing fr; u32 slot; std::vector<size_t> members; std::vector<u32> tail; };
static BatchGroupKey group_key(const Framing& fr, u32 slot) { return BatchGroupKey{ fr.prefixLen, fr.chunkBytes, fr.frameBlocks, fr.dictIndex, fr.rs, slot }; }

// Classify: the single call's argument checks, the entry's framing, and its place — a group, or the alone list
static void batch_classify(BatchCall& b, u32 passLimit, std::vector<BatchGroup>& groups, std::vector<size_t>& aloneList)
{
    ZSTD_CCtx* c = b.c;
    for (size_t i = 0; i < b.n; i++) {
        const size_t S = b.sizes[i];
        if (b.dsts) {         // (the single call's argument checks)
            if (S && !b.srcs[i]) { b.outSizes[i] = ZERR(kErrSrcSizeWrong); continue; }
            if (!b.dsts[i]) { b.outSizes[i] = b.caps[i] ? ZERR(kErrDstBufferNull) : ZERR(kErrDstSizeTooSmall); continue; }
        }
        if (b.cdicts && isErr(b.slotErr[b.slotOf[i]])) { b.outSizes[i] = b.slotErr[b.slotOf[i]]; continue; }
        const CallParams& cpi = b.params_of(i);
        const Framing fr = S ? resolve_framing(c, cpi, S) : Framing{};
        if (!S || !entry_batched(c, cpi, S, fr, passLimit, call_dict_ctables(c, cpi) != nullptr, b.d_stats != nullptr)) { aloneList.push_back(i); continue; }
        b.outSizes[i] = 0;
        const u32 slot = b.cdicts ? b.slotOf[i] : 0u;
        BatchGroup* g = nullptr;
        for (auto& x : groups) if (same_group(group_key(x.fr, x.slot), group_key(fr, slot), b.cdicts != nullptr)) { g = &x; break; }
        if (!g) { groups.push_back(BatchGroup{fr, slot, {}, {}}); g = &groups.back(); }
        g->members.push_back(i);
        if (b.cdicts) g->tail.push_back(fr.prefixLen);
    }
}

// Slot table (per-entry CDicts): the launch state of the pass of members [m0, m1) of g is that of its dictionary, or, behind two or
// more of them, the group's with a slot table (zmi_cdictset.h): each chunk's index into it (b.chunkSlot) and the slots (b.slotTab),
// each from the first entry behind it.  The pass's state ls and its tail fr.prefixLen are its first entry's.
static size_t batch_slot_table(BatchCall& b, const BatchGroup& g, size_t m0, size_t m1, Framing& fr, LaunchState& ls)
{
    b.chunkSlot.clear();
    for (size_t m = m0; m < m1; ++m) b.chunkSlot.insert(b.chunkSlot.end(), chunks_of(b.sizes[g.members[m]], fr.chunkBytes), b.slotOf[g.members[m]]);
    if (!cdict_pass_image(b.chunkSlot, b.used)) return ZERR(kErrMemoryAllocation);
    b.slotTab.assign(b.used.size(), CDictSlot{});
    b.slotDone.assign(b.used.size(), 0);
    for (size_t m = m0; m < m1; ++m) {
        const size_t i = g.members[m];
        const size_t k = std::lower_bound(b.used.begin(), b.used.end(), b.slotOf[i]) - b.used.begin();
        assert(!b.slotDone[k] || b.slotTab[k].tailLen == g.tail[m]);        // (one dictionary, one chunk size: one tail)
        if (b.slotDone[k]) continue;
        fr.prefixLen = g.tail[m];
        const LaunchState lu = launch_state(b.c, b.params_of(i), fr);
        b.slotTab[k] = CDictSlot{ lu.prefix, lu.dct, lu.dix, fr.prefixLen, lu.header.dictID, lu.header.dictIdBytes, { lu.initReps[0], lu.initReps[1], lu.initReps[2] } };
        b.slotDone[k] = 1;
        if (m == m0) ls = lu;
    }
    fr.prefixLen = g.tail[m0];
    return 0;
}

// One pass: members [m0, m0 + nEnt) of its group, nCh chunks.  A pass that holds two or more distinct CDicts (set) uploads the slot
// table and runs the stages' set instances; a pass behind one is launched exactly as the call without `cdicts` launches it.
// carry: carried entropy state (entries of more than one block), the chunks that lead a carry group listed beside the table
// (zmi_carry.h), so that an entry's bytes are the single call's.
struct BatchPass {
    size_t m0; u32 nEnt, nCh; Framing fr; LaunchState ls;
    bool set, carry; u32 carryGroups; const DictCTables* dct;
    BatchPassTab t; BatchPassSpan at;
};
// the pass's table on the host (b.tab): laid out by batch_pass_tab, filled by batch_pass_fill
static size_t batch_pass_image(BatchCall& b, const BatchGroup& g, BatchPass& p)
{
    const size_t m1 = p.m0 + p.nEnt;
    if (b.cdicts) { const size_t e = batch_slot_table(b, g, p.m0, m1, p.fr, p.ls); if (isErr(e)) return e; }
    p.set = b.cdicts && b.used.size() >= 2;
    p.dct = p.ls.dct;
    if (p.set) for (const CDictSlot& r : b.slotTab) if (r.dct) p.dct = r.dct;     // (any: "some slot has tables")
    p.carry = carry_active(b.c, b.params_of(g.members[p.m0]), p.fr, p.ls);
    p.t = batch_pass_tab(p.nCh, p.nEnt, p.fr.frameBlocks != 0, b.seekIdx != nullptr, p.set ? (u32)b.slotTab.size() : 0u, p.carry);
    b.tab.assign(p.t.bytes, 0);
    const BatchPassCols h = batch_pass_cols(p.t, b.tab.data());
    if (p.set) { memcpy(h.chunkSlot, b.chunkSlot.data(), (size_t)p.nCh * 4); memcpy(h.slots, b.slotTab.data(), b.slotTab.size() * sizeof(CDictSlot)); }
    p.at = batch_pass_fill(BatchPassEntries{ g.members.data() + p.m0, p.nEnt, b.srcs, b.sizes, b.dsts, b.caps, b.seekIdx }, p.fr.chunkBytes, p.fr.frameBlocks, h);
    p.carryGroups = 0;
    if (p.carry) { p.carryGroups = carry_leaders_table(h.frame, p.nCh, h.leaders); b.c->lastCarryGroups += p.carryGroups; }
    return 0;
}
// Run it: per pass one table goes up and the entries' sizes come back in one copy.  With destinations, batch_place_kernel gives every
// chunk its place as an offset from the lowest destination pointer and huf_encode and gather write there directly (staged_write);
// without (the trainer), only the sizes come back.
static size_t batch_pass_run(BatchCall& b, const BatchGroup& g, const BatchPass& p, bool& first)
{
    ZSTD_CCtx* c = b.c;
    hipStream_t s = c->stream;
    if (!staged_workspace(c, p.ls, p.fr, p.nCh, p.t.bytes + (size_t)p.nEnt * 8)) return ZERR(kErrMemoryAllocation);
    const BatchPassCols d = batch_pass_cols(p.t, (u8*)c->batchTab.p);
    if (hipMemcpyAsync(c->batchTab.p, b.tab.data(), p.t.bytes, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
    ChunkMeta* meta = (ChunkMeta*)c->meta.p;
    // (dct: single-block frames only, see entry_batched)
    StagedPass pass = staged_pass(p.nCh, p.fr, d.from, d.len, d.frame, p.dct, b.cp.checksumFlag);
    if (p.set) { pass.dSlots = d.slots; pass.dChunkSlot = d.chunkSlot; }
    const SeqCarry sc = { (HufTable*)c->tables.p, d.leaders, p.carryGroups, p.fr.rs.rawLiterals };
    if (p.carry) pass.carry = &sc;
    c->timer.begin(s);
    staged_encode(c, p.ls, p.fr, pass);
    c->lastBatchPasses++; if (p.set) c->lastBatchSetChunks += p.nCh;
    if (b.d_stats) launch_seq_stats((Seq*)c->seqs.p, (u8*)c->lits.p, meta, p.nCh, (const u8*)c->batchStage.p, p.fr.chunkBytes, b.d_stats, s);
    launch_batch_place(meta, p.nEnt, d.entFirst, d.entDst, d.entCap, p.at.span, (u64*)c->offsets.p, d.got, s);
    c->timer.mark("batch_place", s);
    if (b.seekIdx) {
        launch_pack_entries(meta, p.nEnt, d.entFirst, d.len, p.fr.frameBlocks, d.entSeek, (u32*)c->seekEntries.p, b.seekCap, s);
        c->timer.mark("pack_entries", s);
    }
    if (b.dsts) staged_write(c, pass, (u8*)p.at.lo, p.at.span);
    b.got.resize(p.nEnt);
    if (isErr(dev_read(b.got.data(), d.got, (size_t)p.nEnt * 8, s))) return ZERR(kErrGeneric);
    add_stage_times(c, first);
    const size_t* const members = g.members.data() + p.m0;
    for (u32 e = 0; e < p.nEnt; ++e) b.outSizes[members[e]] = (size_t)b.got[e];
    return 0;
}

// Alone tail: what the class model does not cover, in entry order, by the single-call path
static void batch_alone_tail(BatchCall& b, const std::vector<size_t>& aloneList, int& alone)
{
    std::vector<u8> tmp;
    for (size_t i : aloneList) {
        const CallParams& cpi = b.params_of(i);
        if (b.dsts) b.outSizes[i] = compress_device(b.c, cpi, b.dsts[i], b.caps[i], b.srcs[i], b.sizes[i]);
        else { tmp.resize(ZSTD_compressBound(b.sizes[i])); b.outSizes[i] = compress_any(b.c, cpi, tmp.data(), tmp.size(), b.srcs[i], b.sizes[i]); }
        ++alone;
    }
}

// A pass holds whole entries, at most ZSTDMI_CCtx_setPassChunks chunks (batch_pass_cut).
static size_t compress_entries(ZSTD_CCtx* c, const CallParams& cp, const u8* const* srcs, const size_t* sizes, size_t n,
                               u8* const* dsts, const size_t* caps, size_t* outSizes, u32* d_stats, int& alone,
                               const u32* seekIdx = nullptr, u32 seekCap = 0, const ZSTD_CDict_s* const* cdicts = nullptr)
{
    alone = 0;
    c->lastRegionList = nullptr;        // (entries that go alone pass through compress_range, which notes its own)
    c->lastBatchPasses = 0; c->lastBatchSetChunks = 0;
    const u32 passLimit = batch_pass_limit(c);
    BatchCall b{ c, cp, srcs, sizes, n, dsts, caps, outSizes, d_stats, seekIdx, seekCap, cdicts, c->cdict };
    if (cdicts) { const size_t e = b.assign_cdicts(); if (isErr(e)) return e; }
    std::vector<BatchGroup> groups;
    std::vector<size_t> aloneList;
    batch_classify(b, passLimit, groups, aloneList);
    bool first = true;
    for (const BatchGroup& g : groups) {
        const LaunchState ls = launch_state(c, b.params_of(g.members[0]), g.fr);      // (what sizes the workspace is the group's: same_launch_params)
        for (size_t m0 = 0; m0 < g.members.size(); ) {
            u32 nCh = 0;
            const size_t m1 = batch_pass_cut(m0, g.members.size(), passLimit, [&](size_t m) { return (u32)chunks_of(sizes[g.members[m]], g.fr.chunkBytes); }, nCh);
            BatchPass p = { m0, (u32)(m1 - m0), nCh, g.fr, ls };
            size_t e = batch_pass_image(b, g, p); if (isErr(e)) return e;
            e = batch_pass_run(b, g, p, first); if (isErr(e)) return e;
            m0 = m1;
        }
    }
    batch_alone_tail(b, aloneList, alone);
    c->lastChunks = 0;                                  // (ZSTDMI_debugGetChunk: no ordinary call to look at)
    return 0;
}

// the trainer's samples (host memory, sample i at src + offs[i]): uploaded once, then compress_entries without destinations.
// stats (optional, host, 377 u32): literal / LL / ML / offset code counts of the compressed blocks are added to it.
namespace zmi {
size_t compress_samples(ZSTD_CCtx* c, const u8* src, const u64* offs, const size_t* sizes, size_t n, size_t* outSizes, u32* stats)
{
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    c->lastRegionList = nullptr; c->lastCarryGroups = 0;
    CallParams cp = sticky_params(c); cp.seek = false;
    cp.entropyCarry = false;        // (sizes and statistics of the samples are those of the default coding, whatever the context's switch says)
    e = cctx_sync_dictionary(c); if (isErr(e)) return e;
    hipStream_t s = c->stream;
    u64 maxEnd = 0;
    for (size_t i = 0; i < n; i++) if (sizes[i] && offs[i] + sizes[i] > maxEnd) maxEnd = offs[i] + sizes[i];
    DevBuf dSrc, dStats;
    struct Free { DevBuf &a, &b; ~Free() { a.release(); b.release(); } } freeThem{dSrc, dStats};
    if (!dSrc.ensure(maxEnd + 16) || !dStats.ensure(377 * 4)) return ZERR(kErrMemoryAllocation);
    if ((maxEnd && hipMemcpyAsync(dSrc.p, src, maxEnd, hipMemcpyHostToDevice, s) != hipSuccess) || hipMemsetAsync(dStats.p, 0, 377 * 4, s) != hipSuccess) return ZERR(kErrGeneric);
    std::vector<const u8*> srcs(n);
    for (size_t i = 0; i < n; i++) srcs[i] = (const u8*)dSrc.p + offs[i];
    int alone = 0;
    e = compress_entries(c, cp, srcs.data(), sizes, n, nullptr, nullptr, outSizes, stats ? (u32*)dStats.p : nullptr, alone);
    if (isErr(e)) return e;
    if (stats) {
        std::vector<u32> h(377);
        if (hipMemcpyAsync(h.data(), dStats.p, 377 * 4, hipMemcpyDeviceToHost, s) != hipSuccess || (count_wait(), hipStreamSynchronize(s)) != hipSuccess) { (void)hipGetLastError(); return ZERR(kErrGeneric); }
        // (deliberately not dev_read: a failed copy, too, is followed by hipGetLastError here)
        for (u32 i = 0; i < 377; i++) stats[i] += h[i];
    }
    return 0;
}
} // namespace zmi

// The public batch: n device-resident entries, each to its own destination with its own status (include/zstd_mi355x.h)
static size_t compress_batch_impl(ZSTD_CCtx* c, const void* const* srcs, const size_t* srcSizes, size_t n, void* const* dsts, const size_t* dstCapacities, size_t* dstSizes)
{
    if (!c) return ZERR(kErrGeneric);
    if (c->contentCuts) return ZERR(kErrParameterUnsupported);       // (a batch's entries are the caller's cuts)
    c->lastRegionList = nullptr; c->lastCarryGroups = 0;
    if (n == 0) { c->lastBatchAlone = 0; return 0; }
    if (!srcs || !srcSizes || !dsts || !dstCapacities || !dstSizes) return ZERR(kErrGeneric);
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    if (c->workers.size() > 1 || c->seekTable || c->pfx) return ZERR(kErrParameterUnsupported);
    c->lastBatchAlone = 0;
    const CallParams cp = sticky_params(c);
    e = check_call_params(cp);
    if (isErr(e)) { for (size_t i = 0; i < n; i++) dstSizes[i] = e; return 0; }     // (what every single call would answer)
    e = cctx_sync_dictionary(c); if (isErr(e)) return e;
    return compress_entries(c, cp, (const u8* const*)srcs, srcSizes, n, (u8* const*)dsts, dstCapacities, dstSizes, nullptr, c->lastBatchAlone);
}
extern "C" size_t ZSTDMI_compressBatch(ZSTD_CCtx* c, const void* const* srcs, const size_t* srcSizes, size_t n, void* const* dsts, const size_t* dstCapacities, size_t* dstSizes)
{
    return guarded([&] { return compress_batch_impl(c, srcs, srcSizes, n, dsts, dstCapacities, dstSizes); });
}
extern "C" int ZSTDMI_debugLastBatchAlone(const ZSTD_CCtx* c) { return c ? c->lastBatchAlone : -1; }
extern "C" long long ZSTDMI_debugLastBatchPasses(const ZSTD_CCtx* c) { return c ? c->lastBatchPasses : -1; }
extern "C" long long ZSTDMI_debugLastBatchSetChunks(const ZSTD_CCtx* c) { return c ? c->lastBatchSetChunks : -1; }

// ---------------- a batch enqueued from the device (include/zstd_mi355x.h) ----------------
// (the pass's tables, async_tab and async_plan_tab, and what a pack adds to either prepare, pack_async_tab: zmi_batch_pass.h)
// pack_frames_of: pack_async_tab's F for an entry of `bound` bytes under the framing.
static u32 pack_frames_of(size_t bound, const Framing& fr)
{
    const u32 chunks = chunks_of(bound, fr.chunkBytes), F = fr.frameBlocks ? (chunks + fr.frameBlocks - 1) / fr.frameBlocks : chunks;
    return F ? F : 1u;
}
// Both async prepares behind their own device-free refusals, from the call's parameters to the AsyncPrep with its empty frame.
// chunkLimit: the chunks a call may hold (0: every entry's, up to the pass limit).  oneBlock: ZSTDMI_CCtx_prepareBatchAsync, which
// refuses what is not one chunk in a single-block frame.
static size_t prepare_async_core(ZSTD_CCtx* c, size_t maxEntries, size_t bound, size_t chunkLimit, bool oneBlock)
{
    const u32 passLimit = batch_pass_limit(c);
    const CallParams cp = sticky_params(c);
    if (c->contentCuts) return ZERR(kErrParameterUnsupported);       // (the enqueued calls refuse the switch: nothing to prepare for)
    size_t e = check_call_params(cp); if (isErr(e)) return e;
    e = cctx_bind(c); if (isErr(e)) return e;
    e = cctx_sync_dictionary(c); if (isErr(e)) return e;
    // (a formatted dictionary's tail is known once it has been validated, so the framing is resolved behind the upload)
    const Framing fr = resolve_framing(c, cp, bound);
    if ((oneBlock && (bound > fr.chunkBytes || fr.frameBlocks)) || !entry_batched(c, cp, bound, fr, passLimit, call_dict_ctables(c, cp) != nullptr, false))
        return ZERR(kErrParameterUnsupported);
    const LaunchState ls = launch_state(c, cp, fr);
    if (carry_active(c, cp, fr, ls)) return ZERR(kErrParameterUnsupported);       // (its group count is a host launch argument)
    const u32 perEntry = (u32)chunks_of(bound, fr.chunkBytes);
    if (chunkLimit && chunkLimit < perEntry) return ZERR(kErrParameterOutOfBound);
    const u64 most = (u64)maxEntries * perEntry;
    u32 maxChunks = chunkLimit ? (u32)chunkLimit : (u32)(most < passLimit ? most : passLimit);
    // one block in a single-block frame and room for every entry: entry e is chunk e (batch_plan_kernel), whichever prepare was called;
    // the table is sized for the planned kernels too, which the pack runs
    const bool planned = !(perEntry == 1 && !fr.frameBlocks && maxChunks >= maxEntries);
    if (!planned) maxChunks = (u32)maxEntries;
    const u32 nCh = maxChunks ? maxChunks : 1u;
    const size_t tabBytes = async_plan_tab((u32)maxEntries, nCh).bytes;
    if (!staged_workspace(c, ls, fr, nCh, planned ? tabBytes : std::max(async_tab(nCh).bytes, tabBytes)) ||
        !c->packAsync.ensure(pack_async_tab((u32)maxEntries, pack_frames_of(bound, fr)).bytes)) return ZERR(kErrMemoryAllocation);
    if (!c->asyncEv && hipEventCreateWithFlags(&c->asyncEv, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); c->asyncEv = nullptr; return ZERR(kErrMemoryAllocation); }
    AsyncPrep* const P = new AsyncPrep{ cctx_gen(c), (u32)maxEntries, bound, cp, fr, {}, maxChunks, planned };
    u8 f[18 + 3 + 4]; const size_t n = empty_frame_write(cp, f);
    assert(n <= sizeof P->empty.bytes);
    memcpy(P->empty.bytes, f, n); P->empty.len = (u32)n;
    c->asyncPrep = P;
    return 0;
}
static size_t prepare_batch_async_impl(ZSTD_CCtx* c, size_t maxEntries, size_t bound)
{
    if (!c) return ZERR(kErrGeneric);
    delete c->asyncPrep; c->asyncPrep = nullptr;
    // what the one-block batched pass does not cover, as far as the host alone can tell
    if (!bound || bound > kChunkSize || c->workers.size() > 1 || c->seekTable || c->pfx || maxEntries > batch_pass_limit(c)) return ZERR(kErrParameterUnsupported);
    return prepare_async_core(c, maxEntries, bound, maxEntries, true);
}
// ZSTDMI_CCtx_prepareBatchAsyncLimits: the prepare above for a bound of any number of chunks that compress_entries would batch
static size_t prepare_batch_async_limits_impl(ZSTD_CCtx* c, const ZSTDMI_CBatchLimits* L)
{
    if (!c || !L) return ZERR(kErrGeneric);
    delete c->asyncPrep; c->asyncPrep = nullptr;
    const u32 passLimit = batch_pass_limit(c);
    if (!L->maxEntries || L->maxEntries > passLimit || !L->srcSizeBound || L->srcSizeBound > kAsyncBoundMax || L->maxChunks > passLimit ||
        L->reserved[0] || L->reserved[1] || L->reserved[2]) return ZERR(kErrParameterOutOfBound);
    if (c->workers.size() > 1 || c->seekTable || c->pfx) return ZERR(kErrParameterUnsupported);
    return prepare_async_core(c, L->maxEntries, L->srcSizeBound, L->maxChunks, false);
}
static size_t batch_async_plan_impl(const ZSTD_CCtx* c, size_t* chunkBytes, size_t* frameBlocks, size_t* maxChunks)
{
    if (!c) return ZERR(kErrGeneric);
    const AsyncPrep* const P = c->asyncPrep;
    if (!P || P->gen != cctx_gen(c)) return ZERR(kErrStageWrong);
    if (chunkBytes) *chunkBytes = P->fr.chunkBytes;
    if (frameBlocks) *frameBlocks = P->fr.frameBlocks;
    if (maxChunks) *maxChunks = P->maxChunks;
    return 0;
}
// the event behind an enqueued pass (cctx_async_drain waits for it)
static size_t async_enqueued(ZSTD_CCtx* c, hipStream_t s)
{
    if (hipEventRecord(c->asyncEv, s) != hipSuccess) {      // (without the event nothing may stay in flight)
        (void)hipGetLastError();
        return stream_wait(s);
    }
    c->asyncPending = true;
    return 0;
}
// What an async call begins with: the prepare must hold for the context as it stands; then the device, the stage timer off for the
// length of the call (AsyncCall puts it back) and the debug counters of a call of one pass.
struct AsyncCall { StageTimer* timer = nullptr; bool was = false; ~AsyncCall() { if (timer) timer->enabled = was; } };
static size_t async_begin(ZSTD_CCtx* c, size_t n, AsyncCall& call)
{
    const AsyncPrep* const P = c->asyncPrep;
    if (!P || P->gen != cctx_gen(c) || n > P->maxEntries || (c->dictDirty && !cdict_shared(c)) || !c->deviceOk) return ZERR(kErrStageWrong);
    const size_t e = cctx_bind(c); if (isErr(e)) return e;
    call.timer = &c->timer; call.was = c->timer.enabled;
    c->timer.enabled = false;       // (stage events belong to calls that wait for them)
    c->lastRegionList = nullptr; c->lastCarryGroups = 0; c->lastBatchAlone = 0; c->lastBatchPasses = n ? 1 : 0; c->lastBatchSetChunks = 0; c->lastChunks = 0;
    return 0;
}
// The table of a call of n entries as the kernels take it, and nCh, the chunk slots every grid of the call has: host arithmetic on the
// entry count and the prepared limits; slots beyond the call's chunks compress one idle byte that is placed nowhere.  planned: the
// layout of async_plan_tab; else async_tab's, one chunk per entry (no src and size columns, no frame words).
struct AsyncPass { AsyncEntryTab et; u64* dFrom; u32* dLen; u32* dFrame; const u8* dummy; u32 nCh; };
static AsyncPass async_pass(const ZSTD_CCtx* c, const AsyncPrep* P, u32 n, bool planned)
{
    u8* const dTab = (u8*)c->batchTab.p;
    if (!planned) {
        const AsyncTab a = async_tab(n);
        return AsyncPass{ { nullptr, nullptr, (u64*)(dTab + a.atDst), (u64*)(dTab + a.atCap), (u32*)(dTab + a.atFirst), (u32*)(dTab + a.atVerdict) }, (u64*)dTab, (u32*)(dTab + a.atLen), nullptr, dTab + a.atDummy, n };
    }
    const AsyncPlanTab t = async_plan_tab(P->maxEntries, P->maxChunks);
    const u64 most = (u64)n * chunks_of(P->bound, P->fr.chunkBytes);
    return AsyncPass{ { (u64*)(dTab + t.atSrc), (u64*)(dTab + t.atSize), (u64*)(dTab + t.atDst), (u64*)(dTab + t.atCap), (u32*)(dTab + t.atFirst), (u32*)(dTab + t.atVerdict) },
                      (u64*)dTab, (u32*)(dTab + t.atLen), P->fr.frameBlocks ? (u32*)(dTab + t.atFrame) : nullptr, dTab + t.atDummy, (u32)(most < P->maxChunks ? most : P->maxChunks) };
}
// One staged pass of compress_entries with a plan on the device in the place of the host loop and the upload, and the caller's column in
// the place of the read-back: kernels (and the finder's two 4-byte hipMemsetAsync) only.  One chunk per entry: the plan and the
// placement with a lane per entry; a planned call: the two plan kernels, frames from chunk_frame_word (independent frames where the
// framing has no frameBlocks).
static size_t compress_batch_async_impl(ZSTD_CCtx* c, const void* const* d_srcs, const size_t* d_srcSizes, size_t n, void* const* d_dsts,
                                        const size_t* d_dstCapacities, size_t* d_dstSizes)
{
    if (!c) return ZERR(kErrGeneric);
    if (c->contentCuts) return ZERR(kErrParameterUnsupported);
    if (n == 0) return 0;
    if (!d_srcs || !d_srcSizes || !d_dsts || !d_dstCapacities || !d_dstSizes) return ZERR(kErrGeneric);
    AsyncCall call;
    const size_t e = async_begin(c, n, call); if (isErr(e)) return e;
    const AsyncPrep* const P = c->asyncPrep;
    hipStream_t s = c->stream;
    const Framing& fr = P->fr;
    const LaunchState ls = launch_state(c, P->cp, fr);
    const AsyncPass t = async_pass(c, P, (u32)n, P->planned);
    if (P->planned) {
        launch_batch_plan_entries(d_srcs, d_srcSizes, d_dsts, d_dstCapacities, (u32)n, P->bound, P->empty.len, fr.chunkBytes, P->maxChunks, t.et, s);
        launch_batch_plan_chunks(t.et, (u32)n, t.nCh, fr.chunkBytes, fr.frameBlocks, t.dummy, t.dFrom, t.dLen, t.dFrame, s);
    } else launch_batch_plan(d_srcs, d_srcSizes, d_dsts, d_dstCapacities, t.nCh, P->bound, P->empty.len, t.dummy, t.dFrom, t.et.dst, t.et.cap, t.dLen, t.et.first, t.et.verdict, s);
    const StagedPass pass = staged_pass(t.nCh, fr, t.dFrom, t.dLen, t.dFrame, ls.dct, P->cp.checksumFlag);
    staged_encode(c, ls, fr, pass);
    if (P->planned) launch_batch_place_async_frames((const ChunkMeta*)c->meta.p, (u32)n, t.nCh, t.et, P->empty, (u64*)c->offsets.p, d_dstSizes, s);
    else launch_batch_place_async((const ChunkMeta*)c->meta.p, t.nCh, t.et.dst, t.et.cap, t.et.verdict, P->empty, (u64*)c->offsets.p, d_dstSizes, s);
    staged_write(c, pass, (u8*)(uintptr_t)kAsyncBase, kAsyncSpan);
    return async_enqueued(c, s);
}
extern "C" size_t ZSTDMI_CCtx_prepareBatchAsyncLimits(ZSTD_CCtx* c, const ZSTDMI_CBatchLimits* limits)
{
    return guarded([&] { return prepare_batch_async_limits_impl(c, limits); });
}
extern "C" size_t ZSTDMI_CCtx_getBatchAsyncPlan(const ZSTD_CCtx* c, size_t* chunkBytes, size_t* frameBlocks, size_t* maxChunks)
{
    return guarded([&] { return batch_async_plan_impl(c, chunkBytes, frameBlocks, maxChunks); });
}
extern "C" size_t ZSTDMI_CCtx_prepareBatchAsync(ZSTD_CCtx* c, size_t maxEntries, size_t srcSizeBound)
{
    return guarded([&] { return prepare_batch_async_impl(c, maxEntries, srcSizeBound); });
}
extern "C" size_t ZSTDMI_compressBatchAsync(ZSTD_CCtx* c, const void* const* d_srcs, const size_t* d_srcSizes, size_t n, void* const* d_dsts,
                                            const size_t* d_dstCapacities, size_t* d_dstSizes)
{
    return guarded([&] { return compress_batch_async_impl(c, d_srcs, d_srcSizes, n, d_dsts, d_dstCapacities, d_dstSizes); });
}
// ---- a pack enqueued from the device (ZSTDMI_compressPackAsync, include/zstd_mi355x.h) ----
// compress_batch_async_impl's planned pass behind EITHER prepare (one chunk per entry in frames of their own is a case of it;
// prepare_async_core sized the planned table for that), with the pack's plan and placement: no per-entry destination, one decision
// for the whole stream, and the seek table behind the frames.  n == 0: the placement's decision and the table alone.
static size_t pack_async_bound_impl(const ZSTD_CCtx* c, size_t n)
{
    if (!c) return ZERR(kErrGeneric);
    const AsyncPrep* const P = c->asyncPrep;
    if (!P || P->gen != cctx_gen(c)) return ZERR(kErrStageWrong);
    const size_t per = ZSTD_compressBound(P->bound);
    size_t each, all, sum;
    if (isErr(per) || __builtin_add_overflow(per, (size_t)8 * pack_frames_of(P->bound, P->fr), &each) || __builtin_mul_overflow(each, n, &all) ||
        __builtin_add_overflow(all, (size_t)17, &sum) || isErr(sum)) return ZERR(kErrSrcSizeWrong);
    return sum;
}
static size_t compress_pack_async_impl(ZSTD_CCtx* c, u8* d_dst, size_t dstCapacity, const void* const* d_srcs, const size_t* d_srcSizes, size_t n,
                                       size_t* d_packSize, size_t* d_entryEnds)
{
    if (!c || !d_packSize || (n && (!d_srcs || !d_srcSizes))) return ZERR(kErrGeneric);
    if (c->contentCuts) return ZERR(kErrParameterUnsupported);
    if (!d_dst) return dstCapacity ? ZERR(kErrDstBufferNull) : ZERR(kErrDstSizeTooSmall);
    AsyncCall call;
    const size_t e = async_begin(c, n, call); if (isErr(e)) return e;
    const AsyncPrep* const P = c->asyncPrep;
    hipStream_t s = c->stream;
    const Framing& fr = P->fr;
    const u32 cb = fr.chunkBytes, frameBlocks = fr.frameBlocks, F = pack_frames_of(P->bound, fr), nEnt = (u32)n;
    const AsyncPass t = async_pass(c, P, nEnt, true);
    const PackAsyncLayout pt = pack_async_tab(P->maxEntries, F);
    u8* const dPack = (u8*)c->packAsync.p;
    const PackAsyncTab pk = { (u64*)dPack, (u32*)(dPack + pt.atRow), (u32*)(dPack + pt.atRows), (u64*)(dPack + pt.atState) };
    ChunkMeta* meta = (ChunkMeta*)c->meta.p; u64* offsets = (u64*)c->offsets.p;
    if (!t.nCh) {
        launch_pack_place_async(meta, 0, 0, t.et, t.dLen, frameBlocks, P->empty, d_dst, dstCapacity, pk, offsets, d_packSize, d_entryEnds, s);
        launch_pack_table_async(pk, 0, d_dst, s);
        return async_enqueued(c, s);
    }
    const LaunchState ls = launch_state(c, P->cp, fr);
    launch_pack_plan_entries(d_srcs, d_srcSizes, nEnt, P->bound, cb, P->maxChunks, t.et, s);
    launch_batch_plan_chunks(t.et, nEnt, t.nCh, cb, frameBlocks, t.dummy, t.dFrom, t.dLen, t.dFrame, s);
    const StagedPass pass = staged_pass(t.nCh, fr, t.dFrom, t.dLen, t.dFrame, ls.dct, P->cp.checksumFlag);
    staged_encode(c, ls, fr, pass);
    launch_pack_place_async(meta, nEnt, t.nCh, t.et, t.dLen, frameBlocks, P->empty, d_dst, dstCapacity, pk, offsets, d_packSize, d_entryEnds, s);
    staged_write(c, pass, (u8*)(uintptr_t)kAsyncBase, kAsyncSpan);
    launch_pack_table_async(pk, (u64)nEnt * F, d_dst, s);
    return async_enqueued(c, s);
}
extern "C" size_t ZSTDMI_CCtx_packAsyncBound(const ZSTD_CCtx* c, size_t n) { return pack_async_bound_impl(c, n); }
extern "C" size_t ZSTDMI_compressPackAsync(ZSTD_CCtx* c, void* d_dst, size_t dstCapacity, const void* const* d_srcs, const size_t* d_srcSizes, size_t n,
                                           size_t* d_packSize, size_t* d_entryEnds)
{
    return guarded([&] { return compress_pack_async_impl(c, (u8*)d_dst, dstCapacity, d_srcs, d_srcSizes, n, d_packSize, d_entryEnds); });
}
extern "C" long long ZSTDMI_debugHostWaits(const ZSTD_CCtx* c) { return c ? c->tally.waits : -1; }
extern "C" long long ZSTDMI_debugDeviceAllocs(const ZSTD_CCtx* c) { return c ? c->tally.allocs : -1; }

// The batch with a CDict per entry (include/zstd_mi355x.h).  Entries that all name one CDict (or none) ARE ZSTD_CCtx_refCDict + the batch
// above, private upload included; else compress_entries resolves per CDict, and nothing of the context's own dictionary is consulted.
static size_t compress_batch_cdicts_impl(ZSTD_CCtx* c, const void* const* srcs, const size_t* srcSizes, size_t n, void* const* dsts, const size_t* dstCapacities,
                                         size_t* dstSizes, const ZSTD_CDict* const* cdicts)
{
    if (!c) return ZERR(kErrGeneric);
    if (c->contentCuts) return ZERR(kErrParameterUnsupported);
    c->lastRegionList = nullptr; c->lastCarryGroups = 0;
    if (n == 0) { c->lastBatchAlone = 0; c->lastBatchPasses = 0; c->lastBatchSetChunks = 0; return 0; }
    if (!srcs || !srcSizes || !dsts || !dstCapacities || !dstSizes || !cdicts) return ZERR(kErrGeneric);
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    if (c->workers.size() > 1 || c->seekTable || c->pfx) return ZERR(kErrParameterUnsupported);
    // one = every entry names the same CDict (or none); only = the one non-NULL CDict of a call that names no second one; away = a
    // CDict on another device than the context's
    bool one = true, several = false, away = false;
    const ZSTD_CDict_s* only = nullptr;
    for (size_t i = 0; i < n; i++) {
        one = one && cdicts[i] == cdicts[0];
        if (!cdicts[i]) continue;
        away = away || cdicts[i]->device != c->device;
        if (only && cdicts[i] != only) several = true;
        only = cdicts[i];
    }
    if (one) return under_cdict(c, cdicts[0], [&] { return compress_batch_impl(c, srcs, srcSizes, n, dsts, dstCapacities, dstSizes); });
    if (several && away) return ZERR(kErrParameterUnsupported);       // (a private upload per CDict is what the call exists to avoid)
    c->lastBatchAlone = 0;
    auto run = [&]() -> size_t {
        const ZSTD_CDict_s* const was = c->cdict;
        c->cdict = nullptr;
        const CallParams cp = sticky_params(c);     // (the context's own level: each CDict's takes its place in compress_entries)
        c->cdict = was;
        return compress_entries(c, cp, (const u8* const*)srcs, srcSizes, n, (u8* const*)dsts, dstCapacities, dstSizes, nullptr, c->lastBatchAlone, nullptr, 0, cdicts);
    };
    if (!away) return run();
    // one CDict that cannot be shared, beside entries without a dictionary: the context's private upload of it stands in while it is in
    // force (under_cdict; dict_in_force), and the entries without one never ask for a dictionary
    return under_cdict(c, only, [&]() -> size_t { const size_t e2 = cctx_sync_dictionary(c); return isErr(e2) ? e2 : run(); });
}
extern "C" size_t ZSTDMI_compressBatchCDicts(ZSTD_CCtx* c, const void* const* srcs, const size_t* srcSizes, size_t n, void* const* dsts, const size_t* dstCapacities,
                                             size_t* dstSizes, const ZSTD_CDict* const* cdicts)
{
    return guarded([&] { return compress_batch_cdicts_impl(c, srcs, srcSizes, n, dsts, dstCapacities, dstSizes, cdicts); });
}

// ---- a pack: n device-resident entries into ONE seekable stream (ZSTDMI_compressPack, include/zstd_mi355x.h) ----
// The entries are walked in order and cut into ROUNDS: maximal runs of entries compress_entries batches (entry_batched), at most
// ZSTDMI_CCtx_setPassChunks chunks each.  A round goes through compress_entries into the context's arena, entry i at the prefix sum of
// the ZSTD_compressBound of those in front of it (rounded up to 16 bytes); its sizes come back as a batch's do, the host compares their
// sum with what is left of the capacity, and only then are pack_place (the exclusive scan of the sizes) and pack_gather launched, which
// move each entry's bytes to d_dst + at + its place.  An entry the batch would hand to the single-call path is not staged: the host
// knows the running offset, compress_frames writes it straight to d_dst + at with the capacity that is left.  The table's rows are
// filed on the device — a round's by pack_entries_kernel at rows the host counts from each entry's Framing, an alone entry's by the
// seek table's own mechanism (seekOn) — and read back round by round (8 bytes a frame), so that what the call holds on the device is
// bounded by the round; the table goes up behind the last frame in one copy.  Host synchronisations: per pass and per alone entry
// what the batch and the single call make, plus two per round.
constexpr u64 kPackMaxFrames = (u64)1 << 27;        // (the decoder's limit on a table's entries)
static size_t pack_bound(const size_t* sizes, size_t n)
{
    if (n && !sizes) return ZERR(kErrGeneric);
    size_t sum = 17;
    for (size_t i = 0; i < n; i++) {
        const size_t b = ZSTD_compressBound(sizes[i]), t = 8 * seek_max_frames(sizes[i]);
        if (isErr(b) || b < sizes[i]) return ZERR(kErrSrcSizeWrong);
        if (__builtin_add_overflow(sum, b, &sum) || __builtin_add_overflow(sum, t, &sum) || isErr(sum)) return ZERR(kErrSrcSizeWrong);
    }
    return sum;
}
namespace {
// the stage times of a pack: sums by stage name over its rounds and alone entries, in the order the stages first ran
struct PackStages {
    const char* names[kMaxStages]; float ms[kMaxStages]; int n = 0;
    void add(const char* name, float t)
    {
        for (int i = 0; i < n; i++) if (names[i] == name || !strcmp(names[i], name)) { ms[i] += t; return; }
        if (n < kMaxStages) { names[n] = name; ms[n] = t; n++; }
    }
    void add_call(const ZSTD_CCtx* c) { for (int i = 0; i < c->nStages; i++) add(c->stageNames[i], c->stageMs[i]); }
    void add_timer(ZSTD_CCtx* c) { c->timer.finish(); for (int i = 0; i < c->timer.n; i++) add(c->timer.names[i], c->timer.ms[i]); }
    void file(ZSTD_CCtx* c) const { c->nStages = n; for (int i = 0; i < n; i++) { c->stageNames[i] = names[i]; c->stageMs[i] = ms[i]; } }
};
}
// The pack's rounds for a bound context and the call's parameters (cp.seek off).  withTable = false: the frames alone, no table behind
// them (a cut call without the seek-table switch, compress_cut); st: stage times the caller has gathered in front of the rounds.
static size_t compress_pack_core(ZSTD_CCtx* c, const CallParams& cp, u8* d_dst, size_t dstCapacity, const u8* const* srcs, const size_t* sizes, size_t n,
                                 bool withTable, PackStages st)
{
    size_t e = 0;
    c->lastPackAlone = 0; c->lastPackFrames = 0;
    hipStream_t s = c->stream;
    // what the single call would refuse, for the lowest entry it refuses, before a byte is read
    for (size_t i = 0; i < n; i++) if (sizes[i] && !srcs[i]) return ZERR(kErrSrcSizeWrong);
    if (!d_dst) return dstCapacity ? ZERR(kErrDstBufferNull) : ZERR(kErrDstSizeTooSmall);
    if (n) { e = check_call_params(cp); if (isErr(e)) return e; }
    e = cctx_sync_dictionary(c); if (isErr(e)) return e;
    const DictCTables* const dct = call_dict_ctables(c, cp);
    const u32 passLimit = batch_pass_limit(c);
    // per entry: batched or alone, its chunks and its frames (a batched entry's follow from its Framing).  All of it is a function of
    // the size within one call, and a record store's sizes repeat: resolved once per distinct size
    struct Kind { bool batched; u32 chunks, frames; };
    std::unordered_map<size_t, Kind> kinds;
    std::vector<u8> batched(n); std::vector<u32> chunks(n), frames(n);
    for (size_t i = 0; i < n; i++) {
        const size_t S = sizes[i];
        auto it = kinds.find(S);
        if (it == kinds.end()) {
            if (isErr(ZSTD_compressBound(S)) || ZSTD_compressBound(S) < S) return ZERR(kErrSrcSizeWrong);
            const Framing fr = S ? resolve_framing(c, cp, S) : Framing{};
            Kind k = { S && entry_batched(c, cp, S, fr, passLimit, dct != nullptr, false), 0, 0 };
            if (k.batched) {
                k.chunks = (u32)chunks_of(S, fr.chunkBytes);
                k.frames = fr.frameBlocks ? (k.chunks + fr.frameBlocks - 1) / fr.frameBlocks : k.chunks;
            } else {
                e = check_ldm_dict(c, cp, S); if (isErr(e)) return e;
                e = check_single_frame(c, cp, S); if (isErr(e)) return e;
            }
            it = kinds.emplace(S, k).first;
        }
        batched[i] = it->second.batched; chunks[i] = it->second.chunks; frames[i] = it->second.frames;
    }
    struct Off { ZSTD_CCtx* c; ~Off() { c->seekOn = false; c->seekCount = 0; } } off{c};
    std::vector<u32> table;             // the rows, two words each, in stream order
    std::vector<u8*> slotPtr; std::vector<size_t> slotCap, got; std::vector<u32> seekIdx; std::vector<u64> tab;
    size_t at = 0;
    int alone = 0;
    for (size_t i = 0; i < n; ) {
        if (table.size() / 2 > kPackMaxFrames) return ZERR(kErrParameterUnsupported);
        const size_t room = dstCapacity - at;
        if (!batched[i]) {
            // alone: straight to its place.  Its rows: one frame per call knows its own (the empty frame; one frame across passes,
            // which the seek table's switch refuses), the others file theirs pass by pass as under ZSTDMI_CCtx_setSeekTable
            const size_t S = sizes[i];
            const bool oneFrame = S == 0 || single_active(cp, S) || sliding_active(c, cp, S);
            if (!oneFrame) {
                if (!c->seekEntries.ensure(seek_max_frames(S) * 8)) return ZERR(kErrMemoryAllocation);
                c->seekOn = true; c->seekCount = 0;
            }
            const size_t r = compress_frames(c, cp, d_dst + at, room, srcs[i], S);
            c->seekOn = false;
            if (isErr(r)) return r;
            if (S) st.add_call(c);
            if (oneFrame) { if (r > 0xFFFFFFFFu || S > 0xFFFFFFFFu) return ZERR(kErrGeneric); table.push_back((u32)r); table.push_back((u32)S); }
            else {
                const size_t rows = table.size();
                table.resize(rows + 2 * (size_t)c->seekCount);
                if (c->seekCount && isErr(dev_read(table.data() + rows, c->seekEntries.p, (size_t)c->seekCount * 8, s))) return ZERR(kErrGeneric);
            }
            at += r; ++alone; ++i;
            continue;
        }
        // a round: the batched entries [i, j), cut as compress_entries cuts a pass (batch_pass_cut) from the run of batched entries
        // that begins at i
        const size_t runEnd = batch_run_end(batched.data(), i, std::min(n, i + (size_t)passLimit));
        u32 nCh = 0, nRows = 0; size_t arenaBytes = 0;
        const size_t j = batch_pass_cut(i, runEnd, passLimit, [&](size_t k) { return chunks[k]; }, nCh);
        slotPtr.clear(); slotCap.clear(); seekIdx.clear(); tab.clear();
        for (size_t k = i; k < j; ++k) {
            tab.push_back(arenaBytes); seekIdx.push_back(nRows);
            slotCap.push_back(ZSTD_compressBound(sizes[k]));
            arenaBytes += (slotCap.back() + 15) & ~(size_t)15;
            nRows += frames[k];
        }
        const u32 nEnt = (u32)(j - i);
        tab.push_back(arenaBytes);                                  // slot[nEnt + 1] | size[nEnt] | at[nEnt] (device only)
        if (!c->packArena.ensure(arenaBytes + 64) || !c->seekEntries.ensure((size_t)nRows * 8) || !c->packTab.ensure(((size_t)3 * nEnt + 1) * 8)) return ZERR(kErrMemoryAllocation);
        for (u32 k = 0; k < nEnt; k++) slotPtr.push_back((u8*)c->packArena.p + tab[k]);
        got.assign(nEnt, 0);
        int roundAlone = 0;
        e = compress_entries(c, cp, srcs + i, sizes + i, nEnt, slotPtr.data(), slotCap.data(), got.data(), nullptr, roundAlone, seekIdx.data(), nRows);
        if (isErr(e)) return e;
        if (roundAlone) return ZERR(kErrGeneric);                   // (never: the rounds are cut by compress_entries' own rule)
        st.add_call(c);
        u64 total = 0, longest = 0;
        for (u32 k = 0; k < nEnt; k++) {
            if (isErr(got[k])) return got[k];
            tab.push_back(got[k]); total += got[k]; if (got[k] > longest) longest = got[k];
        }
        if (total > room) return ZERR(kErrDstSizeTooSmall);         // (before anything that writes d_dst is launched)
        u64* const dTab = (u64*)c->packTab.p;
        if (hipMemcpyAsync(dTab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        c->timer.begin(s);
        launch_pack_place(dTab + nEnt + 1, nEnt, dTab + 2 * (size_t)nEnt + 1, s);                    c->timer.mark("pack_place", s);
        launch_pack_gather((const u8*)c->packArena.p, dTab, dTab + nEnt + 1, dTab + 2 * (size_t)nEnt + 1, nEnt, longest, d_dst + at, room, s);
        c->timer.mark("pack_gather", s);
        const size_t rows = table.size();
        table.resize(rows + 2 * (size_t)nRows);
        if (isErr(dev_read(table.data() + rows, c->seekEntries.p, (size_t)nRows * 8, s))) return ZERR(kErrGeneric);
        st.add_timer(c);
        at += (size_t)total; i = j;
    }
    const size_t nFrames = table.size() / 2;
    if (nFrames > kPackMaxFrames) return ZERR(kErrParameterUnsupported);
    if (!withTable) {       // (every round and alone entry has been waited for)
        st.file(c);
        c->lastPackAlone = alone; c->lastPackFrames = (long long)nFrames;
        c->lastChunks = 0;
        return at;
    }
    const size_t tableBytes = 17 + 8 * nFrames;
    if (tableBytes > dstCapacity - at) return ZERR(kErrDstSizeTooSmall);
    // the table behind the last frame: skippable header | rows | footer (include/zstd_mi355x.h "Seekable streams"), in one copy
    std::vector<u8> image(tableBytes);
    frame_put_le(image.data(), 0x184D2A5Eu, 4); frame_put_le(image.data() + 4, tableBytes - 8, 4);
    for (size_t k = 0; k < table.size(); k++) frame_put_le(image.data() + 8 + 4 * k, table[k], 4);
    frame_put_le(image.data() + tableBytes - 9, nFrames, 4); image[tableBytes - 5] = 0; frame_put_le(image.data() + tableBytes - 4, 0x8F92EAB1u, 4);
    c->timer.begin(s);
    if (hipMemcpyAsync(d_dst + at, image.data(), tableBytes, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
    c->timer.mark("pack_table", s);
    if (isErr(stream_wait(s))) return ZERR(kErrGeneric);
    st.add_timer(c);
    st.file(c);
    c->lastPackAlone = alone; c->lastPackFrames = (long long)nFrames;
    c->lastChunks = 0;
    return at + tableBytes;
}
static size_t compress_pack_impl(ZSTD_CCtx* c, u8* d_dst, size_t dstCapacity, const u8* const* srcs, const size_t* sizes, size_t n)
{
    if (!c || (n && (!srcs || !sizes))) return ZERR(kErrGeneric);
    if (c->contentCuts) return ZERR(kErrParameterUnsupported);      // (a pack's entries are the caller's cuts)
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    c->lastRegionList = nullptr; c->lastCarryGroups = 0;
    if (c->workers.size() > 1 || c->pfx) return ZERR(kErrParameterUnsupported);
    CallParams cp = sticky_params(c); cp.seek = false;      // (the context's own switch is not consulted)
    return compress_pack_core(c, cp, d_dst, dstCapacity, srcs, sizes, n, true, PackStages());
}
extern "C" size_t ZSTDMI_packBound(const size_t* srcSizes, size_t n) { return pack_bound(srcSizes, n); }
extern "C" size_t ZSTDMI_compressPack(ZSTD_CCtx* c, void* d_dst, size_t dstCapacity, const void* const* srcs, const size_t* srcSizes, size_t n)
{
    return guarded([&] { return compress_pack_impl(c, (u8*)d_dst, dstCapacity, (const u8* const*)srcs, srcSizes, n); });
}
extern "C" int ZSTDMI_debugLastPackAlone(const ZSTD_CCtx* c) { return c ? c->lastPackAlone : -1; }
extern "C" long long ZSTDMI_debugLastPackFrames(const ZSTD_CCtx* c) { return c ? c->lastPackFrames : -1; }

// ---- content-defined cuts (ZSTDMI_CCtx_setContentCuts, include/zstd_mi355x.h; the rule: zmi_cuts.h) ----
// The pieces of [d_src, d_src + n) by the rule -> their sizes in order.  Two host synchronisations: the candidates' count, which sizes
// the list, and the select's output (the piece count and the ends, one copy sized by the most pieces the rule allows).
// dg (ZSTDMI_contentCutsDigests; null: none): the digest of every piece too — the kernel takes the ends where cut_select left them, over
// a grid sized by the most pieces the rule allows, and its output rides behind the ends in front of the same wait.
struct CutDigests { unsigned kind; std::unique_ptr<u8[]> bytes; };      // bytes: pieces x digest_size(kind), piece after piece
static size_t content_cut_sizes(ZSTD_CCtx* c, const u8* d_src, size_t n, unsigned avgLog, std::vector<size_t>& sizes, PackStages& st, CutDigests* dg = nullptr)
{
    sizes.clear();
    if (!n) return 0;
    if ((u64)n > kCutMaxSrc) return ZERR(kErrParameterUnsupported);
    const CutRule rule = cut_rule(avgLog);
    hipStream_t s = c->stream;
    if (!c->cutSmall.ensure(cut_small_bytes(n))) return ZERR(kErrMemoryAllocation);
    u8* const small = (u8*)c->cutSmall.p;
    c->timer.begin(s);
    launch_cut_count(d_src, n, rule.bits, small, s);
    c->timer.mark("cut_mark", s);
    u32 nCand = 0;
    if (isErr(dev_read(&nCand, cut_total_word(small, n), sizeof nCand, s))) return ZERR(kErrGeneric);
    st.add_timer(c);
    // (a hostile input makes the list as long as the source: the call then fails here, the list is never thinned)
    const u64 P = cut_max_pieces(n, rule);
    if (!c->cutList.ensure((size_t)nCand * 4 + 64) || !c->cutEnds.ensure((size_t)(P + 1) * 4)) return ZERR(kErrMemoryAllocation);
    const size_t dgBytes = dg ? (size_t)P * digest_size(dg->kind) : 0;
    if (dg) { if (!c->digOut.ensure(dgBytes)) return ZERR(kErrMemoryAllocation); dg->bytes.reset(new u8[dgBytes]); }
    c->timer.begin(s);
    if (nCand) launch_cut_emit(d_src, n, rule.bits, small, (u32*)c->cutList.p, s);
    c->timer.mark("cut_mark", s);
    launch_cut_select((const u32*)c->cutList.p, nCand, n, rule, (u32*)c->cutEnds.p, (u32)P, s);
    c->timer.mark("cut_select", s);
    if (dg) {
        launch_digest(dg->kind, d_src, DigestPieces{ nullptr, (const u32*)c->cutEnds.p, P, n }, (u8*)c->digOut.p, s);
        c->timer.mark(digest_stage_name(dg->kind), s);
        if (hipMemcpyAsync(dg->bytes.get(), c->digOut.p, dgBytes, hipMemcpyDeviceToHost, s) != hipSuccess) return ZERR(kErrGeneric);
    }
    std::vector<u32> ends((size_t)P + 1);
    if (isErr(dev_read(ends.data(), c->cutEnds.p, ends.size() * 4, s))) return ZERR(kErrGeneric);
    st.add_timer(c);
    const u64 np = ends[0];
    if (np == 0 || np > P || ends[np] != n) return ZERR(kErrGeneric);
    sizes.reserve(np);
    u64 from = 0;
    for (u64 i = 1; i <= np; ++i) {
        if (ends[i] <= from || ends[i] - from > rule.max) return ZERR(kErrGeneric);
        sizes.push_back((size_t)(ends[i] - from)); from = ends[i];
    }
    return 0;
}
// host memory in, device memory out: the call's source where the kernels can read it
static size_t cut_stage_src(ZSTD_CCtx* c, const void* src, size_t srcSize, bool deviceCall, const u8*& d_src)
{
    d_src = (const u8*)src;
    if (deviceCall || !srcSize || is_device_ptr(src)) return 0;
    if (!c->stageSrc.ensure(srcSize + 64)) return ZERR(kErrMemoryAllocation);
    if (hipMemcpyAsync(c->stageSrc.p, src, srcSize, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ZERR(kErrGeneric);
    d_src = (const u8*)c->stageSrc.p;
    return 0;
}
// ZSTD_compress2 / ZSTDMI_compressDevice / ZSTD_compress_usingCDict with the switch on: the source cut by content, the pieces written as
// ZSTDMI_compressPack writes them — with the seek-table switch its one table behind them, without it the frames alone.
static size_t compress_cut(ZSTD_CCtx* c, const CallParams& cp0, void* dst, size_t dstCapacity, const void* src, size_t srcSize, bool deviceCall)
{
    // what the cut call cannot be, before a byte is read (a pending prefix stays pending)
    if (c->workers.size() > 1 || c->pfx || cp0.single || cp0.ldm == ZSTD_ps_enable || (cp0.windowLog >= 10 && cp0.windowLog <= 15)) return ZERR(kErrParameterUnsupported);
    if ((u64)srcSize > kCutMaxSrc) return ZERR(kErrParameterUnsupported);
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    c->lastRegionList = nullptr; c->lastCarryGroups = 0;
    if (srcSize && !src) return ZERR(kErrSrcSizeWrong);
    if (!dst) return deviceCall && dstCapacity ? ZERR(kErrDstBufferNull) : ZERR(kErrDstSizeTooSmall);
    CallParams cp = cp0; cp.seek = false;
    const u8* d_src; e = cut_stage_src(c, src, srcSize, deviceCall, d_src); if (isErr(e)) return e;
    const bool dstDev = deviceCall || is_device_ptr(dst);
    u8* d_dst = (u8*)dst; size_t devCap = dstCapacity;
    if (!dstDev) {
        u64 worst = 0;
        if (!cut_bound(srcSize, cut_rule((unsigned)c->contentCuts), &worst)) return ZERR(kErrSrcSizeWrong);
        devCap = dstCapacity < worst ? dstCapacity : (size_t)worst;
        if (!c->stageDst.ensure(devCap + 64)) return ZERR(kErrMemoryAllocation);
        d_dst = (u8*)c->stageDst.p;
    }
    PackStages st;
    std::vector<size_t> sizes;
    e = content_cut_sizes(c, d_src, srcSize, (unsigned)c->contentCuts, sizes, st); if (isErr(e)) return e;
    std::vector<const u8*> srcs(sizes.size());
    { size_t at = 0; for (size_t i = 0; i < sizes.size(); i++) { srcs[i] = d_src + at; at += sizes[i]; } }
    const size_t r = compress_pack_core(c, cp, d_dst, devCap, srcs.data(), sizes.data(), sizes.size(), cp0.seek, st);
    if (isErr(r)) return r;
    c->lastContentCuts = (long long)sizes.size();
    if (!dstDev && r) {
        if (hipMemcpyAsync(dst, d_dst, r, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return ZERR(kErrGeneric);
        if (isErr(stream_wait(c->stream))) return ZERR(kErrGeneric);
    }
    return r;
}
// kind 0: ZSTDMI_contentCuts; else ZSTDMI_contentCutsDigests, the same call with every piece's digest behind it
static size_t content_cuts_impl(ZSTD_CCtx* c, const void* src, size_t srcSize, unsigned avgLog, size_t* pieceSizes, size_t capacity, size_t* nPieces,
                                bool withDigests = false, unsigned kind = 0, void* digests = nullptr, size_t digestsCapacity = 0)
{
    if (!c || !nPieces || (capacity && !pieceSizes) || (withDigests && digestsCapacity && !digests)) return ZERR(kErrGeneric);
    *nPieces = 0;
    if (!cut_avglog_ok(avgLog)) return ZERR(kErrParameterOutOfBound);
    if (withDigests && !digest_size(kind)) return ZERR(kErrParameterOutOfBound);
    if ((u64)srcSize > kCutMaxSrc) return ZERR(kErrParameterUnsupported);
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    if (srcSize && !src) return ZERR(kErrSrcSizeWrong);
    const u8* d_src; e = cut_stage_src(c, src, srcSize, false, d_src); if (isErr(e)) return e;
    PackStages st;
    std::vector<size_t> sizes;
    CutDigests dg{ kind, nullptr };
    e = content_cut_sizes(c, d_src, srcSize, avgLog, sizes, st, withDigests ? &dg : nullptr); if (isErr(e)) return e;
    st.file(c);
    *nPieces = sizes.size();
    const size_t dgBytes = sizes.size() * digest_size(kind);        // (at most srcSize / 1024 + 1 pieces of 32 bytes: no overflow)
    if (sizes.size() > capacity || (withDigests && dgBytes > digestsCapacity)) return ZERR(kErrDstSizeTooSmall);
    for (size_t i = 0; i < sizes.size(); i++) pieceSizes[i] = sizes[i];
    if (withDigests && dgBytes) memcpy(digests, dg.bytes.get(), dgBytes);
    return 0;
}
// ZSTDMI_digestPieces: the answers in the header's order; the context lends its device, stream, workspaces and stage timer
static size_t digest_pieces_impl(ZSTD_CCtx* c, const void* src, size_t srcSize, const size_t* pieceSizes, size_t nPieces, unsigned kind,
                                 void* digests, size_t digestsCapacity)
{
    if (!c) return ZERR(kErrGeneric);
    if (nPieces && (!pieceSizes || !digests)) return ZERR(kErrGeneric);
    const size_t each = digest_size(kind);
    if (!each) return ZERR(kErrParameterOutOfBound);
    if (!nPieces) return 0;
    size_t outBytes = 0;
    if (__builtin_mul_overflow(nPieces, each, &outBytes) || outBytes > digestsCapacity) return ZERR(kErrDstSizeTooSmall);
    { size_t sum = 0; for (size_t i = 0; i < nPieces; i++) if (__builtin_add_overflow(sum, pieceSizes[i], &sum) || sum > srcSize) return ZERR(kErrSrcSizeWrong); }
    if (srcSize && !src) return ZERR(kErrSrcSizeWrong);
    if (c->workers.size() > 1) return ZERR(kErrParameterUnsupported);
    if ((u64)nPieces >= (1ull << 31)) return ZERR(kErrParameterUnsupported);       // (the grid's reach)
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    const u8* d_src; e = cut_stage_src(c, src, srcSize, false, d_src); if (isErr(e)) return e;
    std::vector<u64> offs(nPieces + 1);
    { u64 at = 0; for (size_t i = 0; i < nPieces; i++) { offs[i] = at; at += pieceSizes[i]; } offs[nPieces] = at; }
    hipStream_t s = c->stream;
    if (!c->digOffs.ensure(offs.size() * sizeof(u64)) || !c->digOut.ensure(outBytes)) return ZERR(kErrMemoryAllocation);
    if (hipMemcpyAsync(c->digOffs.p, offs.data(), offs.size() * sizeof(u64), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
    c->timer.begin(s);
    launch_digest(kind, d_src, DigestPieces{ (const u64*)c->digOffs.p, nullptr, (u64)nPieces, (u64)srcSize }, (u8*)c->digOut.p, s);
    c->timer.mark(digest_stage_name(kind), s);
    if (isErr(dev_read(digests, c->digOut.p, outBytes, s))) return ZERR(kErrGeneric);
    PackStages st; st.add_timer(c); st.file(c);
    return 0;
}
extern "C" size_t ZSTDMI_CCtx_setContentCuts(ZSTD_CCtx* c, unsigned avgLog)
{
    if (!c) return ZERR(kErrGeneric);
    if (avgLog && !cut_avglog_ok(avgLog)) return ZERR(kErrParameterOutOfBound);
    c->contentCuts = (int)avgLog; c->paramGen++;
    return 0;
}
extern "C" size_t ZSTDMI_contentCutsBound(size_t srcSize, unsigned avgLog)
{
    if (!cut_avglog_ok(avgLog)) return ZERR(kErrParameterOutOfBound);
    u64 b = 0;
    if (!cut_bound(srcSize, cut_rule(avgLog), &b) || b > (u64)(size_t)-1 || isErr((size_t)b)) return ZERR(kErrSrcSizeWrong);
    return (size_t)b;
}
extern "C" size_t ZSTDMI_contentCuts(ZSTD_CCtx* c, const void* d_src, size_t srcSize, unsigned avgLog, size_t* pieceSizes, size_t capacity, size_t* nPieces)
{
    return guarded([&] { return content_cuts_impl(c, d_src, srcSize, avgLog, pieceSizes, capacity, nPieces); });
}
extern "C" long long ZSTDMI_debugLastContentCuts(const ZSTD_CCtx* c) { return c ? c->lastContentCuts : -1; }

// ---- piece digests (include/zstd_mi355x.h "Piece digests"; zmi_digest.h, digest.hip) ----
extern "C" size_t ZSTDMI_digestSize(unsigned kind) { return digest_size(kind); }
extern "C" size_t ZSTDMI_digestPieces(ZSTD_CCtx* c, const void* src, size_t srcSize, const size_t* pieceSizes, size_t nPieces, unsigned kind,
                                      void* digests, size_t digestsCapacity)
{
    return guarded([&] { return digest_pieces_impl(c, src, srcSize, pieceSizes, nPieces, kind, digests, digestsCapacity); });
}
extern "C" size_t ZSTDMI_contentCutsDigests(ZSTD_CCtx* c, const void* src, size_t srcSize, unsigned avgLog, unsigned kind,
                                            size_t* pieceSizes, size_t capacity, size_t* nPieces, void* digests, size_t digestsCapacity)
{
    return guarded([&] { return content_cuts_impl(c, src, srcSize, avgLog, pieceSizes, capacity, nPieces, true, kind, digests, digestsCapacity); });
}
extern "C" size_t ZSTDMI_debugDigestModel(unsigned kind, const void* src, size_t srcSize, void* digest)
{
    if (!digest_size(kind)) return ZERR(kErrParameterOutOfBound);
    if (!digest || (srcSize && !src)) return ZERR(kErrGeneric);
    (void)digest_serial(kind, (const u8*)src, srcSize, (u8*)digest);
    return 0;
}

// ---- cuts and digests enqueued from the device (include/zstd_mi355x.h "Cuts and digests enqueued from the device") ----
// the limits as the prepare takes them: 0, or what both ZSTDMI_cutsAsyncWorkspace and the prepare answer before a device is looked for
static size_t cuts_limits_resolve(const ZSTDMI_CutLimits* L, CutsPrep& P)
{
    if (!L) return ZERR(kErrGeneric);
    if (!L->srcSizeBound || (u64)L->srcSizeBound > kCutMaxSrc || !cut_avglog_ok(L->avgLog) || L->kind > 2 || L->reserved[0] || L->reserved[1] || L->reserved[2])
        return ZERR(kErrParameterOutOfBound);
    const CutRule rule = cut_rule(L->avgLog);
    u64 cand = L->maxCandidates ? (u64)L->maxCandidates : 4 * ((u64)L->srcSizeBound >> rule.bits) + 1024;
    if (cand > kCutsAsyncMaxCand) cand = kCutsAsyncMaxCand;         // (node indices are words)
    P.bound = L->srcSizeBound; P.avgLog = L->avgLog; P.kind = L->kind; P.maxCand = (u32)cand;
    P.maxPieces = cut_max_pieces(P.bound, rule); P.digestSize = (u32)digest_size(L->kind);
    P.lay = cuts_async_layout(P.bound, cand, P.maxPieces, P.digestSize);
    return 0;
}
static size_t prepare_cuts_async_impl(ZSTD_CCtx* c, const ZSTDMI_CutLimits* L)
{
    if (!c || !L) return ZERR(kErrGeneric);
    cctx_drop_cuts_prepare(c);
    CutsPrep P;
    size_t e = cuts_limits_resolve(L, P); if (isErr(e)) return e;
    if (c->workers.size() > 1) return ZERR(kErrParameterUnsupported);
    e = cctx_bind(c); if (isErr(e)) return e;
    if (!c->cutsAsync.ensure(P.lay.bytes)) return ZERR(kErrMemoryAllocation);
    if (!c->asyncEv && hipEventCreateWithFlags(&c->asyncEv, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); c->asyncEv = nullptr; return ZERR(kErrMemoryAllocation); }
    c->cutsPrep = new CutsPrep(P);
    return 0;
}
// Kernels only, on the context's stream: the synchronous call's count, the bounded emit, the parallel selection, the fused digest over
// the ends where the selection left them, and the finish that files everything the caller reads.  The host knows srcSize and the
// prepared limits and nothing else: every grid and the round count come from them.
static size_t content_cuts_async_impl(ZSTD_CCtx* c, const u8* d_src, size_t srcSize, size_t* d_pieceSizes, const void** d_pieceSrcs, size_t capacity,
                                      void* d_digests, size_t digestsCapacity, size_t* d_nPieces, size_t* d_status)
{
    if (!c || !d_nPieces || !d_status || (capacity && !d_pieceSizes)) return ZERR(kErrGeneric);
    const CutsPrep* const P = c->cutsPrep;
    if (!P || !c->deviceOk) return ZERR(kErrStageWrong);
    if ((d_digests != nullptr) != (P->kind != 0)) return ZERR(kErrGeneric);
    if ((u64)srcSize > P->bound || (srcSize && !d_src)) return ZERR(kErrSrcSizeWrong);
    const size_t e = cctx_bind(c); if (isErr(e)) return e;
    hipStream_t s = c->stream;
    u8* const ws = (u8*)c->cutsAsync.p;
    const CutsAsyncLayout& L = P->lay;
    u32* const ends = (u32*)(ws + L.atEnds);
    const CutRankWs rk = cut_rank_ws(ws, L);
    const CutRule rule = cut_rule(P->avgLog);
    const u64 n = srcSize, most = cut_max_pieces(n, rule);
    if (n) {
        u8* const small = ws + L.atSmall; u32* const list = (u32*)(ws + L.atList);
        launch_cut_count(d_src, n, rule.bits, small, s);
        launch_cut_emit_bounded(d_src, n, rule.bits, small, list, P->maxCand, s);
        launch_cut_rank(list, cut_total_word(small, n), P->maxCand, n, rule, rk, ends, (u32)P->maxPieces, s);
        if (P->kind) launch_digest(P->kind, d_src, DigestPieces{ nullptr, ends, most, n }, ws + L.atDigests, s);
    }
    launch_cuts_finish(CutsFinishArgs{ ends, rk.state, (u32)P->maxPieces, d_src, n, most, d_pieceSizes, d_pieceSrcs, capacity,
                                       ws + L.atDigests, (u8*)d_digests, digestsCapacity, P->digestSize, d_nPieces, d_status }, s);
    return async_enqueued(c, s);
}
// the selection alone over a host list (synchronous; buffers of its own, freed before it returns)
static size_t debug_cut_select_parallel_impl(ZSTD_CCtx* c, const unsigned* cands, size_t nCand, unsigned long long n, unsigned avgLog, unsigned* outEnds, size_t cap, size_t* nEnds)
{
    if (!c || !nEnds || (nCand && !cands) || (cap && !outEnds)) return ZERR(kErrGeneric);
    *nEnds = 0;
    if (!cut_avglog_ok(avgLog)) return ZERR(kErrParameterOutOfBound);
    if (n > kCutMaxSrc || (u64)nCand > n || (u64)nCand > kCutsAsyncMaxCand) return ZERR(kErrSrcSizeWrong);
    size_t e = cctx_bind(c); if (isErr(e)) return e;
    const CutRule rule = cut_rule(avgLog);
    const u64 P = cut_max_pieces(n, rule);
    const u32 room = (u32)nCand, endsCap = (u32)((u64)cap < P ? (u64)cap : P);
    const CutsAsyncLayout L = cuts_async_layout(1, room, endsCap, 0);
    DevBuf buf;
    struct Free { DevBuf& b; ~Free() { b.release(); } } freeIt{ buf };
    if (!buf.ensure(L.bytes)) return ZERR(kErrMemoryAllocation);
    hipStream_t s = c->stream;
    u8* const ws = (u8*)buf.p;
    u32* const list = (u32*)(ws + L.atList); u32* const total = (u32*)(ws + L.atSmall); u32* const ends = (u32*)(ws + L.atEnds);
    const CutRankWs rk = cut_rank_ws(ws, L);
    if ((nCand && hipMemcpyAsync(list, cands, nCand * 4, hipMemcpyHostToDevice, s) != hipSuccess) ||
        hipMemcpyAsync(total, &room, 4, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
    launch_cut_rank(list, total, room, n, rule, rk, ends, endsCap, s);
    u32 state[2] = { 0, 0 };
    if (isErr(dev_read(state, rk.state, sizeof state, s))) return ZERR(kErrGeneric);
    *nEnds = state[0];
    if (state[1]) return ZERR(kErrWorkSpaceTooSmall);
    if (state[0] > cap) return ZERR(kErrDstSizeTooSmall);
    if (state[0] && isErr(dev_read(outEnds, ends + 1, (size_t)state[0] * 4, s))) return ZERR(kErrGeneric);
    return 0;
}
// the stages of one enqueued call on the prepared workspace, timed by events and waited for (tools/cuts_async_time.py): ms[0] = count and
// bounded emit, ms[1] = the selection, ms[2] = the digests (0 without a kind).  The caller's arrays are not involved: no finish.
static size_t debug_cuts_async_stages_impl(ZSTD_CCtx* c, const u8* d_src, size_t srcSize, float* ms)
{
    if (!c || !ms) return ZERR(kErrGeneric);
    const CutsPrep* const P = c->cutsPrep;
    if (!P || !c->deviceOk) return ZERR(kErrStageWrong);
    if (!srcSize || (u64)srcSize > P->bound || !d_src) return ZERR(kErrSrcSizeWrong);
    const size_t e = cctx_bind(c); if (isErr(e)) return e;
    hipStream_t s = c->stream;
    hipEvent_t ev[4] = {};
    struct Free { hipEvent_t* ev; ~Free() { for (int i = 0; i < 4; i++) if (ev[i]) (void)hipEventDestroy(ev[i]); } } freeThem{ ev };
    for (auto& x : ev) if (hipEventCreate(&x) != hipSuccess) { (void)hipGetLastError(); x = nullptr; return ZERR(kErrMemoryAllocation); }
    u8* const ws = (u8*)c->cutsAsync.p;
    const CutsAsyncLayout& L = P->lay;
    u8* const small = ws + L.atSmall; u32* const list = (u32*)(ws + L.atList); u32* const ends = (u32*)(ws + L.atEnds);
    const CutRule rule = cut_rule(P->avgLog);
    const u64 n = srcSize;
    (void)hipEventRecord(ev[0], s);
    launch_cut_count(d_src, n, rule.bits, small, s);
    launch_cut_emit_bounded(d_src, n, rule.bits, small, list, P->maxCand, s);
    (void)hipEventRecord(ev[1], s);
    launch_cut_rank(list, cut_total_word(small, n), P->maxCand, n, rule, cut_rank_ws(ws, L), ends, (u32)P->maxPieces, s);
    (void)hipEventRecord(ev[2], s);
    if (P->kind) launch_digest(P->kind, d_src, DigestPieces{ nullptr, ends, cut_max_pieces(n, rule), n }, ws + L.atDigests, s);
    (void)hipEventRecord(ev[3], s);
    if (isErr(stream_wait(s))) return ZERR(kErrGeneric);
    for (int i = 0; i < 3; i++) { ms[i] = 0; (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]); }
    return 0;
}
extern "C" size_t ZSTDMI_debugCutsAsyncStages(ZSTD_CCtx* c, const void* d_src, size_t srcSize, float* ms)
{
    return guarded([&] { return debug_cuts_async_stages_impl(c, (const u8*)d_src, srcSize, ms); });
}
extern "C" size_t ZSTDMI_cutsAsyncWorkspace(const ZSTDMI_CutLimits* limits)
{
    CutsPrep P;
    const size_t e = cuts_limits_resolve(limits, P);
    return isErr(e) ? e : P.lay.bytes;
}
extern "C" size_t ZSTDMI_CCtx_prepareCutsAsync(ZSTD_CCtx* c, const ZSTDMI_CutLimits* limits) { return guarded([&] { return prepare_cuts_async_impl(c, limits); }); }
extern "C" size_t ZSTDMI_CCtx_getCutsAsyncPlan(const ZSTD_CCtx* c, size_t* maxPieces, size_t* maxCandidates, size_t* digestSize)
{
    if (!c) return ZERR(kErrGeneric);
    const CutsPrep* const P = c->cutsPrep;
    if (!P) return ZERR(kErrStageWrong);
    if (maxPieces) *maxPieces = (size_t)P->maxPieces;
    if (maxCandidates) *maxCandidates = P->maxCand;
    if (digestSize) *digestSize = P->digestSize;
    return 0;
}
extern "C" size_t ZSTDMI_contentCutsAsync(ZSTD_CCtx* c, const void* d_src, size_t srcSize, size_t* d_pieceSizes, const void** d_pieceSrcs, size_t capacity,
                                          void* d_digests, size_t digestsCapacity, size_t* d_nPieces, size_t* d_status)
{
    return guarded([&] { return content_cuts_async_impl(c, (const u8*)d_src, srcSize, d_pieceSizes, d_pieceSrcs, capacity, d_digests, digestsCapacity, d_nPieces, d_status); });
}
extern "C" size_t ZSTDMI_debugCutSelectParallel(ZSTD_CCtx* c, const unsigned* cands, size_t nCand, unsigned long long n, unsigned avgLog,
                                                unsigned* ends, size_t cap, size_t* nEnds)
{
    return guarded([&] { return debug_cut_select_parallel_impl(c, cands, nCand, n, avgLog, ends, cap, nEnds); });
}

extern "C" size_t ZSTDMI_debugCompressSamples(ZSTD_CCtx* c, const void* src, const size_t* sizes, size_t n, size_t* outSizes)
{
    if (!c || (n && (!sizes || !outSizes))) return ZERR(kErrGeneric);
    if (c->contentCuts) return ZERR(kErrParameterUnsupported);
    return guarded([&] {
        std::vector<u64> offs(n);
        u64 o = 0; for (size_t i = 0; i < n; i++) { offs[i] = o; o += sizes[i]; }
        if (o && !src) return ZERR(kErrSrcSizeWrong);
        return compress_samples(c, (const u8*)src, offs.data(), sizes, n, outSizes, nullptr);
    });
}
