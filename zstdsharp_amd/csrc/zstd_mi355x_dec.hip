// zstd_mi355x_dec.hip — the decoder's host side: the decompression context, its parameters and dictionary, the host-side frame-header
// functions, the launch sequences of the decompress pipeline (one buffer, a batch, a range and many ranges of a seekable stream,
// several devices), the ZSTD_decompressStream adapter and every decoder entry point of the C ABI (include/zstd_mi355x.h).
#include <stdlib.h>
#include <stdio.h>
#include <functional>
#include "zmi_pack_runs.h"
#include "zmi_stream_scan.h"
#include "zmi_host.h"
#include "zmi_dictid.h"

struct ZSTD_DCtx_s {
    int windowLogMax = 27;
    int device = 0; bool deviceOk = false;
    hipStream_t ownStream = nullptr, stream = nullptr;
    hipStream_t aux = nullptr; hipEvent_t auxDone = nullptr;     // the literal decoder beside seq_decode (decompress_device)
    int overlapMode = 0;        // ZSTDMI_DCtx_setOverlap: 0 = by block count, 1 = never, 2 = always
    bool lastWalkSerial = false; // the last call's frames were listed by the serial walk (ZSTDMI_debugLastWalkSerial)
    int execWaves = 0;          // ZSTDMI_DCtx_setExecWaves: waves per frame in exec_matches, 0 = by the number of frames
    DevBuf frames, blocks, recs, status, scratch, walkWs, slowFlags, stageSrc, stageDst, origin, originList;
    PinBuf pin;                 // the status words as the host reads them (status_read)
    DevBuf seqPlane;            // one u32 per block: the sequences it files records for (block_prepass writes it, seq_scan sums it)
    DevBuf sizePlane;           // one u64 per frame, only in a call with frames without a content size: their regenerated sizes (block_offsets writes it, frame_rescan sums it)
    DevBuf farPlane;            // one u32 per sequence record, only in a call with a far-capable frame (kRecFar, zmi_common.h; decompress_device)
    int lastFarPlane = 0;       // the last decompress_device run had one (ZSTDMI_debugLastFarPlane)
    DevBuf batchIn, batchOut, blockKeys;    // ZSTDMI_decompressBatch: the entries' table, what the batch walk made of them, one error key per block
    int lastBatchAlone = 0;     // entries of the last ZSTDMI_decompressBatch that were decoded by the single-call path (debug hook)
    // ZSTDMI_DCtx_setBatchUnsized: 1 = an entry of a batch / range(s) call that holds a frame without a content size takes the shared
    // pass (decode_entries) instead of going alone.  litRooms: one u64 per frame of such a pass, the room its literals have in the scratch
    int batchUnsized = 0;
    DevBuf litRooms;
    long long lastBatchWs = 0;  // device bytes the last decode_entries run asked its work buffers for (ZSTDMI_debugLastBatchWorkspace)
    DevBuf seekTab, seekSum, edge;          // ZSTDMI_decompressRange: a host source's seek table, the summary words, the frames the range cuts
    int lastRangeFrames = 0; long long lastRangeStaged = 0;     // table entries the last range call decoded, bytes it copied host -> device (debug hooks)
    // ZSTDMI_decompressRanges: the pass's workspace (RangesWs), the ranges as the host states them / as ranges_select files them /
    // their results, and the arena that holds every touched frame's content once
    DevBuf rangesWs, rangesIn, rangesRec, rangesRes, arena;
    int lastRangesFrames = 0, lastRangesAlone = 0; long long lastRangesStaged = 0;      // (debug hooks)
    int originMode = 0;         // ZSTDMI_DCtx_setLongFrames: 0 = by cost (see decompress_device), 1 = never, 2 = every frame of 1 MiB or more
    StageTimer timer;
    // streaming adapter (ZSTD_decompressStream): whole frames are collected on the host, decoded in batches
    std::vector<u8> dIn, dOut; size_t dOutPos = 0; bool hostage = false;
    // ZSTDMI_DCtx_setStreamSegment: a frame that is still arriving is decoded in segments, runs of whole blocks; `seg`
    // is what one segment leaves for the next.  dIn then starts at the first block that has not been decoded yet.
    size_t segBytes = 0;        // 0 = off: whole frames only
    struct CarriedBlock { std::vector<u8> bytes; u32 defines; };        // a block (header and body) that defines a live table
    struct SegBlock { size_t off, size; u32 defines; };                 // a whole block of dIn, scanned and not yet decoded
    struct StreamSeg {
        bool active = false;    // inside a frame
        bool first = true;      // no segment of it decoded yet: repcodes from the dictionary or the format's
        bool lastSeen = false;  // `blocks` ends with the frame's last block (and the checksum behind it is there)
        u8 hdr[12] = {}; u32 hdrLen = 0;        // the header every fragment begins with
        u8 lastByte = 0;        // (source of a one-byte copy)
        u64 histKeep = 0;       // bytes of history a later block may reach once the frame has produced a window: the window, at most
                                // what a sequence record can name.  Until then everything is kept: the format lets a block reach the
                                // WHOLE dictionary while the frame's output has not exceeded the window (ZSTD_checkDictValidity)
        u64 window = 0;         // the window the header declares (a single-segment frame: its content size)
        XxhCarry xxhHost = {};  // (source and target of the checksum state's asynchronous copies)
        u64 blockMax = 0;       // the bound of a block's content as the fragment's header states it: min(window, 128 KiB)
        u64 fcs = ~0ull, produced = 0; bool checksum = false;
        std::vector<CarriedBlock> carried;      // at most four, in stream order
        std::vector<SegBlock> blocks; size_t scanned = 0;
        u64 histLen = 0; int histCur = 0;
        u64 skip = 0;           // bytes of a skippable frame still to drop
    } seg;
    DevBuf hist[2], segReps, segXxh;            // the history (rolled from one buffer into the other), the repcode triple (a DictInfo), the XXH64 state
    int streamSegments = 0; long long streamPeakInput = 0;      // (debug hooks; the setter zeroes them)
    u32 litDecoder = 0;         // 0 auto, 1 serial (4 lanes per frame), 2 self-synchronising (256 lanes per frame), 3 serial with compact tables
    // dictionary (ZSTD_DCtx_loadDictionary): host copy, uploaded at the next decompression.  Raw content: the bytes are the
    // history.  Formatted (magic 0xEC30A437): dict_parse_kernel validates the header and fills `info`; the history is the content.
    std::vector<u8> dictHost; DevBuf dict, dictInfoDev; bool dictDirty = false, dictFormatted = false;
    DictInfo info = {};
    u64 dictGen = 0;
    // ZSTD_DCtx_refDDict: a digested dictionary, referenced.  decode_dict() hands the kernels its device copies and ready-made
    // sequence tables where they can be shared (ddict_shared); elsewhere the fields above hold a private copy of its bytes (dctx_adopt_ddict)
    const ZSTD_DDict_s* ddict = nullptr;
    long long dictUploads = 0;          // uploads this context made itself (ZSTDMI_debugDictUploadsD)
    long long lastDictTabBlocks = 0;    // blocks of the last call that copied a ready-made table (ZSTDMI_debugLastDictTableBlocks)
    // ZSTD_d_refMultipleDDicts (U/ZstdDecompress.cs:8-115, 2300-2339): while the parameter is 1, ZSTD_DCtx_refDDict also files the DDict in
    // ddictSet (references, sorted by dictID; lives until ZSTD_freeDCtx).  With a DDict current and two or more in the set, a decode call
    // runs the kernels' set instances over slotTab: the set's sorted image (zmi_dictset.h) with the current DDict's record behind it,
    // uploaded by the first call after setGen moved (dctx_sync_slots).
    int refMultiple = 0;
    DictSet<const ZSTD_DDict_s*> ddictSet;
    std::vector<DictSlot> slotHost; DevBuf slotTab;
    u64 setGen = 0, slotGen = ~(u64)0;  // setGen: bumped when the set, the current DDict or the context's device changes
    u64 foreignGen = ~(u64)0; bool foreign = false;     // (at setGen == foreignGen) some DDict of the set lives on another device
    long long lastSetFrames = 0;        // frames of the last call whose dictionary was found in the set (ZSTDMI_debugLastSetFrames)
    std::vector<ZSTD_DCtx_s*> workers;      // ZSTDMI_DCtx_setDevices (decompress_multi)
    // ZSTD_DCtx_refPrefix: the caller's bytes (host or device), referenced until the next ZSTD_decompressDCtx / ZSTDMI_decompressDevice
    // has consumed them.  pfxDev: the prefix as that call's kernels read it (the caller's device pointer, or pfxStage for a host prefix)
    const void* pfx = nullptr; size_t pfxSize = 0; DevBuf pfxStage; const u8* pfxDev = nullptr;
    // ZSTDMI_DCtx_prepareBatchAsync / ZSTDMI_decompressBatchAsync: what the prepare resolved (asyncPrep: host state only,
    // valid while dctx_gen() is what it was then; paramGen: bumped by every setter whatever it sets), the plan's verdicts, and the event
    // recorded behind the last enqueued call (asyncPending: not yet waited for).  dctx_async_drain is the one place that waits for it;
    // every buffer of the context names `tally`, so that no growth or release frees memory an enqueued call still uses, and counts there.
    HostTally tally; u64 paramGen = 0;
    struct DAsyncPrep* asyncPrep = nullptr; hipEvent_t asyncEv = nullptr; bool asyncPending = false;
    DevBuf asyncVerdict;
    // ZSTDMI_DCtx_prepareRangesAsync / ZSTDMI_decompressRangesAsync: the other kind of prepare — a context holds one of
    // the two, dctx_drop_prepares is what every prepare begins with — and the prepared stream's index, a RangesWs of its own: the
    // synchronous range calls index into rangesWs on every call and must not disturb this one
    struct DRangesPrep* rangesPrep = nullptr;
    DevBuf rangesAsyncWs;
    ZSTD_DCtx_s();
};
// what either prepare resolved: dctx_gen() as it was then, and the limits with their defaults filled in (the decode core lays its lists out from them)
struct DPrepCore { u64 gen; BatchLimitsD lim; };
struct DAsyncPrep : DPrepCore { size_t maxEntries; u64 bound; };
// (the stream too: the caller keeps its bytes; its table as the footer and seek_index state it; the rows of the decode core's table)
struct DRangesPrep : DPrepCore { size_t maxRanges; u64 maxRangeBytes; const u8* src; const u8* tab; u32 n, stride; u64 total; u32 nRows; };
static void dctx_drop_prepares(ZSTD_DCtx* d) { delete d->asyncPrep; d->asyncPrep = nullptr; delete d->rangesPrep; d->rangesPrep = nullptr; }
static void dctx_async_drain(ZSTD_DCtx* d);
ZSTD_DCtx_s::ZSTD_DCtx_s()
{
    tally.self = this; tally.beforeFree = [](void* self) { dctx_async_drain((ZSTD_DCtx_s*)self); };
    for (DevBuf* b : { &frames, &blocks, &recs, &status, &scratch, &walkWs, &slowFlags, &stageSrc, &stageDst, &origin, &originList, &farPlane, &batchIn, &batchOut, &blockKeys, &litRooms,
                       &seekTab, &seekSum, &edge, &rangesWs, &rangesIn, &rangesRec, &rangesRes, &arena, &hist[0], &hist[1], &segReps, &segXxh, &dict, &dictInfoDev, &slotTab,
                       &pfxStage, &asyncVerdict, &rangesAsyncWs, &seqPlane, &sizePlane }) b->owner = &tally;
    pin.owner = &tally;
}
// The lifetime rule of an enqueued batch (ZSTDMI_decompressBatchAsync), in one place: wait for the event behind the last enqueued call.
// Called by every DevBuf of the context before it frees (HostTally::beforeFree: growth and release alike), by ZSTD_freeDCtx, by
// ZSTDMI_DCtx_setStream to another stream, by ZSTD_DCtx_loadDictionary and ZSTD_DCtx_refDDict, and in front of a re-upload of the
// dictionary or of the DDict set's slot table (the device must be current).
static void dctx_async_drain(ZSTD_DCtx* d)
{
    if (!d->asyncPending) return;
    d->asyncPending = false;
    d->tally.waits++;
    if (hipEventSynchronize(d->asyncEv) != hipSuccess) (void)hipGetLastError();
}
// moves whenever a prepare may have become stale: a setter, the dictionary in force, the DDict set or the device
static u64 dctx_gen(const ZSTD_DCtx* d) { return d->paramGen + d->dictGen + d->setGen; }

// ZSTD_createDDict: a dictionary uploaded, validated and digested once on `device`, immutable afterwards (any number of contexts and
// threads read it without a lock): the bytes with 64 readable ones behind them, DictInfo, and for a formatted dictionary its three
// sequence decoding tables ready-made in seq_decode_kernel's LDS format (seqTabs: kDictTabWords words, decode_seq.hip).
struct ZSTD_DDict_s { std::vector<u8> host; DevBuf dict, dictInfoDev, seqTabs; DictInfo info = {}; bool formatted = false; int device = 0; };
static bool ddict_shared(const ZSTD_DCtx* d) { return d->ddict && d->ddict->device == d->device && d->workers.size() <= 1; }
// the set is in force: frames select their DDict by dictID (a set of one is the single-DDict path, private upload included)
static bool set_active(const ZSTD_DCtx* d) { return d->refMultiple && d->ddict && d->ddictSet.size() >= 2; }
// what a decode call answers before it reads a byte: the set's kernels serve one device and whole frames only.  Touches no device.
static size_t set_check(ZSTD_DCtx* d, bool segmented = false)
{
    if (!set_active(d)) return 0;
    if (d->workers.size() > 1 || segmented || !ddict_shared(d)) return ZERR(kErrParameterUnsupported);
    if (d->foreignGen != d->setGen) {
        d->foreign = false;
        for (const auto& e : d->ddictSet.entries) if (e.ref->device != d->device) { d->foreign = true; break; }
        d->foreignGen = d->setGen;
    }
    return d->foreign ? ZERR(kErrParameterUnsupported) : 0;
}

static size_t dctx_sync_dictionary(ZSTD_DCtx* d);
// (inside an ABI call's guarded(): the waits of this thread count for this context from here on, see HostTally)
static size_t dctx_bind(ZSTD_DCtx* d)
{
    if (d && tl_guarded) tl_waits = &d->tally.waits;
    const size_t e = ctx_bind(d); if (isErr(e)) return e;
    if (!d->aux && hipStreamCreateWithFlags(&d->aux, hipStreamNonBlocking) != hipSuccess) return ZERR(kErrMemoryAllocation);
    if (!d->auxDone && hipEventCreateWithFlags(&d->auxDone, hipEventDisableTiming) != hipSuccess) return ZERR(kErrMemoryAllocation);
    return 0;
}

extern "C" {

// ---------------- decompression ----------------
ZSTD_DCtx* ZSTD_createDCtx(void) { return new (std::nothrow) ZSTD_DCtx_s(); }
size_t ZSTD_freeDCtx(ZSTD_DCtx* d)
{
    if (!d) return 0;
    for (ZSTD_DCtx* w : d->workers) (void)ZSTD_freeDCtx(w);
    d->workers.clear();
    if (tl_waits == &d->tally.waits) tl_waits = nullptr;
    if (d->deviceOk) {
        (void)hipSetDevice(d->device);
        dctx_async_drain(d);        // (an enqueued batch may run on a stream that is not the context's own)
        if (d->asyncEv) (void)hipEventDestroy(d->asyncEv);
        d->asyncVerdict.release(); d->rangesAsyncWs.release();
        if (d->ownStream) (void)hipStreamSynchronize(d->ownStream);
        d->frames.release(); d->blocks.release(); d->recs.release(); d->status.release(); d->scratch.release(); d->walkWs.release(); d->slowFlags.release(); d->stageSrc.release(); d->stageDst.release(); d->dict.release(); d->dictInfoDev.release(); d->origin.release(); d->originList.release(); d->farPlane.release(); d->batchIn.release(); d->batchOut.release(); d->blockKeys.release(); d->litRooms.release(); d->seekTab.release(); d->seekSum.release(); d->edge.release(); d->pfxStage.release(); d->rangesWs.release(); d->rangesIn.release(); d->rangesRec.release(); d->rangesRes.release(); d->arena.release(); d->slotTab.release();
        d->hist[0].release(); d->hist[1].release(); d->segReps.release(); d->segXxh.release(); d->seqPlane.release(); d->sizePlane.release(); d->pin.release();
        d->timer.destroy();
        if (d->aux) { (void)hipStreamSynchronize(d->aux); (void)hipStreamDestroy(d->aux); }
        if (d->auxDone) (void)hipEventDestroy(d->auxDone);
        if (d->ownStream) (void)hipStreamDestroy(d->ownStream);
    }
    dctx_drop_prepares(d);
    delete d;
    return 0;
}
size_t ZSTD_DCtx_setParameter(ZSTD_DCtx* d, int param, int value)
{
    if (!d) return ZERR(kErrGeneric);
    d->paramGen++;
    if (param == ZSTD_d_windowLogMax) { if (value != 0 && (value < 10 || value > 31)) return ZERR(kErrParameterOutOfBound); d->windowLogMax = value ? value : 27; return 0; }
    if (param == ZSTD_d_refMultipleDDicts) {        // sticky; the set itself stays as it is (U/ZstdDecompress.cs:2441-2447)
        if (value != ZSTD_rmd_refSingleDDict && value != ZSTD_rmd_refMultipleDDicts) return ZERR(kErrParameterOutOfBound);
        d->refMultiple = value;
        return 0;
    }
    return ZERR(kErrParameterUnsupported);
}
size_t ZSTD_DCtx_getParameter(ZSTD_DCtx* d, int param, int* value)
{
    if (!d || !value) return ZERR(kErrGeneric);
    if (param == ZSTD_d_windowLogMax) { *value = d->windowLogMax; return 0; }
    if (param == ZSTD_d_refMultipleDDicts) { *value = d->refMultiple; return 0; }
    return ZERR(kErrParameterUnsupported);
}
// ZSTD_decompress_insertDictionary, U/ZstdDecompress.cs:1909-1931: without the magic the bytes are raw content, history in
// front of every frame (ZSTD_refDictContent, :1758-1771); with it (0xEC30A437) the header's Huffman and FSE tables and
// repcodes are what every frame starts from and frames must name its dictID or none (ZSTD_loadDEntropy, :1773-1875).
static size_t ZSTD_DCtx_loadDictionary_impl(ZSTD_DCtx* d, const void* dict, size_t dictSize)
{
    if (!d) return ZERR(kErrGeneric);
    if (tl_guarded) tl_waits = &d->tally.waits;
    if (d->deviceOk && hipSetDevice(d->device) == hipSuccess) dctx_async_drain(d);      // (an enqueued batch reads the dictionary it was prepared behind)
    d->dictGen++;
    d->pfx = nullptr; d->pfxSize = 0;       // (a pending prefix is cancelled: ZSTD_clearAllDicts)
    d->ddict = nullptr;                     // (and a referenced DDict)
    if (dict == nullptr || dictSize == 0) { d->dictHost.clear(); d->dictDirty = true; return 0; }
    if (dictSize > (size_t)1 << 30) return ZERR(kErrParameterUnsupported);
    std::vector<u8> h(dictSize);
    if (is_device_ptr(dict)) {
        if (hipMemcpy(h.data(), dict, dictSize, hipMemcpyDeviceToHost) != hipSuccess) return ZERR(kErrGeneric);
    } else memcpy(h.data(), dict, dictSize);
    d->dictFormatted = is_formatted_dictionary(h.data(), dictSize);
    d->dictHost.swap(h);
    d->dictDirty = true;
    if (d->dictFormatted && !isErr(dctx_bind(d))) return dctx_sync_dictionary(d);      // validated now when a device is there, else at first use
    d->dictDirty = true;
    return 0;
}

// Host-side header walk for host buffers (ZSTD_findFrameSizeInfo, U/ZstdDecompress.cs:877-951): headers only, no payload.
static size_t host_frame_size_info(const u8* src, size_t srcSize, unsigned long long* bound)
{
    auto rd32 = [](const u8* p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); };
    if (srcSize >= 4 && (rd32(src) & 0xFFFFFFF0u) == 0x184D2A50u) {
        if (srcSize < 8) return ZERR(kErrSrcSizeWrong);         // a skippable frame's header that is still arriving: wait, as for a zstd frame's
        const u64 sz = (u64)rd32(src + 4) + 8;
        if (sz > srcSize) return ZERR(kErrSrcSizeWrong);
        *bound = 0; return (size_t)sz;
    }
    if (srcSize < 5) return ZERR(kErrSrcSizeWrong);
    if (rd32(src) != 0xFD2FB528u) return ZERR(kErrPrefixUnknown);
    const u8 fhd = src[4];
    static const size_t did[4] = { 0, 1, 2, 4 }, fcsB[4] = { 0, 2, 4, 8 };
    const u32 single = (fhd >> 5) & 1, fcsId = fhd >> 6;
    const size_t fhs = 5 + !single + did[fhd & 3] + fcsB[fcsId] + (single && !fcsId);
    if (srcSize < fhs) return ZERR(kErrSrcSizeWrong);
    if (fhd & 0x08) return ZERR(kErrFrameParameterUnsupported);
    size_t pos = 5; u64 windowSize = 0, fcs = ~0ull;
    if (!single) { const u8 wl = src[pos++]; const u32 wlog = (wl >> 3) + 10; if (wlog > 31) return ZERR(kErrWindowTooLarge); windowSize = 1ull << wlog; windowSize += (windowSize >> 3) * (wl & 7); }
    pos += did[fhd & 3];
    switch (fcsId) {
    case 0: if (single) fcs = src[pos]; break;
    case 1: fcs = (u64)((u32)src[pos] | ((u32)src[pos + 1] << 8)) + 256; break;
    case 2: fcs = rd32(src + pos); break;
    default: fcs = (u64)rd32(src + pos) | ((u64)rd32(src + pos + 4) << 32); break;
    }
    if (single) windowSize = fcs;
    const u64 blockSizeMax = windowSize < (1u << 17) ? windowSize : (1u << 17);
    const u8* ip = src + fhs; size_t remaining = srcSize - fhs; u64 nbBlocks = 0;
    for (;;) {
        if (remaining < 3) return ZERR(kErrSrcSizeWrong);
        const u32 bh = (u32)ip[0] | ((u32)ip[1] << 8) | ((u32)ip[2] << 16);
        const u32 last = bh & 1, type = (bh >> 1) & 3; u32 cSize = bh >> 3;
        if (type == 3) return ZERR(kErrCorruption);
        if (type == 1) cSize = 1;
        if (3 + (size_t)cSize > remaining) return ZERR(kErrSrcSizeWrong);
        ip += 3 + cSize; remaining -= 3 + cSize; nbBlocks++;
        if (last) break;
    }
    if ((fhd >> 2) & 1) { if (remaining < 4) return ZERR(kErrSrcSizeWrong); ip += 4; }
    *bound = fcs != ~0ull ? fcs : nbBlocks * blockSizeMax;
    return (size_t)(ip - src);
}

// Window size a frame header declares (ZSTD_getFrameHeader_advanced, U/ZstdDecompress.cs:462-634): the window descriptor, or the
// content size of a single-segment frame.  0 = not a zstd frame header, or not all of it is there yet.
static u64 host_frame_window(const u8* src, size_t srcSize)
{
    auto rd32 = [](const u8* p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); };
    if (srcSize < 5 || rd32(src) != 0xFD2FB528u) return 0;
    const u8 fhd = src[4];
    static const size_t did[4] = { 0, 1, 2, 4 }, fcsB[4] = { 0, 2, 4, 8 };
    const u32 single = (fhd >> 5) & 1, fcsId = fhd >> 6;
    const size_t fhs = 5 + !single + did[fhd & 3] + fcsB[fcsId] + (single && !fcsId);
    if (srcSize < fhs) return 0;
    if (!single) { const u8 wl = src[5]; const u32 wlog = (wl >> 3) + 10; if (wlog > 31) return ~0ull; const u64 w = 1ull << wlog; return w + (w >> 3) * (wl & 7); }
    const size_t pos = 5 + did[fhd & 3];
    switch (fcsId) {
    case 0: return src[pos];
    case 1: return (u64)((u32)src[pos] | ((u32)src[pos + 1] << 8)) + 256;
    case 2: return rd32(src + pos);
    default: return (u64)rd32(src + pos) | ((u64)rd32(src + pos + 4) << 32);
    }
}

static const u8* host_view(const void* src, size_t srcSize, std::vector<u8>& tmp)
{
    if (!is_device_ptr(src)) return (const u8*)src;
    tmp.resize(srcSize);
    if (hipMemcpy(tmp.data(), src, srcSize, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
    return tmp.data();
}

static unsigned long long ZSTD_decompressBound_impl(const void* src, size_t srcSize)
{
    std::vector<u8> tmp; const u8* ip = srcSize ? host_view(src, srcSize, tmp) : (const u8*)src;
    if (srcSize && !ip) return (unsigned long long)0 - 2;
    unsigned long long bound = 0;
    while (srcSize > 0) {
        unsigned long long b = 0; const size_t cs = host_frame_size_info(ip, srcSize, &b);
        if (isErr(cs)) return (unsigned long long)0 - 2;
        ip += cs; srcSize -= cs; bound += b;
    }
    return bound;
}
static size_t ZSTD_findFrameCompressedSize_impl(const void* src, size_t srcSize)
{
    std::vector<u8> tmp; const u8* ip = host_view(src, srcSize, tmp);
    if (!ip) return ZERR(kErrSrcSizeWrong);
    unsigned long long b; return host_frame_size_info(ip, srcSize, &b);
}
static unsigned long long ZSTD_getFrameContentSize_impl(const void* src, size_t srcSize)
{
    std::vector<u8> tmp; const size_t look = srcSize < 18 ? srcSize : 18;
    const u8* ip = look ? host_view(src, look, tmp) : nullptr;
    if (!ip || look < 5) return (unsigned long long)0 - 2;
    auto rd32 = [](const u8* p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); };
    if ((rd32(ip) & 0xFFFFFFF0u) == 0x184D2A50u) return 0;
    if (rd32(ip) != 0xFD2FB528u) return (unsigned long long)0 - 2;
    const u8 fhd = ip[4]; static const size_t did[4] = { 0, 1, 2, 4 }, fcsB[4] = { 0, 2, 4, 8 };
    const u32 single = (fhd >> 5) & 1, fcsId = fhd >> 6;
    const size_t fhs = 5 + !single + did[fhd & 3] + fcsB[fcsId] + (single && !fcsId);
    if (look < fhs) return (unsigned long long)0 - 2;
    size_t pos = 5 + !single + did[fhd & 3];
    switch (fcsId) {
    case 0: return single ? ip[pos] : (unsigned long long)0 - 1;
    case 1: return (u64)((u32)ip[pos] | ((u32)ip[pos + 1] << 8)) + 256;
    case 2: return rd32(ip + pos);
    default: return (u64)rd32(ip + pos) | ((u64)rd32(ip + pos + 4) << 32);
    }
}

// upload a newly loaded dictionary; a formatted one is validated on the device (ZSTD_loadDEntropy's checks) -> dictionary_corrupted
static size_t dctx_sync_dictionary(ZSTD_DCtx* d)
{
    if (ddict_shared(d) || !d->dictDirty) return 0;     // (a shared DDict is on the device already)
    dctx_async_drain(d);        // (a re-upload writes what an enqueued batch may still read)
    hipStream_t s = d->stream;
    if (!d->dictHost.empty()) {
        d->dictUploads++;
        if (!d->dict.ensure(d->dictHost.size() + 64) || !d->dictInfoDev.ensure(sizeof(DictInfo))) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(d->dict.p, d->dictHost.data(), d->dictHost.size(), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        if (d->dictFormatted) {
            launch_dict_parse((const u8*)d->dict.p, (u32)d->dictHost.size(), (DictInfo*)d->dictInfoDev.p, s);
            if (hipMemcpyAsync(&d->info, d->dictInfoDev.p, sizeof(DictInfo), hipMemcpyDeviceToHost, s) != hipSuccess) return ZERR(kErrGeneric);
        }
        { const size_t e = stream_wait(s); if (isErr(e)) return e; }
        if (d->dictFormatted && d->info.err) { d->dictHost.clear(); d->dictFormatted = false; d->dictDirty = false; return ZERR(kErrDictionaryCorrupted); }
    }
    d->dictDirty = false;
    return 0;
}

// the loaded dictionary as the decode kernels take it (DecodeDict, zmi_host.h; slots: dctx_sync_slots)
// a dictionary as its owner holds it (a DDict, or the context's private copy): formatted or raw, its bytes on the host (0: none), the parsed
// header there, the device copies.  dict_fields is the one place that derives the kernels' fields from it.
struct DictView { bool formatted; size_t bytes; const DictInfo& info; const void* dev; const void* infoDev; const void* seqTabs; };
static DictView ddict_view(const ZSTD_DDict_s& g) { return { g.formatted, g.host.size(), g.info, g.dict.p, g.dictInfoDev.p, g.seqTabs.p }; }
static DecodeDict dict_fields(const DictView& v)
{
    DecodeDict k;
    k.slots = nullptr; k.nSet = 0;
    k.fmt = v.formatted && v.bytes;
    k.dictFull = k.fmt ? (const u8*)v.dev : nullptr;
    k.dinfo = k.fmt ? (const DictInfo*)v.infoDev : nullptr;
    k.dictContent = v.bytes ? (const u8*)v.dev + (k.fmt ? v.info.contentOff : 0u) : nullptr;
    k.dictContentSize = v.bytes ? (k.fmt ? v.info.contentSize : (u32)v.bytes) : 0u;
    k.dictID = k.fmt ? v.info.dictID : 0u;
    k.seqTabs = k.fmt ? (const u32*)v.seqTabs : nullptr;
    return k;
}
static DecodeDict decode_dict(const ZSTD_DCtx* d)
{
    if (ddict_shared(d)) return dict_fields(ddict_view(*d->ddict));
    return dict_fields(DictView{ d->dictFormatted, d->dictHost.size(), d->info, d->dict.p, d->dictInfoDev.p, nullptr });
}

// a DDict as a record of the slot table (what decode_dict says of a shared one)
static void fill_slot(const ZSTD_DDict_s* g, DictSlot& r)
{
    r = DictSlot{};
    if (!g || g->host.empty()) return;
    const DecodeDict k = dict_fields(ddict_view(*g));
    r.formatted = k.fmt ? 1u : 0u; r.dictFull = k.dictFull; r.content = k.dictContent; r.contentSize = k.dictContentSize; r.seqTabs = k.seqTabs;
    if (!k.fmt) return;
    r.dictID = g->info.dictID;
    r.hufOff = g->info.hufOff; r.hufSize = g->info.hufSize; r.ofOff = g->info.ofOff; r.mlOff = g->info.mlOff; r.llOff = g->info.llOff; r.repOff = g->info.repOff;
    for (int i = 0; i < 3; ++i) r.rep[i] = g->info.rep[i];
}
// The set for this call (after set_check): nothing while it is not in force; else the slot table, uploaded when the set, the current
// DDict or the device changed since the last upload — one small copy on the context's stream, in front of the kernels that read it.
static size_t dctx_sync_slots(ZSTD_DCtx* d, DecodeDict& dd)
{
    dd.slots = nullptr; dd.nSet = 0;
    if (!set_active(d) || d->pfxDev) return 0;
    if (d->slotGen != d->setGen) {
        dctx_async_drain(d);    // (as for the dictionary)
        if (!d->ddictSet.image(d->slotHost, d->ddict, fill_slot)) return ZERR(kErrMemoryAllocation);
        if (!d->slotTab.ensure(d->slotHost.size() * sizeof(DictSlot) + 64)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(d->slotTab.p, d->slotHost.data(), d->slotHost.size() * sizeof(DictSlot), hipMemcpyHostToDevice, d->stream) != hipSuccess) return ZERR(kErrGeneric);
        { const size_t e = stream_wait(d->stream); if (isErr(e)) return e; }       // (slotHost may change before the next call's kernels run)
        d->slotGen = d->setGen;
    }
    dd.slots = (const DictSlot*)d->slotTab.p; dd.nSet = (u32)d->ddictSet.size();
    return 0;
}
// the DecodeDict of a call: the dictionary uploaded where it is new, viewed as the kernels take it, the set's slot table behind it
static size_t call_dict(ZSTD_DCtx* d, DecodeDict& dd)
{
    const size_t e = dctx_sync_dictionary(d); if (isErr(e)) return e;
    dd = decode_dict(d);
    return dctx_sync_slots(d, dd);
}

// the status words (d->status, kSt*): error key = "none" (all ones), everything else zero — stores of a one-wave kernel, no upload
static size_t status_reset(ZSTD_DCtx* d)
{
    launch_status_reset((u32*)d->status.p, d->stream);
    return 0;
}
// The host's view of the status words: d->pin (PinBuf, zmi_host.h), kStWords words that a kernel of the call's stream fills — the
// mirror kernel, or a single-workgroup stage that is the last to write the words the host wants next (walk_link, seq_scan: they get
// the block as an argument) — and that the host copies out behind its wait.  status_wait: the wait and the copy alone.
static bool status_pin(ZSTD_DCtx* d) { return d->pin.ensure(kStWords * sizeof(u32)); }
static size_t status_wait(ZSTD_DCtx* d, u32* st)
{
    const size_t e = stream_wait(d->stream); if (isErr(e)) return e;
    memcpy(st, d->pin.p, kStWords * sizeof(u32));
    return 0;
}
static size_t status_read(ZSTD_DCtx* d, u32* st)
{
    if (!status_pin(d)) return ZERR(kErrMemoryAllocation);
    launch_status_mirror((const u32*)d->status.p, (u32*)d->pin.p, d->stream);
    return status_wait(d, st);
}
static u64 st_u64(const u32* st, u32 lo, u32 hi) { return (u64)st[lo] | ((u64)st[hi] << 32); }

// how a run ended (0: well): the first failing block's first error, then the run's own (unsized frames regenerated more than the destination holds)
static size_t status_error(const u32* st)
{
    if (st[kStErrKeyLo] != 0xFFFFFFFFu || st[kStErrKeyHi] != 0xFFFFFFFFu) return ZERR(st[kStErrKeyLo] & 0xFFFFu);
    return st[kStErr] ? ZERR(st[kStErr]) : 0;
}

// The work lists of a run over nFrames frames and nBlocks blocks with `content` bytes of literals, stated once: each buffer's bytes, and
// where behind the frames' skewed literals the dump area of a pass with open entries lies (withDump: the scratch holds it; the open
// kernel instances and batch_init_d_kernel find it through the status words).  blockKeys and litRooms are the batch's.
struct ListsLayout { size_t frames, blocks, scratch, slowFlags, blockKeys, litRooms; u64 dumpOff; };
static ListsLayout lists_layout(u32 nFrames, u32 nBlocks, u64 content, bool withDump)
{
    ListsLayout l;
    l.dumpOff = content + (u64)nFrames * kLitSkew + 256;
    l.frames = (size_t)nFrames * sizeof(FrameDesc); l.blocks = (size_t)nBlocks * sizeof(BlockDesc) + 64;
    l.scratch = (size_t)l.dumpOff + (withDump ? kLitDump : 0u);
    l.slowFlags = (size_t)nBlocks + 64; l.blockKeys = (size_t)nBlocks * sizeof(u64) + 8; l.litRooms = (size_t)nFrames * sizeof(u64);
    return l;
}
// (the four every run has)
static bool ensure_lists(ZSTD_DCtx* d, const ListsLayout& l) { return d->frames.ensure(l.frames) && d->blocks.ensure(l.blocks) && d->scratch.ensure(l.scratch) && d->slowFlags.ensure(l.slowFlags); }
// exec_matches' waves per frame: the setter's, else by the number of frames (64 x W sequences in flight per frame: measured on 1 - 4 MiB level-5 frames)
static int exec_waves_for(const ZSTD_DCtx* d, u32 n) { return d->execWaves ? d->execWaves : n <= 256 ? 16 : n <= 512 ? 8 : n <= 1024 ? 4 : n <= 2048 ? 2 : 1; }

// Everything behind the frame walk: the lists (d->frames, d->blocks; offsets relative to d_src and d_dst) through block_prepass,
// seq_decode, block_offsets, the literal decoder, the origin path and exec_matches.  `tail` enqueues what the caller wants read back
// with the last status read (-> false: failed); st = the status words after it.  -> 0 or the error of the whole run.
// `link` (a fragment of a segmented stream, decode_fragment): the first link->phantoms blocks only define tables, and the frame's
// repcodes start from link->reps where that is not NULL.
// `open` (a batch whose lists hold entries with unsized frames, decode_entries): block_link and block_offsets run their open instances,
// and batch_rescan_kernel settles those entries' places behind block_offsets, in front of everything that writes into a destination
// (the literal decoder beside seq_decode writes only where block_link found the place final).
// `far` (decompress_device alone): some frame of the lists may reach further back than a record's 29 offset bits — seq_decode,
// exec_matches and origin_init run their far instances over d->farPlane, one u32 per record (4 bytes per sequence of such a call).
struct StreamLink { u32 phantoms; const DictInfo* reps; };
struct OpenEntries { const BatchEntryIn* in; BatchEntryOut* out; u32 n; };
static size_t decode_lists(ZSTD_DCtx* d, const DecodeDict& dd, u8* d_dst, const u8* d_src, u32 nFrames, u32 nBlocks, u32 nUnsized, size_t dstCapacity, u32* st, const std::function<bool()>& tail,
                           const StreamLink* link = nullptr, const OpenEntries* open = nullptr, bool far = false)
{
    hipStream_t s = d->stream;
    u32* status = (u32*)d->status.p;
    FrameDesc* frames = (FrameDesc*)d->frames.p; BlockDesc* blocks = (BlockDesc*)d->blocks.p;
    // (dd.slots not null: every stage below runs its set instance and reads the dictionary per frame)
    // The literal decoder and seq_decode need nothing of each other (a block's Huffman streams and its FSE chains).  With few
    // blocks neither fills the chip — both are serial chains per block — so below kOverlapBlocks the literal decoder may run beside
    // seq_decode on a stream of its own (`early`: block_link then lets it write only the outputs whose place is known by now).
    // Whether it does is decided once the pre-pass has counted both kinds of work (below).
    constexpr u32 kOverlapBlocks = 12288;
    // Not in a single call of several frames with an unsized one among them: a sized frame behind an unsized one has, until
    // frame_rescan, a dstOff computed from the bound in front of it, and block_link (which knows a frame's header, not its
    // neighbours) would let its first block be written there.  (A batch marks such frames itself: kFrameOpen.)
    const bool early = !(nUnsized && nFrames > 1) && (d->overlapMode == 2 || (d->overlapMode == 0 && nBlocks <= kOverlapBlocks));
    if (!d->seqPlane.ensure((size_t)nBlocks * sizeof(u32) + 64) || !status_pin(d)) return ZERR(kErrMemoryAllocation);
    if (nUnsized && !d->sizePlane.ensure((size_t)nFrames * sizeof(u64) + 64)) return ZERR(kErrMemoryAllocation);
    launch_block_prepass(d_src, frames, blocks, nFrames, nBlocks, dd, early ? 1u : 0u, status, s, (u32*)d->seqPlane.p, (u32*)d->pin.p, link ? link->phantoms : 0u, open != nullptr);
    { const size_t e = status_wait(d, st); if (isErr(e)) return e; }       // (seq_scan has filed the status words in the pinned block itself)
    d->timer.mark("block_prepass", s);
    const u64 nSeq = st_u64(st, kStSeqLo, kStSeqHi);
    if (!d->recs.ensure((size_t)(nSeq + 64) * sizeof(SeqRec))) return ZERR(kErrMemoryAllocation);
    if (far && !d->farPlane.ensure((size_t)(nSeq + 64) * sizeof(u32))) return ZERR(kErrMemoryAllocation);
    u32* const farPlane = far ? (u32*)d->farPlane.p : nullptr;
    // Long frames (decode_origin.hip).  The ordered walk of exec_matches moves a frame at about kWalkRate, all frames at
    // once; the origin path sweeps the frames it is given at about kSweepRate together.  A frame belongs on the origin path when its
    // own walk would outlast the sweep of every frame at least as long: the smallest size class 2^(20+k) with
    // 2^(20+k) / kWalkRate >= bytes(frames >= 2^(20+k)) / kSweepRate, from the per-class sums block_link filed.
    u64 originMin = 0, originBytes = 0, originLongest = 0; u32 originCap = 0;
    const int execWaves = exec_waves_for(d, nFrames);
    if (d->originMode != 1) {
        const double kWalkRate = execWaves >= 16 ? 0.42e9 : execWaves == 8 ? 0.33e9 : execWaves == 4 ? 0.24e9 : execWaves == 2 ? 0.19e9 : 0.15e9;
        constexpr double kSweepRate = 20e9;
        u64 above = 0;
        u64 sums[12];
        for (int k = 0; k < 12; ++k) sums[k] = st_u64(st, kStBigBins + 2 * k, kStBigBins + 2 * k + 1);
        for (int k = 11; k >= 0; --k) {
            above += sums[k];
            if (!above) continue;
            const double size = (double)((u64)1 << (20 + k));
            if (d->originMode == 2 || size / kWalkRate >= (double)above / kSweepRate) { originMin = (u64)1 << (20 + k); originBytes = above; }
        }
        if (originMin) {
            // how many frames that can be (a frame of class k holds at least 2^(20+k) bytes) and how long the longest (below 2^(21+k))
            u64 cap = 0;
            for (int k = 0; k < 12; ++k) if (((u64)1 << (20 + k)) >= originMin && sums[k]) { cap += sums[k] >> (20 + k); originLongest = (u64)1 << (21 + k); }
            if (originLongest > originBytes) originLongest = originBytes;
            originCap = (u32)(cap < 65535 ? cap : 65535);       // (a grid dimension; more long frames than that keep the walk)
            // (+ one word per 1024 origins: origin_jump_kernel's finished regions)
            if (!d->origin.ensure((size_t)(originBytes + 1024 * (u64)originCap) * sizeof(u32) + (size_t)((originBytes + 1024 * (u64)originCap) / 1024 + 64) * sizeof(u32)) ||
                !d->originList.ensure((size_t)originCap * sizeof(u32))) { originMin = 0; (void)hipGetLastError(); }
        }
    }
    SeqRec* recs = (SeqRec*)d->recs.p;
    struct AuxGuard { hipStream_t a; bool on; ~AuxGuard() { if (on) (void)hipStreamSynchronize(a); } } auxGuard{ d->aux, false };   // nothing of this call outlives it
    // Beside each other only when both are substantial (from five coded literal bytes per sequence): a Huffman symbol costs its chain
    // about 26 ns per literal byte (four streams), a sequence about 270 ns — text (three or four literal bytes per sequence) has nothing to hide behind seq_decode and only loses LDS
    // bandwidth to the company (measured: 1 GiB of 1 MiB level-5 frames, mixed corpus 14.7 -> 13.4 ms, text 15.5 -> 15.7 ms), and
    // input without sequences (Zipf bytes) has no seq_decode to hide behind.
    const u64 litBytes = st_u64(st, kStLitLo, kStLitHi);
    const bool beside = early && nSeq && (d->overlapMode == 2 || (litBytes >= 5 * nSeq && nSeq >= 64 * (u64)nBlocks));
    if (getenv("ZMI_DEBUG")) fprintf(stderr, "zmi: blocks %u seqs %llu coded literal bytes %llu early %d beside %d\n", nBlocks, (unsigned long long)nSeq, (unsigned long long)litBytes, (int)early, (int)beside);
    if (beside) {               // (the host has just waited for the pre-pass: everything the literal decoder reads is there)
        launch_decode_literals(d_src, d_dst, (u8*)d->scratch.p, frames, blocks, nBlocks, status, (u8*)d->slowFlags.p, d->litDecoder, dd, d->aux, StageHook());
        if (hipEventRecord(d->auxDone, d->aux) != hipSuccess) return ZERR(kErrGeneric);
        auxGuard.on = true;
    }
    launch_seq_decode(d_src, frames, blocks, nBlocks, recs, status, dd, s, farPlane);     d->timer.mark("seq_decode", s);
    launch_block_offsets(frames, blocks, nFrames, dd, link && link->reps ? link->reps : dd.dinfo, nUnsized ? (u64*)d->sizePlane.p : nullptr, dstCapacity, status, s, open != nullptr);  d->timer.mark("block_offsets", s);
    if (open) { launch_batch_rescan(open->in, open->out, open->n, frames, s); d->timer.mark("batch_rescan", s); }
    if (auxGuard.on) { if (hipStreamWaitEvent(s, d->auxDone, 0) != hipSuccess) return ZERR(kErrGeneric); d->timer.mark("decode_literals", s); }     // (what of it seq_decode did not cover)
    else launch_decode_literals(d_src, d_dst, (u8*)d->scratch.p, frames, blocks, nBlocks, status, (u8*)d->slowFlags.p, d->litDecoder, dd, s, d->timer.hook());
    launch_place_literals(d_src, d_dst, (const u8*)d->scratch.p, frames, blocks, nBlocks, recs, status, s);    d->timer.mark("place_literals", s);
    if (originMin) {
        const u64 entries = originBytes + 1024 * (u64)originCap, longest = originLongest;
        u32* const origin = (u32*)d->origin.p; const u32* const list = (const u32*)d->originList.p;
        launch_origin_select(frames, nFrames, originMin, (u32*)d->originList.p, originCap, entries, status, s);
        launch_origin_init(frames, blocks, list, originCap, longest, recs, status, origin, dd, s, farPlane);    d->timer.mark("origin_init", s);
        // The rounds in groups of six, the host looking at the last one's verdict in between: ordinary data settles in about ten
        // rounds, and a round that only finds out that nothing is left still costs its launch (the kernels check the flag too).
        for (u32 r = 0; r < kOriginRounds; r += 6) {
            launch_origin_jump(frames, list, originCap, longest, status, origin, origin + entries, r, r + 6, s);
            u32 open = 0;
            const u32 lastRound = (r + 6 < kOriginRounds ? r + 6 : kOriginRounds) - 1;
            { const size_t e = dev_read(&open, status + kStOriginChanged + lastRound, sizeof(u32), s); if (isErr(e)) return e; }
            if (!open) break;
        }
        d->timer.mark("origin_jump", s);
        launch_origin_gather(frames, list, originCap, longest, status, origin, d_dst, dd, s);    d->timer.mark("origin_gather", s);
    }
    launch_exec_matches(d_src, d_dst, frames, blocks, nFrames, recs, status, dd, s, execWaves, farPlane);  d->timer.mark("exec_matches", s);
    if (!tail()) return ZERR(kErrGeneric);
    { const size_t e = status_read(d, st); if (isErr(e)) return e; }
    d->lastDictTabBlocks += st[kStDictTabBlocks];
    return 0;
}

// The decompress pipeline over device-resident buffers.  Two host round trips size the work lists (frames + blocks after the
// counting walk, sequence records after the block pre-pass); everything else is one launch sequence.  A round trip is a wait and a read
// of the context's pinned block (status_wait): walk_link and seq_scan, the kernels in front of the two waits, file the status words
// there themselves, and the mirror kernel does at the end of the call — no copy between device and pageable memory stands in a call.
//   walk (count) | walk (emit) -> block_parse -> block_link -> seq_scan | seq_decode -> block_offsets [-> frame_rescan]
//   -> decode_literals -> place_literals -> exec_matches
// allowFar = false (an entry that a batch, range or ranges call left to this path): offsets above kRecOffMax keep the refusal those calls state
static size_t decompress_device(ZSTD_DCtx* d, u8* d_dst, size_t dstCapacity, const u8* d_src, size_t srcSize, bool allowFar = true)
{
    hipStream_t s = d->stream;
    if (srcSize == 0) return 0;
    // a frame is at least 9 bytes; our own streams hold one per 64 KiB, foreign ones usually far fewer
    const u32 maxFrames = (u32)((srcSize / 9 + 1) < (1u << 26) ? (srcSize / 9 + 1) : (1u << 26));
    if (!d->status.ensure(kStWords * sizeof(u32)) || !d->walkWs.ensure(decode_walk_workspace_bytes(srcSize))) return ZERR(kErrMemoryAllocation);
    u32* status = (u32*)d->status.p;
    DecodeDict dd;
    { const size_t e = call_dict(d, dd); if (isErr(e)) return e; }
    if (d->pfxDev) { dd.dictContent = d->pfxDev; dd.dictContentSize = (u32)d->pfxSize; }      // ZSTD_DCtx_refPrefix: raw content, read where it lies
    d->timer.begin(s);
    { const size_t e = status_reset(d); if (isErr(e)) return e; }
    u32 st[kStWords] = {};
    if (!status_pin(d)) return ZERR(kErrMemoryAllocation);
    launch_frame_walk_count(d_src, srcSize, maxFrames, status, (u8*)d->walkWs.p, s, (u32*)d->pin.p);
    { const size_t e = status_wait(d, st); if (isErr(e)) return e; }      // (walk_link has filed its words in the pinned block itself)
    const bool serialWalk = !st[kStUsable];
    d->lastWalkSerial = serialWalk;
    // (the parallel walk lists only frames that name no dictionary: all of them are the current DDict's, the single-dictionary kernels' case)
    if (!serialWalk) { dd.slots = nullptr; dd.nSet = 0; }
    if (serialWalk) {   // the segment links did not close: take the exact serial walk (it also yields the reference's error code)
        launch_frame_walk_serial(d_src, srcSize, nullptr, nullptr, maxFrames, status, dd, 0, s);
        const size_t e = status_read(d, st); if (isErr(e)) return e;
        if (dd.slots) d->lastSetFrames += st[kStSetFrames];
    }
    if (st[kStErr]) return ZERR(st[kStErr]);
    const u32 nFrames = st[kStFrames], nBlocks = st[kStBlocks], nUnsized = st[kStUnsized];
    const u64 total = st_u64(st, kStTotalLo, kStTotalHi);       // content sizes (bounds for frames without one)
    if (!nUnsized && total > dstCapacity) return ZERR(kErrDstSizeTooSmall);
    if (nFrames == 0) { d->timer.finish(); return 0; }
    if (!ensure_lists(d, lists_layout(nFrames, nBlocks, total, false))) return ZERR(kErrMemoryAllocation);
    FrameDesc* frames = (FrameDesc*)d->frames.p; BlockDesc* blocks = (BlockDesc*)d->blocks.p;
    if (serialWalk) launch_frame_walk_serial(d_src, srcSize, frames, blocks, maxFrames, status, dd, 1, s);
    else            launch_frame_walk_emit(d_src, srcSize, frames, blocks, (u8*)d->walkWs.p, s);
    d->timer.mark("frame_walk", s);
    // A far-capable frame: its content (an unsized frame: its bound) plus the dictionary or prefix content in front of it exceeds what a
    // record's offset bits name.  `total` is the sum over the call's frames and the dictionary the largest a frame can have, so the test
    // errs toward the plane; seq_decode's far instance holds each block to its own frame's reach.
    u64 dictReach = dd.dictContent ? dd.dictContentSize : 0u;
    if (dd.slots) for (const DictSlot& r : d->slotHost) if (r.content && r.contentSize > dictReach) dictReach = r.contentSize;
    const bool far = allowFar && total + dictReach > kRecOffMax;
    d->lastFarPlane = far ? 1 : 0;
    { const size_t e = decode_lists(d, dd, d_dst, d_src, nFrames, nBlocks, nUnsized, dstCapacity, st, [] { return true; }, nullptr, nullptr, far); if (isErr(e)) return e; }
    d->timer.finish();
    { const size_t e = status_error(st); if (isErr(e)) return e; }
    if (nUnsized) return (size_t)st_u64(st, kStActualLo, kStActualHi);
    return (size_t)total;
}

// ---- a batch of independent entries, each decoded as the single call would decode it alone (ZSTDMI_decompressBatch) ----
// The decoder's unit of parallelism is the block and its lists hold 64-bit offsets, so n entries are ONE run of the pipeline: the
// batch walk (one lane per entry, the exact serial walk) lists every entry's frames and blocks side by side, with offsets relative to
// the lowest source and the lowest destination pointer of the call, and block_prepass .. exec_matches run once over the merged lists.
// Errors stay with their entry: header-stage errors and dstSize_tooSmall are found by the walk (such an entry emits no frames), later
// ones are filed per block (report_error, kStBlockKeysLo) and folded per entry.  The host synchronises as often as for one single
// call.  An entry that holds a frame without a content size (where its output goes is known only after decoding: frame_rescan is
// global by construction) or more than kBatchAloneAbove compressed bytes (one lane walks an entry's block headers) is decoded alone
// afterwards by decompress_device, and counted.  Under ZSTDMI_DCtx_setBatchUnsized the former take the shared pass too: an entry's
// first frame starts at its destination whatever its header says, and batch_rescan_kernel places the others per entry from the
// regenerated sizes block_offsets has computed before a byte of output is written.
constexpr u64 kBatchAloneAbove = (u64)4 << 20;
// the batch's core over a device-resident entry table (d->batchIn, n entries; d->batchOut gets what the walk and the decoder make of
// them): batch_walk_count -> batch_scan -> batch_walk_emit -> decode_lists -> batch_fold.  `readBack` enqueues the caller's copy of
// whatever it wants of d->batchOut: called in front of each of the two host synchronisations that see final entries (after the
// count: entries without frames are final; after the fold: all are).  -> 0, or the error of the whole run.
static size_t decode_entries(ZSTD_DCtx* d, const DecodeDict& dd, const u8* srcBase, u8* dstBase, size_t dstSpan, u32 n, const std::function<bool()>& readBack)
{
    hipStream_t s = d->stream;
    if (!d->status.ensure(kStWords * sizeof(u32))) return ZERR(kErrMemoryAllocation);
    u32* status = (u32*)d->status.p;
    const BatchEntryIn* dIn = (const BatchEntryIn*)d->batchIn.p; BatchEntryOut* dOut = (BatchEntryOut*)d->batchOut.p;
    u32 st[kStWords] = {};
    { const size_t e = status_reset(d); if (isErr(e)) return e; }
    d->lastBatchWs = 0;
    launch_batch_walk_count(srcBase, dIn, dOut, n, dd, kBatchAloneAbove, status, s, d->batchUnsized != 0);
    if (!readBack() ||
        hipMemcpyAsync(st, status, sizeof st, hipMemcpyDeviceToHost, s) != hipSuccess) return ZERR(kErrGeneric);
    { const size_t e = stream_wait(s); if (isErr(e)) return e; }
    if (st[kStErr]) return ZERR(st[kStErr]);
    if (dd.slots) d->lastSetFrames += st[kStSetFrames];
    const u32 nFrames = st[kStFrames], nBlocks = st[kStBlocks];
    const u64 total = st_u64(st, kStTotalLo, kStTotalHi);
    // entries with unsized frames in the lists (ZSTDMI_DCtx_setBatchUnsized; none: the pass is the one it always was): `total` holds
    // their clamped literal rooms, the dump area lies behind the frames' scratch, and the open instances find both through the status words
    const bool open = st[kStOpenEntries] != 0;
    const ListsLayout l = lists_layout(nFrames, nBlocks, total, open);
    const OpenEntries openEntries = { dIn, dOut, n };
    u32 keyWords[2] = {0, 0}, openWords[4] = {0, 0, 0, 0};      // (sources of asynchronous copies: they live until decode_lists has synchronised)
    if (nFrames) {
        if (!ensure_lists(d, l) || !d->blockKeys.ensure(l.blockKeys)) return ZERR(kErrMemoryAllocation);
        d->lastBatchWs += (long long)(l.frames + l.blocks + l.scratch + l.slowFlags + l.blockKeys);
        if (open) {
            if (!d->litRooms.ensure(l.litRooms)) return ZERR(kErrMemoryAllocation);
            d->lastBatchWs += (long long)l.litRooms;
            const u64 rooms = (u64)(uintptr_t)d->litRooms.p;
            openWords[0] = (u32)rooms; openWords[1] = (u32)(rooms >> 32); openWords[2] = (u32)l.dumpOff; openWords[3] = (u32)(l.dumpOff >> 32);
            static_assert(kStRoomHi == kStRoomLo + 1 && kStDumpLo == kStRoomLo + 2 && kStDumpHi == kStRoomLo + 3, "one copy fills the four words");
            if (hipMemcpyAsync(status + kStRoomLo, openWords, sizeof openWords, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        }
        keyWords[0] = (u32)(uintptr_t)d->blockKeys.p; keyWords[1] = (u32)((u64)(uintptr_t)d->blockKeys.p >> 32);
        if (hipMemsetAsync(d->blockKeys.p, 0xFF, (size_t)nBlocks * sizeof(u64), s) != hipSuccess ||
            hipMemcpyAsync(status + kStBlockKeysLo, &keyWords[0], sizeof(u32), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(status + kStBlockKeysHi, &keyWords[1], sizeof(u32), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        launch_batch_walk_emit(srcBase, dIn, dOut, n, (FrameDesc*)d->frames.p, (BlockDesc*)d->blocks.p, s, dd, open ? (u64*)d->litRooms.p : nullptr);
        d->timer.mark("batch_walk", s);
        const size_t e = decode_lists(d, dd, dstBase, srcBase, nFrames, nBlocks, 0, dstSpan, st, [&]() -> bool {
            launch_batch_fold(dOut, n, (const u64*)d->blockKeys.p, s);
            return readBack();
        }, nullptr, open ? &openEntries : nullptr);
        if (isErr(e)) return e;
        d->lastBatchWs += (long long)((st_u64(st, kStSeqLo, kStSeqHi) + 64) * sizeof(SeqRec));      // (what decode_lists asked d->recs for)
    }
    return 0;
}

static size_t decompress_batch_impl(ZSTD_DCtx* d, const void* const* srcs, const size_t* srcSizes, size_t n, void* const* dsts, const size_t* dstCapacities, size_t* dstSizes)
{
    if (!d) return ZERR(kErrGeneric);
    if (n == 0) { d->lastBatchAlone = 0; d->lastBatchWs = 0; return 0; }
    if (!srcs || !srcSizes || !dsts || !dstCapacities || !dstSizes) return ZERR(kErrGeneric);
    if (n > 0xFFFFFFF0ull) return ZERR(kErrMemoryAllocation);
    size_t e = dctx_bind(d); if (isErr(e)) return e;
    if (d->workers.size() > 1 || d->pfx) return ZERR(kErrParameterUnsupported);      // (a pending ZSTD_DCtx_refPrefix serves one single call)
    e = set_check(d); if (isErr(e)) return e;
    d->lastBatchAlone = 0; d->lastBatchWs = 0;
    hipStream_t s = d->stream;
    DecodeDict dd;
    e = call_dict(d, dd); if (isErr(e)) return e;
    // one base pointer each: the lowest source, the lowest destination
    uintptr_t loS = ~(uintptr_t)0, loD = ~(uintptr_t)0, hiD = 0;
    for (size_t i = 0; i < n; i++) {
        if (srcSizes[i] && srcs[i] && (uintptr_t)srcs[i] < loS) loS = (uintptr_t)srcs[i];
        if (dsts[i]) { const uintptr_t p = (uintptr_t)dsts[i]; if (p < loD) loD = p; if (p + dstCapacities[i] > hiD) hiD = p + dstCapacities[i]; }
    }
    if (loS == ~(uintptr_t)0) loS = 0;
    if (loD == ~(uintptr_t)0) loD = 0;
    std::vector<BatchEntryIn> hIn(n);
    for (size_t i = 0; i < n; i++) {
        const bool noSrc = srcSizes[i] && !srcs[i];           // (the single call: srcSize_wrong, below)
        hIn[i].srcOff = (srcSizes[i] && !noSrc) ? (u64)((uintptr_t)srcs[i] - loS) : 0;
        hIn[i].srcSize = noSrc ? 0 : (u64)srcSizes[i];
        hIn[i].dstOff = dsts[i] ? (u64)((uintptr_t)dsts[i] - loD) : 0;
        hIn[i].dstCap = dsts[i] ? (u64)dstCapacities[i] : 0;
    }
    if (!d->batchIn.ensure(n * sizeof(BatchEntryIn)) || !d->batchOut.ensure(n * sizeof(BatchEntryOut))) return ZERR(kErrMemoryAllocation);
    BatchEntryOut* dOut = (BatchEntryOut*)d->batchOut.p;
    std::vector<BatchEntryOut> hOut(n);
    d->timer.begin(s);
    if (hipMemcpyAsync(d->batchIn.p, hIn.data(), n * sizeof(BatchEntryIn), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
    e = decode_entries(d, dd, (const u8*)loS, (u8*)loD, (size_t)(hiD - loD), (u32)n, [&]() -> bool {
        return hipMemcpyAsync(hOut.data(), dOut, n * sizeof(BatchEntryOut), hipMemcpyDeviceToHost, s) == hipSuccess;
    });
    if (isErr(e)) return e;
    d->timer.finish();
    for (size_t i = 0; i < n; i++) {
        if (srcSizes[i] && !srcs[i]) { dstSizes[i] = ZERR(kErrSrcSizeWrong); continue; }
        if (hOut[i].state != kBatchAlone) dstSizes[i] = (size_t)hOut[i].result;
    }
    for (size_t i = 0; i < n; i++) {
        if ((srcSizes[i] && !srcs[i]) || hOut[i].state != kBatchAlone) continue;
        dstSizes[i] = decompress_device(d, (u8*)dsts[i], dstCapacities[i], (const u8*)srcs[i], srcSizes[i], false);
        d->lastBatchAlone++;
    }
    return 0;
}

// ---- a batch enqueued from the device (ZSTDMI_DCtx_prepareBatchAsync / ZSTDMI_decompressBatchAsync) ----
// decode_entries stops the host three times — to size the lists, to size the records, to read the answers — and copies a handful of
// words to the device in between.  Here the caller states limits once, the prepare sizes every work buffer from them, and a call is
// kernels only: the plan kernel reads the caller's arrays, the init kernel fills the status words, the scans hold the entries and the
// blocks to the limits (batch_scan_kernel<true>, seq_scan_kernel<true>), every stage takes its count from the status words over a
// grid sized from the limit, and the finish kernel writes the caller's sizes column.
// The limits rule of both prepares: content, and frames (framesDefault: what 0 stands for), blocks and sequences with their defaults
// filled in -> false: no content, or a limit beyond the lists' index range
static bool dcore_limits(u64 maxFrames, u64 maxBlocks, u64 maxSequences, u64 maxContent, u64 framesDefault, BatchLimitsD& lim)
{
    const u64 frames = maxFrames ? maxFrames : framesDefault;
    if (!maxContent || maxContent > ((u64)1 << 48) || frames > ((u64)1 << 26)) return false;
    const u64 blocks = maxBlocks ? maxBlocks : frames + maxContent / 16384, seqs = maxSequences ? maxSequences : maxContent / 3 + 64;
    if (blocks > 0xFFFFFFF0ull || seqs > ((u64)1 << 48)) return false;
    lim.frames = (u32)frames; lim.blocks = (u32)blocks; lim.content = maxContent; lim.sequences = seqs;
    return true;
}
// the batch's own: entries and the bound of one entry's compressed bytes -> false: a zero where none is allowed, or the rule above
static bool dbatch_limits(const ZSTDMI_DBatchLimits* L, size_t& maxEntries, u64& bound, BatchLimitsD& lim)
{
    if (!L->maxEntries || L->maxEntries > 0xFFFFFFF0ull || !L->srcSizeBound || L->srcSizeBound > kBatchAloneAbove) return false;
    maxEntries = L->maxEntries; bound = L->srcSizeBound;
    return dcore_limits(L->maxFrames, L->maxBlocks, L->maxSequences, L->maxContent, L->maxEntries, lim);
}
// One table of the work buffers of an enqueued call at the limits, in the order a prepare asks for them: a prepare ensures its entries, a
// workspace entry point sums them.  dcore_needs: the decode core's, over `rows` table rows, outRows answers and verdictRows verdicts.
struct BufNeeds {
    struct { DevBuf ZSTD_DCtx_s::* buf; size_t bytes; } e[16]; int n = 0;
    void add(DevBuf ZSTD_DCtx_s::* buf, size_t bytes) { e[n].buf = buf; e[n].bytes = bytes; n++; }
    size_t sum() const { size_t t = 0; for (int i = 0; i < n; ++i) t += e[i].bytes; return t; }
    bool ensure(ZSTD_DCtx* d, int from) const { for (int i = from; i < n; ++i) if (!(d->*e[i].buf).ensure(e[i].bytes)) return false; return true; }
};
static void dcore_needs(BufNeeds& t, size_t rows, size_t outRows, size_t verdictRows, const BatchLimitsD& lim)
{
    typedef ZSTD_DCtx_s D;
    const ListsLayout l = lists_layout(lim.frames, lim.blocks, lim.content, true);
    t.add(&D::batchIn, rows * sizeof(BatchEntryIn)); t.add(&D::batchOut, outRows * sizeof(BatchEntryOut)); t.add(&D::asyncVerdict, verdictRows * sizeof(u32));
    t.add(&D::frames, l.frames); t.add(&D::blocks, l.blocks); t.add(&D::scratch, l.scratch); t.add(&D::slowFlags, l.slowFlags);
    t.add(&D::blockKeys, l.blockKeys); t.add(&D::litRooms, l.litRooms);
    t.add(&D::recs, (size_t)(lim.sequences + 64) * sizeof(SeqRec)); t.add(&D::status, kStWords * sizeof(u32));
}
static BufNeeds dbatch_needs(size_t maxEntries, const BatchLimitsD& lim) { BufNeeds t; dcore_needs(t, maxEntries, maxEntries, maxEntries, lim); return t; }
// What both prepares do alike, in two steps (the ranges prepare reads the footer behind the bind and indexes the table in front of the core's
// buffers).  The first, behind a prepare's own limits: what the pass does not cover, as far as the host alone can tell (a pending prefix stays pending).
static size_t prepare_d_enter(ZSTD_DCtx* d)
{
    if (d->workers.size() > 1 || d->pfx || d->originMode == 2) return ZERR(kErrParameterUnsupported);
    const size_t e = set_check(d); if (isErr(e)) return e;
    return dctx_bind(d);
}
// the second: the table's buffers from entry `from` on, and the event behind an enqueued call
static size_t prepare_d_buffers(ZSTD_DCtx* d, const BufNeeds& needs, int from)
{
    if (!needs.ensure(d, from)) { (void)hipGetLastError(); return ZERR(kErrMemoryAllocation); }
    if (!d->asyncEv && hipEventCreateWithFlags(&d->asyncEv, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); d->asyncEv = nullptr; return ZERR(kErrMemoryAllocation); }
    return 0;
}
static size_t prepare_batch_async_d_impl(ZSTD_DCtx* d, const ZSTDMI_DBatchLimits* limits)
{
    if (!d || !limits) return ZERR(kErrGeneric);
    dctx_drop_prepares(d);
    size_t maxEntries; u64 bound; BatchLimitsD lim; DecodeDict dd;
    if (!dbatch_limits(limits, maxEntries, bound, lim)) return ZERR(kErrParameterOutOfBound);
    size_t e = prepare_d_enter(d); if (isErr(e)) return e;
    e = call_dict(d, dd); if (isErr(e)) return e;
    e = prepare_d_buffers(d, dbatch_needs(maxEntries, lim), 0); if (isErr(e)) return e;
    d->asyncPrep = new DAsyncPrep{ { dctx_gen(d), lim }, maxEntries, bound };
    return 0;
}
// this prepare still holds for the context as it stands: nothing dctx_gen() covers moved, and neither the dictionary nor the slot table waits for an upload
static bool prep_valid(const ZSTD_DCtx* d, const DPrepCore* P)
{
    return P && P->gen == dctx_gen(d) && d->deviceOk && !(d->dictDirty && !ddict_shared(d)) && !(set_active(d) && d->slotGen != d->setGen);
}
// an enqueued call's stage timer: off for the length of the call (stage events belong to calls that wait for them)
struct TimerOff { StageTimer& t; const bool was; explicit TimerOff(StageTimer& timer) : t(timer), was(timer.enabled) { t.enabled = false; } ~TimerOff() { t.enabled = was; } };
// The decode core of an enqueued call, shared by ZSTDMI_decompressBatchAsync and ZSTDMI_decompressRangesAsync: decode_entries between
// its table upload and its read-back, kernels only (and one hipMemsetAsync over the block keys), over nE rows of d->batchIn whose
// sources and destinations are offsets from kAsyncBase.  `plan` enqueues whatever fills those rows (-> false: failed); it runs behind
// the init kernel, where the batch's plan kernel has always run.  Behind the core, d->batchOut holds every row's answer.
static size_t decode_core_d(ZSTD_DCtx* d, const DecodeDict& dd, const BatchLimitsD& lim, u32 nE, const std::function<bool()>& plan)
{
    hipStream_t s = d->stream;
    const u64 dumpOff = lists_layout(lim.frames, lim.blocks, lim.content, true).dumpOff;
    BatchEntryIn* const dIn = (BatchEntryIn*)d->batchIn.p; BatchEntryOut* const dOut = (BatchEntryOut*)d->batchOut.p;
    FrameDesc* const frames = (FrameDesc*)d->frames.p; BlockDesc* const blocks = (BlockDesc*)d->blocks.p; SeqRec* const recs = (SeqRec*)d->recs.p;
    u32* const status = (u32*)d->status.p; u64* const keys = (u64*)d->blockKeys.p; u64* const rooms = (u64*)d->litRooms.p;
    u8* const scratch = (u8*)d->scratch.p; u8* const slowFlags = (u8*)d->slowFlags.p;
    // the bases are constants: the plan states every source and destination as an offset from kAsyncBase
    const u8* const srcBase = (const u8*)(uintptr_t)kAsyncBase; u8* const dstBase = (u8*)(uintptr_t)kAsyncBase;
    launch_batch_init_d(status, keys, rooms, dumpOff, lim, s);
    if (!plan()) { (void)hipGetLastError(); return ZERR(kErrGeneric); }
    if (hipMemsetAsync(keys, 0xFF, (size_t)lim.blocks * sizeof(u64), s) != hipSuccess) { (void)hipGetLastError(); return ZERR(kErrGeneric); }
    // (frames without a content size always take the shared pass: there is no single-call path to hand them to)
    launch_batch_walk_count(srcBase, dIn, dOut, nE, dd, kBatchAloneAbove, status, s, true, true);
    launch_batch_walk_emit(srcBase, dIn, dOut, nE, frames, blocks, s, dd, rooms);
    launch_block_prepass_d(srcBase, frames, blocks, lim.frames, lim.blocks, dd, status, s);
    launch_seq_decode_d(srcBase, frames, blocks, lim.blocks, recs, status, dd, s);
    launch_block_offsets_d(frames, blocks, lim.frames, dd, status, s);
    launch_batch_rescan(dIn, dOut, nE, frames, s);
    launch_decode_literals_d(srcBase, dstBase, scratch, frames, blocks, lim.blocks, status, slowFlags, d->litDecoder, dd, s);
    launch_place_literals_d(srcBase, dstBase, scratch, frames, blocks, lim.blocks, recs, status, s);
    // (every long frame takes the ordered walk; its waves per frame by the setter, else by the limit for the frames)
    launch_exec_matches_d(srcBase, dstBase, frames, blocks, lim.frames, recs, status, dd, s, exec_waves_for(d, lim.frames));
    launch_batch_fold(dOut, nE, keys, s);
    return 0;
}
// the event behind an enqueued call (without the event nothing may stay in flight)
static size_t dctx_async_record(ZSTD_DCtx* d)
{
    if (hipEventRecord(d->asyncEv, d->stream) != hipSuccess) {
        (void)hipGetLastError();
        return stream_wait(d->stream);
    }
    d->asyncPending = true;
    return 0;
}
static size_t decompress_batch_async_impl(ZSTD_DCtx* d, const void* const* d_srcs, const size_t* d_srcSizes, size_t n, void* const* d_dsts,
                                          const size_t* d_dstCapacities, size_t* d_dstSizes)
{
    if (!d) return ZERR(kErrGeneric);
    if (n == 0) return 0;
    if (!d_srcs || !d_srcSizes || !d_dsts || !d_dstCapacities || !d_dstSizes) return ZERR(kErrGeneric);
    const DAsyncPrep* const P = d->asyncPrep;
    if (!prep_valid(d, P) || n > P->maxEntries) return ZERR(kErrStageWrong);
    size_t e = dctx_bind(d); if (isErr(e)) return e;
    const TimerOff timerOff(d->timer);
    hipStream_t s = d->stream;
    DecodeDict dd;
    e = call_dict(d, dd); if (isErr(e)) return e;       // (prep_valid: the dictionary and the table are current, nothing is uploaded)
    const u32 nE = (u32)n;
    u32* const verdict = (u32*)d->asyncVerdict.p;
    e = decode_core_d(d, dd, P->lim, nE, [&]() -> bool {
        launch_batch_plan_d(d_srcs, d_srcSizes, d_dsts, d_dstCapacities, nE, P->bound, (BatchEntryIn*)d->batchIn.p, verdict, s);
        return true;
    });
    if (isErr(e)) return e;
    launch_batch_finish_d((const BatchEntryOut*)d->batchOut.p, verdict, nE, d_dstSizes, s);
    return dctx_async_record(d);
}

// ---- a byte range of a seekable stream (ZSTDMI_decompressRange) ----
// The stream ends in a seek table (include/zstd_mi355x.h): one (compressed size, content size) pair per frame.  The host reads the
// 9-byte footer (how long the table is); seek_select_kernel checks the rest of it and finds the entries whose content meets
// [offset, offset + length) — one read-back of its summary words —; seek_emit_kernel turns those entries into the batch walk's table on
// the device, and the batch's core (decode_entries) decodes them in one run: frames wholly inside the range straight to their place in
// dst, the at most two frames the range cuts into an edge buffer, from which range_clip_kernel copies the wanted part.  An entry the
// walk leaves to the single-call path (a frame without a content size, more than kBatchAloneAbove compressed bytes) is decoded by
// decompress_device into the same place.  range_check_kernel holds every entry to the content size its table entry names.  A host
// source is staged in two pieces only: the table, and the compressed bytes of the selected entries.
// a stream's seek table as the kernels read it: n entries of `stride` bytes in tableBytes bytes at tab (device memory: in a device
// source where it lies, a host source's copy in d->seekTab)
struct SeekTable { const u8* tab; u32 n, stride; u64 tableBytes; bool srcDev; };
// the 9-byte footer of the stream's seek table, read on the host (a device source: one small copy back) -> the entry count, the
// entries' stride and the table's length, or the table's error
static size_t read_seek_footer(ZSTD_DCtx* d, const void* src, size_t srcSize, bool srcDev, u32& N, u32& stride, u64& tableBytes)
{
    if (srcSize && !src) return ZERR(kErrSrcSizeWrong);
    if (srcSize < 17) return ZERR(kErrPrefixUnknown);
    hipStream_t s = d->stream;
    auto rd32 = [](const u8* p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); };
    u8 foot[9];
    if (srcDev) {
        const size_t e = dev_read(foot, (const u8*)src + srcSize - 9, 9, s); if (isErr(e)) return e;
    } else memcpy(foot, (const u8*)src + srcSize - 9, 9);
    if (rd32(foot + 5) != 0x8F92EAB1u) return ZERR(kErrPrefixUnknown);
    if (foot[4] & 0x7C) return ZERR(kErrCorruption);                    // reserved descriptor bits
    N = rd32(foot);
    if (N > (1u << 27)) return ZERR(kErrCorruption);
    stride = (foot[4] & 0x80) ? 12u : 8u;                               // (checksums, where the table has them, are skipped)
    tableBytes = 17 + (u64)N * stride;
    if (tableBytes > srcSize) return ZERR(kErrCorruption);
    return 0;
}
// what a call on a seekable stream begins with: the footer first, then the dictionary, a host source's table staged (its bytes counted
// in *staged), and the call's DecodeDict with the slot table behind it
static size_t open_seek_table(ZSTD_DCtx* d, const void* src, size_t srcSize, SeekTable* t, long long* staged, DecodeDict& dd)
{
    t->srcDev = is_device_ptr(src);
    size_t e = read_seek_footer(d, src, srcSize, t->srcDev, t->n, t->stride, t->tableBytes); if (isErr(e)) return e;
    e = dctx_sync_dictionary(d); if (isErr(e)) return e;
    t->tab = (const u8*)src + (srcSize - t->tableBytes);
    if (!t->srcDev) {
        if (!d->seekTab.ensure((size_t)t->tableBytes + 64)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(d->seekTab.p, t->tab, (size_t)t->tableBytes, hipMemcpyHostToDevice, d->stream) != hipSuccess) return ZERR(kErrGeneric);
        t->tab = (const u8*)d->seekTab.p; *staged += (long long)t->tableBytes;
    }
    dd = decode_dict(d);
    return dctx_sync_slots(d, dd);
}
// what a range returns of a stream of `total` bytes of content when nothing fails
static u64 range_returned(u64 offset, u64 length, u64 total) { return offset < total ? (length < total - offset ? length : total - offset) : 0; }
// the entry tables of the last decode_entries run, brought to the host (rare: only when an entry was left to the single-call path)
static size_t fetch_entries(ZSTD_DCtx* d, u32 n, std::vector<BatchEntryIn>& hIn, std::vector<BatchEntryOut>& hOut)
{
    hIn.resize(n); hOut.resize(n);
    if (hipMemcpyAsync(hIn.data(), d->batchIn.p, (size_t)n * sizeof(BatchEntryIn), hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
        hipMemcpyAsync(hOut.data(), d->batchOut.p, (size_t)n * sizeof(BatchEntryOut), hipMemcpyDeviceToHost, d->stream) != hipSuccess) return ZERR(kErrGeneric);
    return stream_wait(d->stream);
}

static size_t decompress_range_impl(ZSTD_DCtx* d, void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned long long offset, size_t length)
{
    size_t e = dctx_bind(d); if (isErr(e)) return e;
    if (d->workers.size() > 1 || d->pfx) return ZERR(kErrParameterUnsupported);
    e = set_check(d); if (isErr(e)) return e;
    d->lastRangeFrames = 0; d->lastRangeStaged = 0; d->lastBatchWs = 0;
    hipStream_t s = d->stream;
    const bool dstDev = dst ? is_device_ptr(dst) : false;
    SeekTable t; DecodeDict dd;
    e = open_seek_table(d, src, srcSize, &t, &d->lastRangeStaged, dd); if (isErr(e)) return e;
    const bool srcDev = t.srcDev;
    if (!d->seekSum.ensure(kSeekWords * sizeof(u64))) return ZERR(kErrMemoryAllocation);
    u64* const sum = (u64*)d->seekSum.p;
    d->timer.begin(s);
    launch_seek_select(t.tab, t.tableBytes, t.n, t.stride, srcSize, offset, length, sum, s);
    u64 sm[kSeekWords] = {};
    e = dev_read(sm, sum, sizeof sm, s); if (isErr(e)) return e;
    d->timer.mark("seek_select", s);
    if (sm[kSeekErr]) return ZERR((u32)sm[kSeekErr]);
    const u64 returned = range_returned(offset, length, sm[kSeekTotal]);
    if (returned > dstCapacity) return ZERR(kErrDstSizeTooSmall);
    if (!returned) { d->timer.finish(); return 0; }
    if (!dst) return ZERR(kErrDstBufferNull);
    const u64 nMeet = sm[kSeekMeet];
    if (!nMeet || sm[kSeekLast] < sm[kSeekFirst]) return ZERR(kErrCorruption);
    const u32 first = (u32)sm[kSeekFirst], last = (u32)sm[kSeekLast], nSel = last - first + 1;
    const u64 cLo = sm[kSeekCLo], cHi = sm[kSeekCHi], end = offset + returned;
    const u64 dFirst = sm[kSeekDFirst], sizeFirst = sm[kSeekSizeFirst], dLast = sm[kSeekDLast], sizeLast = sm[kSeekSizeLast];
    const bool cutFirst = dFirst < offset || dFirst + sizeFirst > end, cutLast = last != first && dLast + sizeLast > end;
    const u64 slot1 = cutFirst ? ((sizeFirst + 255) & ~(u64)255) : 0, edgeBytes = slot1 + (cutLast ? sizeLast : 0);
    if (edgeBytes && !d->edge.ensure((size_t)edgeBytes + 64)) return ZERR(kErrMemoryAllocation);
    const u8* srcBase = (const u8*)src + cLo;
    if (!srcDev) {              // only the selected frames travel
        if (!d->stageSrc.ensure((size_t)(cHi - cLo) + 64)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(d->stageSrc.p, (const u8*)src + cLo, (size_t)(cHi - cLo), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        srcBase = (const u8*)d->stageSrc.p; d->lastRangeStaged += (long long)(cHi - cLo);
    }
    u8* d_dst = (u8*)dst;
    if (!dstDev) { if (!d->stageDst.ensure((size_t)returned + 64)) return ZERR(kErrMemoryAllocation); d_dst = (u8*)d->stageDst.p; }
    // one base pointer for the destinations, the lowest: dst or the edge buffer
    const uintptr_t pD = (uintptr_t)d_dst, pE = edgeBytes ? (uintptr_t)d->edge.p : pD;
    const uintptr_t lo = pD < pE ? pD : pE, hi = (pD + returned > pE + edgeBytes) ? pD + (uintptr_t)returned : pE + (uintptr_t)edgeBytes;
    if (!d->batchIn.ensure((size_t)nSel * sizeof(BatchEntryIn)) || !d->batchOut.ensure((size_t)nSel * sizeof(BatchEntryOut))) return ZERR(kErrMemoryAllocation);
    launch_seek_emit(t.tab, t.stride, first, nSel, dFirst, offset, (u64)(pD - lo), (u64)(pE - lo), slot1, cutFirst ? 1u : 0u, cutLast ? 1u : 0u, (BatchEntryIn*)d->batchIn.p, s);
    d->timer.mark("seek_emit", s);
    e = decode_entries(d, dd, srcBase, (u8*)lo, (size_t)(hi - lo), nSel, [] { return true; });
    if (isErr(e)) return e;
    launch_range_check((const BatchEntryIn*)d->batchIn.p, (const BatchEntryOut*)d->batchOut.p, nSel, sum, s);
    e = dev_read(sm, sum, sizeof sm, s); if (isErr(e)) return e;
    if (sm[kSeekKey] != ~0ull) return ZERR((u32)(sm[kSeekKey] & 0xFFFFu));
    if (sm[kSeekAlone]) {       // (rare: the entries come to the host only then)
        std::vector<BatchEntryIn> hIn; std::vector<BatchEntryOut> hOut;
        e = fetch_entries(d, nSel, hIn, hOut); if (isErr(e)) return e;
        for (u32 i = 0; i < nSel; ++i) {
            if (hOut[i].state != kBatchAlone) continue;
            const size_t r = decompress_device(d, (u8*)lo + hIn[i].dstOff, (size_t)hIn[i].dstCap, srcBase + hIn[i].srcOff, (size_t)hIn[i].srcSize, false);
            if (isErr(r)) return r == ZERR(kErrDstSizeTooSmall) ? ZERR(kErrCorruption) : r;
            if (r != hIn[i].dstCap) return ZERR(kErrCorruption);
        }
    }
    if (edgeBytes) {
        ClipJob j0 = {0, 0, 0}, j1 = {0, 0, 0};
        if (cutFirst) { const u64 from = offset > dFirst ? offset - dFirst : 0, stop = dFirst + sizeFirst < end ? dFirst + sizeFirst : end;
                        j0.from = from; j0.to = dFirst + from - offset; j0.len = stop - (dFirst + from); }
        if (cutLast) { j1.from = slot1; j1.to = dLast - offset; j1.len = end - dLast; }
        launch_range_clip(d_dst, (const u8*)d->edge.p, j0, j1, s);
        d->timer.mark("range_clip", s);
    }
    if (!dstDev && hipMemcpyAsync(dst, d_dst, (size_t)returned, hipMemcpyDeviceToHost, s) != hipSuccess) return ZERR(kErrGeneric);
    e = stream_wait(s); if (isErr(e)) return e;
    d->timer.finish();
    d->lastRangeFrames = (int)nMeet;
    return (size_t)returned;
}


// ---- many ranges of a seekable stream in one call (ZSTDMI_decompressRanges) ----
// While one of these lives, the context's stage timer is off and keeps what it has recorded: the single-call paths that the pass hands
// a frame or a range to begin the timer anew, and ZSTDMI_DCtx_getStageTimes is to show the pass.
struct TimerPause {
    StageTimer& t; const bool was; const int n;
    explicit TimerPause(StageTimer& timer) : t(timer), was(timer.enabled), n(timer.n) { t.enabled = false; }
    ~TimerPause() { t.enabled = was; t.n = n; }
};
// seek_index turns the table into prefix arrays once; ranges_select answers every range that needs no decoding and marks the entries
// the others meet; ranges_plan makes ONE decode table of the touched entries — each decoded once, into its slot of the context's
// arena, whatever number of ranges meets it — and decode_entries runs over it as over any batch.  An entry the walk leaves to the
// single-call path is decoded by decompress_device into its slot; ranges_gather then checks each range's entries and copies its
// bytes.  From a host source the table and the touched entries' compressed bytes travel, packed into one staging buffer.  A range of
// more than kRangesAloneAbove bytes is handed to decompress_range_impl afterwards: it wants its frames decoded in place.
static size_t decompress_ranges_impl(ZSTD_DCtx* d, const void* src, size_t srcSize, const unsigned long long* offsets, const size_t* lengths, size_t n,
                                     void* const* dsts, const size_t* dstCapacities, size_t* dstSizes)
{
    if (!d) return ZERR(kErrGeneric);
    if (n == 0) { d->lastRangesFrames = 0; d->lastRangesAlone = 0; d->lastRangesStaged = 0; return 0; }
    if (!offsets || !lengths || !dsts || !dstCapacities || !dstSizes) return ZERR(kErrGeneric);
    if (n > 0xFFFFFFF0ull) return ZERR(kErrMemoryAllocation);
    size_t e = dctx_bind(d); if (isErr(e)) return e;
    if (d->workers.size() > 1 || d->pfx) return ZERR(kErrParameterUnsupported);      // (a pending ZSTD_DCtx_refPrefix serves one single call)
    e = set_check(d); if (isErr(e)) return e;
    d->lastRangesFrames = 0; d->lastRangesAlone = 0; d->lastRangesStaged = 0; d->lastBatchWs = 0;
    hipStream_t s = d->stream;
    SeekTable t; DecodeDict dd;
    e = open_seek_table(d, src, srcSize, &t, &d->lastRangesStaged, dd); if (isErr(e)) return e;
    const bool srcDev = t.srcDev; const u32 N = t.n;
    const u32 nR = (u32)n;
    if (!d->rangesWs.ensure(ranges_ws_bytes(N)) || !d->batchIn.ensure((size_t)N * sizeof(BatchEntryIn) + 64) ||
        !d->rangesIn.ensure(n * sizeof(RangeIn)) || !d->rangesRec.ensure(n * sizeof(RangeRec)) || !d->rangesRes.ensure(n * sizeof(u64))) return ZERR(kErrMemoryAllocation);
    const RangesWs ws = ranges_ws((u8*)d->rangesWs.p, N);
    std::vector<RangeIn> hIn(n);
    for (size_t i = 0; i < n; i++) { hIn[i].offset = offsets[i]; hIn[i].length = lengths[i]; hIn[i].dstCap = dstCapacities[i]; hIn[i].dst = (u64)(uintptr_t)dsts[i]; }
    if (hipMemcpyAsync(d->rangesIn.p, hIn.data(), n * sizeof(RangeIn), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
    const RangeIn* dRanges = (const RangeIn*)d->rangesIn.p; RangeRec* dRecs = (RangeRec*)d->rangesRec.p;
    d->timer.begin(s);
    launch_seek_index(t.tab, t.tableBytes, N, t.stride, srcSize, ws, s);                               d->timer.mark("seek_index", s);
    launch_ranges_select(dRanges, dRecs, nR, N, ws, s);                                                d->timer.mark("ranges_select", s);
    launch_ranges_plan(t.tab, N, t.stride, srcDev ? 1u : 0u, ws, (BatchEntryIn*)d->batchIn.p, s);          d->timer.mark("ranges_plan", s);
    u64 sm[kRgWords] = {};
    e = dev_read(sm, ws.sum, sizeof sm, s); if (isErr(e)) return e;
    if (sm[kRgErr]) { d->timer.finish(); return ZERR((u32)sm[kRgErr]); }
    const u64 total = sm[kRgTotal], arenaBytes = sm[kRgArena], packedBytes = sm[kRgCompact], nRuns = sm[kRgRuns];
    const u32 nTouched = (u32)sm[kRgTouched];
    std::vector<u8> packed;     // (these four are sources of asynchronous copies: they live until the last synchronisation below)
    std::vector<u64> runs;
    std::vector<BatchEntryIn> eIn; std::vector<BatchEntryOut> eOut;
    if (nTouched) {
        if (!d->arena.ensure((size_t)arenaBytes + 64) || !d->batchOut.ensure((size_t)nTouched * sizeof(BatchEntryOut))) return ZERR(kErrMemoryAllocation);
        const u8* srcBase = (const u8*)src;
        if (!srcDev) {          // only the touched frames travel, in one copy
            runs.resize(2 * (size_t)nRuns); packed.resize((size_t)packedBytes);
            e = dev_read(runs.data(), ws.runs, runs.size() * sizeof(u64), s); if (isErr(e)) return e;
            if (pack_runs(runs.data(), (size_t)nRuns, (const u8*)src, srcSize, packed.data(), packed.size()) != packed.size()) return ZERR(kErrGeneric);
            if (!d->stageSrc.ensure(packed.size() + 64)) return ZERR(kErrMemoryAllocation);
            if (hipMemcpyAsync(d->stageSrc.p, packed.data(), packed.size(), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
            srcBase = (const u8*)d->stageSrc.p; d->lastRangesStaged += (long long)packed.size();
        }
        u64 someAlone = 0;
        e = decode_entries(d, dd, srcBase, (u8*)d->arena.p, (size_t)arenaBytes, nTouched, [&]() -> bool {
            launch_ranges_alone((const BatchEntryOut*)d->batchOut.p, nTouched, ws, s);
            return hipMemcpyAsync(&someAlone, ws.sum + kRgAloneEntries, sizeof(u64), hipMemcpyDeviceToHost, s) == hipSuccess;
        });
        if (isErr(e)) return e;
        if (someAlone) {        // (rare: the entries come to the host only then)
            e = fetch_entries(d, nTouched, eIn, eOut); if (isErr(e)) return e;
            const TimerPause pause(d->timer);       // (decompress_device times itself: the pass keeps its own stages)
            for (u32 i = 0; i < nTouched; ++i) {
                if (eOut[i].state != kBatchAlone) continue;
                eOut[i].result = (u64)decompress_device(d, (u8*)d->arena.p + eIn[i].dstOff, (size_t)eIn[i].dstCap, srcBase + eIn[i].srcOff, (size_t)eIn[i].srcSize, false);
                if (hipMemcpyAsync((BatchEntryOut*)d->batchOut.p + i, &eOut[i], sizeof(BatchEntryOut), hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
            }
        }
    }
    std::vector<u64> hRes(n);
    // (what a range returns: ranges_select's rule, on the host: it has the total now)
    u64 longest = 0;            // of the ranges the gather serves: the number of its slices
    for (size_t i = 0; i < n; i++) {
        const u64 ret = range_returned(offsets[i], lengths[i], total);
        if (ret <= dstCapacities[i] && ret <= kRangesAloneAbove && dsts[i] && ret > longest) longest = ret;
    }
    launch_ranges_gather(dRanges, dRecs, (u64*)d->rangesRes.p, nR, (u32)((longest + kGatherSlice - 1) / kGatherSlice), ws, (const BatchEntryOut*)d->batchOut.p,
                         (const u8*)d->arena.p, s);
    d->timer.mark("ranges_gather", s);
    e = dev_read(hRes.data(), d->rangesRes.p, n * sizeof(u64), s); if (isErr(e)) return e;
    d->timer.finish();
    d->lastRangesFrames = (int)nTouched;
    // the ranges that go alone, in range order
    const long long staged = d->lastRangesStaged; long long stagedAlone = 0; int alone = 0;
    const TimerPause pause(d->timer);               // (the stage times stay the gathered pass's)
    for (size_t i = 0; i < n; i++) {
        const u64 ret = range_returned(offsets[i], lengths[i], total);
        if (ret > dstCapacities[i] || !dsts[i] || ret <= kRangesAloneAbove) { dstSizes[i] = (size_t)hRes[i]; continue; }
        dstSizes[i] = decompress_range_impl(d, dsts[i], dstCapacities[i], src, srcSize, offsets[i], lengths[i]);
        stagedAlone += d->lastRangeStaged; alone++;
    }
    d->lastRangesAlone = alone; d->lastRangesStaged = staged + stagedAlone;
    return 0;
}

// ---- gather reads enqueued from the device (ZSTDMI_DCtx_prepareRangesAsync / ZSTDMI_decompressRangesAsync) ----
// decompress_ranges_impl stops the host for the footer, for the plan's summary (to size the arena) and for the answers, and indexes
// the table on every call.  Here the prepare reads the footer and runs seek_index once, into an index of its own, and sizes the arena
// and the decode core's buffers from the caller's limits; a call is the per-call reset of the marks, the select over the caller's
// device arrays, the plan over N entries (a host constant now), the decode core above over min(N, maxFrames) rows, and the gather over
// a grid sized from maxRangeBytes, which writes the caller's sizes column.
// the ranges' own limits for a table of tableEntries entries, and the rows of the decode core's table -> false: a zero where none is
// allowed, a range bound above what the gather serves, a table beyond the format's, or dcore_limits' rule
static bool dranges_limits(const ZSTDMI_DRangesLimits* L, u64 tableEntries, BatchLimitsD& lim, u32& nRows)
{
    if (!L->maxRanges || L->maxRanges > 0xFFFFFFF0ull || !L->maxRangeBytes || L->maxRangeBytes > kRangesAloneAbove || tableEntries > ((u64)1 << 27)) return false;
    // (an empty table: the core still runs, over one empty row)
    if (!dcore_limits(L->maxFrames, L->maxBlocks, L->maxSequences, L->maxContent, tableEntries ? tableEntries : 1, lim)) return false;
    nRows = !tableEntries ? 1u : (u32)(tableEntries < lim.frames ? tableEntries : lim.frames);
    return true;
}
// the buffers of a call at the limits: the index (first: seek_index runs into it before the others are asked for), the ranges' rows, the
// arena, and the decode core's with two verdict rows behind its table and no verdict column
static BufNeeds dranges_needs(size_t maxRanges, u32 tableEntries, u32 nRows, const BatchLimitsD& lim)
{
    typedef ZSTD_DCtx_s D;
    BufNeeds t;
    t.add(&D::rangesAsyncWs, ranges_ws_bytes(tableEntries)); t.add(&D::rangesIn, maxRanges * sizeof(RangeIn)); t.add(&D::rangesRec, maxRanges * sizeof(RangeRec));
    t.add(&D::arena, (size_t)lim.content + 64);
    dcore_needs(t, nRows, (size_t)nRows + 2, 0, lim);
    return t;
}
static size_t prepare_ranges_async_impl(ZSTD_DCtx* d, const void* d_src, size_t srcSize, const ZSTDMI_DRangesLimits* limits)
{
    if (!d || !limits) return ZERR(kErrGeneric);
    dctx_drop_prepares(d);
    BatchLimitsD lim; u32 nRows; DecodeDict dd;
    if (!dranges_limits(limits, 0, lim, nRows)) return ZERR(kErrParameterOutOfBound);
    size_t e = prepare_d_enter(d); if (isErr(e)) return e;
    if (d_src && !is_device_ptr(d_src)) return ZERR(kErrParameterUnsupported);
    hipStream_t s = d->stream;
    u32 N, stride; u64 tableBytes;
    e = read_seek_footer(d, d_src, srcSize, true, N, stride, tableBytes); if (isErr(e)) return e;
    e = call_dict(d, dd); if (isErr(e)) return e;
    if (!dranges_limits(limits, N, lim, nRows)) return ZERR(kErrParameterOutOfBound);      // (maxFrames 0 = N: known only now)
    const BufNeeds needs = dranges_needs(limits->maxRanges, N, nRows, lim);
    if (!d->rangesAsyncWs.ensure(needs.e[0].bytes)) { (void)hipGetLastError(); return ZERR(kErrMemoryAllocation); }
    const RangesWs ws = ranges_ws((u8*)d->rangesAsyncWs.p, N);
    const u8* const tab = (const u8*)d_src + (srcSize - tableBytes);
    launch_seek_index(tab, tableBytes, N, stride, srcSize, ws, s);
    u64 sm[kRgWords] = {};
    e = dev_read(sm, ws.sum, sizeof sm, s); if (isErr(e)) return e;
    if (sm[kRgErr]) return ZERR((u32)sm[kRgErr]);
    e = prepare_d_buffers(d, needs, 1); if (isErr(e)) return e;
    d->rangesPrep = new DRangesPrep{ { dctx_gen(d), lim }, limits->maxRanges, limits->maxRangeBytes, (const u8*)d_src, tab, N, stride, sm[kRgTotal], nRows };
    return 0;
}
static size_t decompress_ranges_async_impl(ZSTD_DCtx* d, const unsigned long long* d_offsets, const size_t* d_lengths, size_t n, void* const* d_dsts,
                                           const size_t* d_dstCapacities, size_t* d_dstSizes)
{
    if (!d) return ZERR(kErrGeneric);
    if (n == 0) return 0;
    if (!d_offsets || !d_lengths || !d_dsts || !d_dstCapacities || !d_dstSizes) return ZERR(kErrGeneric);
    const DRangesPrep* const P = d->rangesPrep;
    if (!prep_valid(d, P) || n > P->maxRanges) return ZERR(kErrStageWrong);
    size_t e = dctx_bind(d); if (isErr(e)) return e;
    const TimerOff timerOff(d->timer);
    hipStream_t s = d->stream;
    DecodeDict dd;
    e = call_dict(d, dd); if (isErr(e)) return e;       // (prep_valid: the dictionary and the table are current, nothing is uploaded)
    const u32 nR = (u32)n, N = P->n;
    const RangesWs ws = ranges_ws((u8*)d->rangesAsyncWs.p, N);
    RangeIn* const dRanges = (RangeIn*)d->rangesIn.p; RangeRec* const dRecs = (RangeRec*)d->rangesRec.p;
    e = decode_core_d(d, dd, P->lim, P->nRows, [&]() -> bool {
        // the index persists from the prepare, the marks and the plan's summary are this call's
        if (hipMemsetAsync(ws.diff, 0, ((size_t)N + 1) * sizeof(u32), s) != hipSuccess ||
            hipMemsetAsync(ws.sum + kRgTouched, 0, (kRgWords - kRgTouched) * sizeof(u64), s) != hipSuccess) return false;
        launch_ranges_select_d(d_offsets, d_lengths, d_dsts, d_dstCapacities, nR, P->maxRangeBytes, dRanges, dRecs, N, ws, s);
        launch_ranges_plan_d(P->tab, N, P->stride, ws, (u64)(uintptr_t)P->src - kAsyncBase, (u64)(uintptr_t)d->arena.p - kAsyncBase, P->lim.frames, P->lim.content,
                             kBatchAloneAbove, P->nRows, (BatchEntryIn*)d->batchIn.p, (BatchEntryOut*)d->batchOut.p, s);
        return true;
    });
    if (isErr(e)) return e;
    static_assert(sizeof(size_t) == sizeof(u64), "the gather writes the caller's sizes column");
    launch_ranges_gather(dRanges, dRecs, (u64*)d_dstSizes, nR, (u32)((P->maxRangeBytes + kGatherSlice - 1) / kGatherSlice), ws, (const BatchEntryOut*)d->batchOut.p,
                         (const u8*)d->arena.p, s);
    return dctx_async_record(d);
}

static size_t decompress_multi(ZSTD_DCtx* d, void* dst, size_t dstCapacity, const void* src, size_t srcSize);
// ZSTD_DCtx_refPrefix (U/ZstdDecompress.cs:2164-2202): the pending prefix becomes this call's raw-content dictionary — a device prefix
// where it lies, a host prefix staged to HBM — and is consumed, whatever the call returns (PrefixUse's destructor)
struct PrefixUse {
    ZSTD_DCtx* d;
    explicit PrefixUse(ZSTD_DCtx* dd) : d(dd) {}
    size_t begin()
    {
        if (!d->pfx) return 0;
        if (d->workers.size() > 1) return ZERR(kErrParameterUnsupported);
        if (is_device_ptr(d->pfx)) { d->pfxDev = (const u8*)d->pfx; return 0; }
        if (!d->pfxStage.ensure(d->pfxSize + 64)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(d->pfxStage.p, d->pfx, d->pfxSize, hipMemcpyHostToDevice, d->stream) != hipSuccess) return ZERR(kErrGeneric);
        d->pfxDev = (const u8*)d->pfxStage.p;
        return 0;
    }
    ~PrefixUse() { d->pfx = nullptr; d->pfxSize = 0; d->pfxDev = nullptr; }
};
static size_t ZSTDMI_decompressDevice_impl(ZSTD_DCtx* d, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize)
{
    if (!d) return ZERR(kErrGeneric);
    PrefixUse use(d);
    size_t e = set_check(d); if (isErr(e)) return e;
    e = dctx_bind(d); if (isErr(e)) return e;
    e = use.begin(); if (isErr(e)) return e;
    if (srcSize && !d_src) return ZERR(kErrSrcSizeWrong);
    if (d->workers.size() > 1 && srcSize) return decompress_multi(d, d_dst, dstCapacity, d_src, srcSize);
    return decompress_device(d, (u8*)d_dst, dstCapacity, (const u8*)d_src, srcSize);
}

static size_t ZSTD_decompressDCtx_impl(ZSTD_DCtx* d, void* dst, size_t dstCapacity, const void* src, size_t srcSize)
{
    if (!d) return ZERR(kErrGeneric);
    PrefixUse use(d);
    size_t e = set_check(d); if (isErr(e)) return e;
    e = dctx_bind(d); if (isErr(e)) return e;
    e = use.begin(); if (isErr(e)) return e;
    if (srcSize && !src) return ZERR(kErrSrcSizeWrong);
    if (srcSize == 0) return 0;
    if (d->workers.size() > 1) return decompress_multi(d, dst, dstCapacity, src, srcSize);
    const bool srcDev = is_device_ptr(src), dstDev = dst ? is_device_ptr(dst) : false;
    const u8* d_src = (const u8*)src; u8* d_dst = (u8*)dst;
    if (!srcDev) {
        if (!d->stageSrc.ensure(srcSize + 64)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(d->stageSrc.p, src, srcSize, hipMemcpyHostToDevice, d->stream) != hipSuccess) return ZERR(kErrGeneric);
        d_src = (const u8*)d->stageSrc.p;
    }
    if (!dstDev) {
        if (!d->stageDst.ensure(dstCapacity + 64)) return ZERR(kErrMemoryAllocation);
        d_dst = (u8*)d->stageDst.p;
    }
    const size_t r = decompress_device(d, d_dst, dstCapacity, d_src, srcSize);
    if (isErr(r)) return r;
    if (!dstDev && r) {
        if (hipMemcpyAsync(dst, d_dst, r, hipMemcpyDeviceToHost, d->stream) != hipSuccess) return ZERR(kErrGeneric);
        if (hipStreamSynchronize(d->stream) != hipSuccess) return ZERR(kErrGeneric);      // (deliberately not stream_wait: no hipGetLastError behind this wait)
    }
    return r;
}

// ---------------- several devices behind one context (ZSTDMI_DCtx_setDevices; the compressor's side: compress_multi, zstd_mi355x.hip) ----------------
// decompress: the frames of the input (a host-side header walk) in contiguous shares by compressed size
static size_t decompress_multi(ZSTD_DCtx* d, void* dst, size_t dstCapacity, const void* src, size_t srcSize)
{
    const size_t W = d->workers.size();
    bool ok = true;
    std::vector<u8> tmp;
    const u8* const ip = host_view(src, srcSize, tmp);
    if (!ip) return ZERR(kErrGeneric);
    struct Piece { size_t off, len; unsigned long long bound; bool sized; };
    std::vector<Piece> frames;
    { size_t pos = 0;
      while (pos < srcSize) {
          unsigned long long b = 0; const size_t fs = host_frame_size_info(ip + pos, srcSize - pos, &b);
          if (isErr(fs)) { if (frames.empty() || fs != ZERR(kErrPrefixUnknown)) return fs; return ZERR(kErrSrcSizeWrong); }     // as ZSTD_decompressMultiFrame: garbage behind a frame
          Piece p; p.off = pos; p.len = fs; p.bound = b;
          p.sized = ZSTD_getFrameContentSize_impl(ip + pos, fs) < (unsigned long long)0 - 2;
          frames.push_back(p); pos += fs;
      } }
    // shares of about equal compressed size
    std::vector<size_t> lo(W + 1, frames.size());
    { size_t acc = 0, k = 0; lo[0] = 0;
      for (size_t f = 0; f < frames.size(); ++f) { while (k + 1 < W && acc >= srcSize * (k + 1) / W) lo[++k] = f; acc += frames[f].len; }
      while (k + 1 < W) lo[++k] = frames.size(); lo[W] = frames.size(); }
    std::vector<size_t> res(W, 0), got(W, 0);
    std::vector<unsigned long long> bound(W, 0);
    bool allSized = true;
    for (size_t i = 0; i < W; ++i) for (size_t f = lo[i]; f < lo[i + 1]; ++f) { bound[i] += frames[f].bound; allSized = allSized && frames[f].sized; }
    if (allSized) { unsigned long long t = 0; for (size_t i = 0; i < W; ++i) t += bound[i]; if (t > dstCapacity) return ZERR(kErrDstSizeTooSmall); }
    { const size_t e = dctx_sync_dictionary(d); if (isErr(e)) return e; }
    for (ZSTD_DCtx* w : d->workers) {
        w->litDecoder = d->litDecoder; w->originMode = d->originMode; w->overlapMode = d->overlapMode; w->timer.enabled = d->timer.enabled;
        if (w->dictGen != d->dictGen) { w->dictHost = d->dictHost; w->dictFormatted = d->dictFormatted; w->dictDirty = true; w->dictGen = d->dictGen; }
    }
    std::vector<size_t> at(W, 0);
    for (size_t i = 1; i < W; ++i) at[i] = at[i - 1] + (size_t)bound[i - 1];       // exact when every frame has a content size
    ok = run_on_workers(W, [&](size_t i) {
        ZSTD_DCtx* w = d->workers[i];
        size_t e = dctx_bind(w); if (isErr(e)) { res[i] = e; return; }
        if (lo[i] == lo[i + 1]) return;
        const size_t a = frames[lo[i]].off, n = frames[lo[i + 1] - 1].off + frames[lo[i + 1] - 1].len - a;
        if (!w->stageSrc.ensure(n + 64) || !w->stageDst.ensure((size_t)bound[i] + 64)) { res[i] = ZERR(kErrMemoryAllocation); return; }
        e = copy_any(w->stageSrc.p, ip + a, n, w->stream); if (isErr(e)) { res[i] = e; return; }
        const size_t r = decompress_device(w, (u8*)w->stageDst.p, (size_t)bound[i], (const u8*)w->stageSrc.p, n);
        if (isErr(r)) { res[i] = r; return; }
        got[i] = r;
        if (allSized) {         // its place in the caller's buffer is known
            e = copy_any((u8*)dst + at[i], w->stageDst.p, r, w->stream);
            if (!isErr(e)) e = stream_wait(w->stream);
            if (isErr(e)) res[i] = e;
        }
    });
    if (!ok) return ZERR(kErrMemoryAllocation);
    for (size_t i = 0; i < W; ++i) if (isErr(res[i])) return res[i];          // the first share's error is the first frame's
    size_t total = 0;
    for (size_t i = 0; i < W; ++i) total += got[i];
    if (!allSized) {            // frames without a content size: the shares' places follow from what they regenerated
        if (total > dstCapacity) return ZERR(kErrDstSizeTooSmall);
        size_t pos = 0;
        for (size_t i = 0; i < W; ++i) {
            ZSTD_DCtx* w = d->workers[i];
            if (isErr(dctx_bind(w))) return ZERR(kErrGeneric);
            size_t e = copy_any((u8*)dst + pos, w->stageDst.p, got[i], w->stream); if (isErr(e)) return e;
            e = stream_wait(w->stream); if (isErr(e)) return e;
            pos += got[i];
        }
    }
    d->timer.n = d->workers[0]->timer.n;
    for (int i = 0; i < d->timer.n; i++) { d->timer.ms[i] = d->workers[0]->timer.ms[i]; d->timer.names[i] = d->workers[0]->timer.names[i]; }
    (void)dctx_bind(d);
    return total;
}

// ---------------- streaming adapter on the batched engine ----------------
// ZSTD_decompressStream (S/Decompressor.cs:97-106 <- S/DecompressionStream.cs:88-162; U/ZstdDecompress.cs:2816-3205).
// Compressed bytes are collected until at least one whole frame is present (frame sizes come from the block headers,
// ZSTD_findFrameSizeInfo); all whole frames collected so far are decoded in one GPU batch into a pending buffer that is
// handed out as the caller's output space allows.  Returns 0 when a frame boundary is reached and everything is flushed,
// an error, or a non-zero hint.  As in the reference (U/ZstdDecompress.cs:3170-3194) the last input byte is held hostage
// while decoded data is still pending, so that a caller who stops feeding at end of input still gets called back.
static size_t dstream_drain(ZSTD_DCtx* d, ZSTD_outBuffer* o)
{
    const size_t avail = d->dOut.size() - d->dOutPos, room = o->size - o->pos;
    const size_t n = avail < room ? avail : room;
    if (n) { memcpy((u8*)o->dst + o->pos, d->dOut.data() + d->dOutPos, n); o->pos += n; d->dOutPos += n; }
    if (d->dOutPos == d->dOut.size()) { d->dOut.clear(); d->dOutPos = 0; }
    return d->dOut.size() - d->dOutPos;
}
// ---------------- a long frame in segments (ZSTDMI_DCtx_setStreamSegment) ----------------
// With the switch on, a frame that is not whole when the adapter first looks at it — or holds at least `segBytes` of blocks — is decoded
// as it arrives: whenever that many bytes of whole blocks are buffered they become one FRAGMENT, an ordinary frame as far as the
// pipeline can tell: a header without content size and checksum, the carried blocks (earlier blocks that define a Huffman or FSE table
// still in force; the link kernels parse them and make them regenerate nothing), and the segment's blocks, the last one marked last.
// History is the context's device buffer, passed the way a referenced prefix is; the repcodes come from and go to a device triple;
// the frame's checksum runs over the segments' outputs with carried state (decode_stream.hip).
// a segment holds at most this many blocks, so that its output's bound (blocks x 128 KiB) stays 256 MiB whatever the blocks hold
constexpr size_t kSegMaxBlocks = 2048;
constexpr u64 kHistMax = kRecOffMax;            // (a match further back is refused by seq_decode: windowTooLarge)

// a zstd frame header as the segmented adapter needs it -> false: not all of it is there (or no zstd frame)
struct HostHeader { size_t fhs; u64 window, fcs; u32 didBytes; bool single, checksum; u8 wd; };
static bool host_header(const u8* src, size_t n, HostHeader* h)
{
    auto rd32 = [](const u8* p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); };
    if (n < 5 || rd32(src) != 0xFD2FB528u) return false;
    const u8 fhd = src[4];
    static const u32 did[4] = { 0, 1, 2, 4 }, fcsB[4] = { 0, 2, 4, 8 };
    const u32 single = (fhd >> 5) & 1, fcsId = fhd >> 6;
    h->fhs = 5 + !single + did[fhd & 3] + fcsB[fcsId] + (single && !fcsId);
    if (n < h->fhs) return false;
    h->single = single != 0; h->checksum = ((fhd >> 2) & 1) != 0; h->didBytes = did[fhd & 3]; h->wd = single ? 0 : src[5];
    size_t pos = 5 + !single + h->didBytes;
    h->fcs = ~0ull;
    switch (fcsId) {
    case 0: if (single) h->fcs = src[pos]; break;
    case 1: h->fcs = (u64)((u32)src[pos] | ((u32)src[pos + 1] << 8)) + 256; break;
    case 2: h->fcs = rd32(src + pos); break;
    default: h->fcs = (u64)rd32(src + pos) | ((u64)rd32(src + pos + 4) << 32); break;
    }
    if (single) h->window = h->fcs;
    else { const u32 wlog = (h->wd >> 3) + 10; const u64 w = 1ull << wlog; h->window = w + (w >> 3) * (h->wd & 7); }
    return true;
}
static u64 window_of_descriptor(u8 wd) { const u64 w = 1ull << ((wd >> 3) + 10); return w + (w >> 3) * (wd & 7); }
// the smallest window descriptor that covers `size` bytes (a single-segment frame has none of its own)
static u8 descriptor_covering(u64 size)
{
    for (u32 e = 0; e < 22; ++e) for (u32 m = 0; m < 8; ++m) { const u8 wd = (u8)((e << 3) | m); if (window_of_descriptor(wd) >= size) return wd; }
    return (u8)((21u << 3) | 7u);
}

static void stream_end_frame(ZSTD_DCtx* d)
{
    ZSTD_DCtx_s::StreamSeg& g = d->seg;
    g.active = false; g.first = true; g.lastSeen = false; g.carried.clear(); g.blocks.clear(); g.scanned = 0; g.histLen = 0; g.skip = 0;
}
static void stream_note_input(ZSTD_DCtx* d)
{
    size_t held = d->dIn.size();
    for (const auto& c : d->seg.carried) held += c.bytes.size();
    if ((long long)held > d->streamPeakInput) d->streamPeakInput = (long long)held;
}

// the frame whose header (all of it) is at the front of dIn begins: the fragment header, the first history, the checksum state
static size_t stream_begin_frame(ZSTD_DCtx* d, const HostHeader& h)
{
    ZSTD_DCtx_s::StreamSeg& g = d->seg;
    size_t e = dctx_bind(d); if (isErr(e)) return e;
    e = dctx_sync_dictionary(d); if (isErr(e)) return e;
    stream_end_frame(d);
    const u8* src = d->dIn.data();
    const u8 wd = h.single ? descriptor_covering(h.fcs) : h.wd;
    u32 n = 0;
    g.hdr[n++] = 0x28; g.hdr[n++] = 0xB5; g.hdr[n++] = 0x2F; g.hdr[n++] = 0xFD;
    g.hdr[n++] = (u8)(src[4] & 3);              // the dictID's size; no content size, no checksum, a window descriptor
    g.hdr[n++] = wd;
    for (u32 i = 0; i < h.didBytes; ++i) g.hdr[n++] = src[5 + !h.single + i];
    g.hdrLen = n;
    const u64 fragWindow = window_of_descriptor(wd);
    g.blockMax = fragWindow < (1u << 17) ? fragWindow : (1u << 17);
    g.histKeep = h.window < kHistMax ? h.window : kHistMax; g.window = h.window;
    g.fcs = h.fcs; g.checksum = h.checksum; g.produced = 0;
    if (!d->segReps.ensure(sizeof(DictInfo)) || !d->segXxh.ensure(sizeof(XxhCarry)) || !d->status.ensure(kStWords * sizeof(u32))) return ZERR(kErrMemoryAllocation);
    hipStream_t s = d->stream;
    const DecodeDict dd = decode_dict(d);
    if (dd.dictContent && dd.dictContentSize) {         // the dictionary's content, all of it, is the first history
        const u64 keep = dd.dictContentSize < kHistMax ? dd.dictContentSize : kHistMax;
        if (!d->hist[0].ensure((size_t)keep + 64)) return ZERR(kErrMemoryAllocation);
        if (hipMemcpyAsync(d->hist[0].p, dd.dictContent + (dd.dictContentSize - keep), (size_t)keep, hipMemcpyDeviceToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        g.histLen = keep; g.histCur = 0;
    }
    if (g.checksum) {
        xxh_carry_reset(&g.xxhHost);
        if (hipMemcpyAsync(d->segXxh.p, &g.xxhHost, sizeof g.xxhHost, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
    }
    e = stream_wait(s); if (isErr(e)) return e;
    d->dIn.erase(d->dIn.begin(), d->dIn.begin() + (ptrdiff_t)h.fhs);
    g.active = true;
    return 0;
}

// one fragment (srcSize bytes at d_src: header, `phantoms` carried blocks, the segment's blocks) through the pipeline -> its content
// in d_dst, the repcodes behind it in d->segReps.  -> the content's size, or the error
static size_t decode_fragment(ZSTD_DCtx* d, u8* d_dst, size_t dstCapacity, const u8* d_src, size_t srcSize, u32 phantoms)
{
    ZSTD_DCtx_s::StreamSeg& g = d->seg;
    hipStream_t s = d->stream;
    u32* status = (u32*)d->status.p;
    DecodeDict dd = decode_dict(d);
    dd.dictContent = g.histLen ? (const u8*)d->hist[g.histCur].p : nullptr; dd.dictContentSize = (u32)g.histLen;
    d->timer.begin(s);
    { const size_t e = status_reset(d); if (isErr(e)) return e; }
    u32 st[kStWords] = {};
    // (the exact serial walk: one frame, and it checks the dictID the fragment's header repeats)
    launch_frame_walk_serial(d_src, srcSize, nullptr, nullptr, 1, status, dd, 0, s);
    { const size_t e = status_read(d, st); if (isErr(e)) return e; }
    if (st[kStErr]) return ZERR(st[kStErr]);
    const u32 nFrames = st[kStFrames], nBlocks = st[kStBlocks];
    const u64 total = st_u64(st, kStTotalLo, kStTotalHi);
    if (nFrames != 1 || nBlocks <= phantoms || total > dstCapacity) return ZERR(kErrGeneric);       // (the host built it otherwise)
    if (!ensure_lists(d, lists_layout(nFrames, nBlocks, total, false))) return ZERR(kErrMemoryAllocation);
    FrameDesc* frames = (FrameDesc*)d->frames.p; BlockDesc* blocks = (BlockDesc*)d->blocks.p;
    launch_frame_walk_serial(d_src, srcSize, frames, blocks, 1, status, dd, 1, s);
    d->timer.mark("frame_walk", s);
    const StreamLink link = { phantoms, g.first ? nullptr : (const DictInfo*)d->segReps.p };
    { const size_t e = decode_lists(d, dd, d_dst, d_src, nFrames, nBlocks, 1, dstCapacity, st, [&]() -> bool {
          launch_stream_carry(blocks, nBlocks, (DictInfo*)d->segReps.p, s);
          return true;
      }, &link);
      if (isErr(e)) return e; }
    d->timer.finish();
    { const size_t e = status_error(st); if (isErr(e)) return e; }
    return (size_t)st_u64(st, kStActualLo, kStActualHi);
}

// the whole blocks at the front of dIn (g.blocks) as one segment: decoded into dOut, the carried state brought forward
static size_t stream_decode_segment(ZSTD_DCtx* d)
{
    ZSTD_DCtx_s::StreamSeg& g = d->seg;
    hipStream_t s = d->stream;
    size_t e = dctx_bind(d); if (isErr(e)) return e;
    const u32 P = (u32)g.carried.size();
    size_t fragSize = g.hdrLen + g.scanned;
    for (const auto& c : g.carried) fragSize += c.bytes.size();
    const size_t cap = (size_t)((P + g.blocks.size()) * g.blockMax);
    if (!d->stageSrc.ensure(fragSize + 64) || !d->stageDst.ensure(cap + 64)) return ZERR(kErrMemoryAllocation);
    u8* const frag = (u8*)d->stageSrc.p; u8* const out = (u8*)d->stageDst.p;
    size_t at = 0;
    auto put = [&](const u8* p, size_t n) -> bool { const bool ok = hipMemcpyAsync(frag + at, p, n, hipMemcpyHostToDevice, s) == hipSuccess; at += n; return ok; };
    if (!put(g.hdr, g.hdrLen)) return ZERR(kErrGeneric);
    for (const auto& c : g.carried) if (!put(c.bytes.data(), c.bytes.size())) return ZERR(kErrGeneric);
    const size_t lastAt = at + g.blocks.back().off;
    if (!put(d->dIn.data(), g.scanned)) return ZERR(kErrGeneric);
    g.lastByte = (u8)(d->dIn[g.blocks.back().off] | 1);         // the fragment ends with its last block
    if (hipMemcpyAsync(frag + lastAt, &g.lastByte, 1, hipMemcpyHostToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
    const size_t n = decode_fragment(d, out, cap, frag, fragSize, P);
    if (isErr(n)) return n;
    g.produced += n;
    if (g.fcs != ~0ull && (g.produced > g.fcs || (g.lastSeen && g.produced != g.fcs))) return ZERR(kErrCorruption);      // U/ZstdDecompress.cs:1177-1184
    XxhCarry& x = g.xxhHost;
    if (g.checksum) {           // (on this stream: beside the copies below, on the context's second stream, the stream was measured slower)
        launch_stream_xxh((XxhCarry*)d->segXxh.p, out, n, g.lastSeen ? 1u : 0u, s);
        if (g.lastSeen && hipMemcpyAsync(&x, d->segXxh.p, sizeof x, hipMemcpyDeviceToHost, s) != hipSuccess) return ZERR(kErrGeneric);
    }
    d->dOut.resize(n); d->dOutPos = 0;
    if (n && hipMemcpyAsync(d->dOut.data(), out, n, hipMemcpyDeviceToHost, s) != hipSuccess) return ZERR(kErrGeneric);
    if (!g.lastSeen) {          // what later blocks may reach of (history, this output), into the other buffer: everything while the
                                // frame has produced less than its window, the last histKeep bytes from then on
        const u64 limit = g.produced >= g.window ? g.histKeep : kHistMax;
        const u64 keep = g.histLen + n < limit ? g.histLen + n : limit;
        const u64 fromOut = n < keep ? n : keep, fromOld = keep - fromOut;
        DevBuf& to = d->hist[g.histCur ^ 1];
        // (a window of up to 64 MiB is allocated at once, a larger one doubles: every growth is a hipFree and a hipMalloc)
        u64 room = keep;
        if (to.cap < keep + 64) { const u64 top = g.histKeep > keep ? g.histKeep : keep; room = (g.histKeep <= (64u << 20) || 2 * keep > top) ? top : 2 * keep; }
        if (!to.ensure((size_t)room + 64)) return ZERR(kErrMemoryAllocation);
        if (fromOld && hipMemcpyAsync(to.p, (const u8*)d->hist[g.histCur].p + (g.histLen - fromOld), (size_t)fromOld, hipMemcpyDeviceToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        if (fromOut && hipMemcpyAsync((u8*)to.p + fromOld, out + (n - fromOut), (size_t)fromOut, hipMemcpyDeviceToDevice, s) != hipSuccess) return ZERR(kErrGeneric);
        g.histCur ^= 1; g.histLen = keep;
    }
    e = stream_wait(s); if (isErr(e)) return e;
    d->streamSegments++;
    g.first = false;
    size_t consumed = g.scanned;
    if (g.lastSeen) {
        if (g.checksum) {
            const u8* c = d->dIn.data() + g.scanned;
            const u32 want = (u32)c[0] | ((u32)c[1] << 8) | ((u32)c[2] << 16) | ((u32)c[3] << 24);
            if (x.hash != want) return ZERR(kErrChecksumWrong);
            consumed += 4;
        }
        d->dIn.erase(d->dIn.begin(), d->dIn.begin() + (ptrdiff_t)consumed);
        stream_end_frame(d);
        return 0;
    }
    // which blocks define the tables in force now: per table the latest definer, among the carried blocks and this segment's
    int owner[4] = { -1, -1, -1, -1 };
    for (u32 i = 0; i < P; ++i) for (u32 t = 0; t < 4; ++t) if (g.carried[i].defines & (1u << t)) owner[t] = (int)i;
    for (size_t j = 0; j < g.blocks.size(); ++j) for (u32 t = 0; t < 4; ++t) if (g.blocks[j].defines & (1u << t)) owner[t] = (int)(P + j);
    std::vector<ZSTD_DCtx_s::CarriedBlock> next;
    for (int k = 0; k < (int)(P + g.blocks.size()); ++k) {      // (stream order; at most four are kept)
        if (k != owner[0] && k != owner[1] && k != owner[2] && k != owner[3]) continue;
        ZSTD_DCtx_s::CarriedBlock c;
        if (k < (int)P) c = std::move(g.carried[k]);
        else { const ZSTD_DCtx_s::SegBlock& b = g.blocks[k - P]; c.bytes.assign(d->dIn.begin() + (ptrdiff_t)b.off, d->dIn.begin() + (ptrdiff_t)(b.off + b.size)); c.defines = b.defines; c.bytes[0] &= 0xFE; }
        next.push_back(std::move(c));
    }
    g.carried.swap(next);
    d->dIn.erase(d->dIn.begin(), d->dIn.begin() + (ptrdiff_t)consumed);
    g.blocks.clear(); g.scanned = 0;
    return 0;
}

// one step of the segmented adapter with nothing pending in dOut -> 1: something moved (output in dOut, or state), 0: more input is
// needed, or an error
static size_t stream_step(ZSTD_DCtx* d)
{
    ZSTD_DCtx_s::StreamSeg& g = d->seg;
    if (g.skip) {               // inside a skippable frame
        const size_t n = g.skip < d->dIn.size() ? (size_t)g.skip : d->dIn.size();
        d->dIn.erase(d->dIn.begin(), d->dIn.begin() + (ptrdiff_t)n); g.skip -= n;
        return n ? 1 : 0;
    }
    if (g.active) {
        const size_t segBytes = d->segBytes ? d->segBytes : 1;
        while (!g.lastSeen && g.blocks.size() < kSegMaxBlocks) {
            ScanBlock b;
            const size_t sz = scan_block(d->dIn.data() + g.scanned, d->dIn.size() - g.scanned, &b);
            if (!sz) break;
            if (b.type == 3) return ZERR(kErrCorruption);
            if (b.last && g.checksum && d->dIn.size() - (g.scanned + sz) < 4) break;        // whole only with its checksum
            g.blocks.push_back({ g.scanned, sz, b.defines }); g.scanned += sz;
            if (b.last) g.lastSeen = true;
        }
        if (g.blocks.empty() || !(g.lastSeen || g.scanned >= segBytes || g.blocks.size() >= kSegMaxBlocks)) return 0;
        const size_t e = stream_decode_segment(d);
        return isErr(e) ? e : 1;
    }
    // on a frame boundary: whole frames below the segment size go the way they always went, all that are there in one run
    size_t whole = 0; unsigned long long bound = 0;
    while (whole < d->dIn.size()) {
        const u8* p = d->dIn.data() + whole; const size_t n = d->dIn.size() - whole;
        { u64 w = host_frame_window(p, n);
          if (w && w < 1024) w = 1024;
          if (w > (1ull << d->windowLogMax)) { if (whole) break; return ZERR(kErrWindowTooLarge); } }
        unsigned long long b = 0;
        const size_t fs = host_frame_size_info(p, n, &b);
        HostHeader h;
        if (isErr(fs)) {
            if (whole) break;                                   // (first what is whole)
            if (fs != ZERR(kErrSrcSizeWrong)) return fs;
            if (n >= 8 && (((u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24)) & 0xFFFFFFF0u) == 0x184D2A50u) {
                g.skip = (u64)((u32)p[4] | ((u32)p[5] << 8) | ((u32)p[6] << 16) | ((u32)p[7] << 24)) + 8;
                return 1;
            }
            if (!host_header(p, n, &h)) return 0;               // the header itself is still arriving
            const size_t e = stream_begin_frame(d, h);
            return isErr(e) ? e : 1;
        }
        if (d->segBytes && host_header(p, n, &h) && fs - h.fhs - (h.checksum ? 4 : 0) >= d->segBytes) {
            if (whole) break;
            const size_t e = stream_begin_frame(d, h);
            return isErr(e) ? e : 1;
        }
        whole += fs; bound += b;
    }
    if (!whole) return 0;
    d->dOut.resize((size_t)bound); d->dOutPos = 0;
    const size_t r = ZSTD_decompressDCtx_impl(d, d->dOut.data(), d->dOut.size(), d->dIn.data(), whole);
    if (isErr(r)) { d->dOut.clear(); return r; }
    d->dOut.resize(r);
    d->dIn.erase(d->dIn.begin(), d->dIn.begin() + (ptrdiff_t)whole);
    return 1;
}

static size_t stream_segmented(ZSTD_DCtx* d, ZSTD_outBuffer* output, ZSTD_inBuffer* input)
{
    if (d->workers.size() > 1) return ZERR(kErrParameterUnsupported);      // (segments are one device's)
    if (d->hostage && input->pos < input->size) { input->pos++; d->hostage = false; }
    size_t pending = dstream_drain(d, output);
    if (!pending) {
        if (input->size > input->pos) { d->dIn.insert(d->dIn.end(), (const u8*)input->src + input->pos, (const u8*)input->src + input->size); input->pos = input->size; }
        stream_note_input(d);
        for (;;) {
            const size_t r = stream_step(d);
            if (isErr(r)) { d->dIn.clear(); d->dOut.clear(); d->dOutPos = 0; d->hostage = false; stream_end_frame(d); return r; }     // what was handed out stays handed out
            if (!r) break;
            pending = dstream_drain(d, output);
            if (pending) break;
        }
    }
    if (pending) {
        if (!d->hostage && input->pos == input->size && input->pos > 0) { input->pos--; d->hostage = true; }
        return 1;
    }
    if (d->hostage) return 1;
    return (!d->seg.active && !d->seg.skip && d->dIn.empty()) ? 0 : 1;     // 0 only on a frame boundary
}

static size_t ZSTD_decompressStream_impl(ZSTD_DCtx* d, ZSTD_outBuffer* output, ZSTD_inBuffer* input)
{
    if (!d || !output || !input) return ZERR(kErrGeneric);
    if (output->pos > output->size) return ZERR(104);
    if (input->pos > input->size) return ZERR(105);
    if (input->size > input->pos && !input->src) return ZERR(kErrSrcSizeWrong);
    if (output->size > output->pos && !output->dst) return ZERR(kErrDstBufferNull);
    if (d->pfx) return ZERR(kErrParameterUnsupported);         // (a referenced prefix serves one single call)
    { const size_t e = set_check(d, d->segBytes != 0); if (isErr(e)) return e; }       // (a DDict set serves whole frames only)
    if (d->segBytes || d->seg.active || d->seg.skip) return stream_segmented(d, output, input);     // (a frame begun in segments ends in segments)
    if (d->hostage && input->pos < input->size) { input->pos++; d->hostage = false; }       // that byte was consumed earlier
    size_t pending = dstream_drain(d, output);
    if (!pending) {
        const size_t n = input->size - input->pos;
        if (n) { d->dIn.insert(d->dIn.end(), (const u8*)input->src + input->pos, (const u8*)input->src + input->size); input->pos = input->size; }
        size_t whole = 0; unsigned long long bound = 0;
        while (whole < d->dIn.size()) {
            unsigned long long b = 0;
            // ZSTD_d_windowLogMax bounds what a streamed frame may ask for (U/ZstdDecompress.cs:2966-2969, with the 1 KiB floor of
            // :2965): checked as soon as the header is there, before the frame is collected or anything is sized from it
            { u64 w = host_frame_window(d->dIn.data() + whole, d->dIn.size() - whole);
              if (w && w < 1024) w = 1024;
              if (w > (1ull << d->windowLogMax)) { d->dIn.clear(); return ZERR(kErrWindowTooLarge); } }
            const size_t fs = host_frame_size_info(d->dIn.data() + whole, d->dIn.size() - whole, &b);
            if (isErr(fs)) { if (fs == ZERR(kErrSrcSizeWrong)) break; return fs; }          // incomplete frame: wait for more input
            whole += fs; bound += b;
        }
        if (whole) {
            d->dOut.resize((size_t)bound); d->dOutPos = 0;
            const size_t r = ZSTD_decompressDCtx_impl(d, d->dOut.data(), d->dOut.size(), d->dIn.data(), whole);
            if (isErr(r)) { d->dOut.clear(); return r; }
            d->dOut.resize(r);
            d->dIn.erase(d->dIn.begin(), d->dIn.begin() + (ptrdiff_t)whole);
            pending = dstream_drain(d, output);
        }
    }
    if (pending) {
        if (!d->hostage && input->pos == input->size && input->pos > 0) { input->pos--; d->hostage = true; }
        return 1;
    }
    if (d->hostage) return 1;                                  // flushed, but the hostage byte has not been handed back yet
    return d->dIn.empty() ? 0 : 1;                             // 0 only on a frame boundary
}

// ---------------- digested dictionaries (ZSTD_createDDict, U/ZstdDdict.cs:178-279; ZSTD_DCtx_refDDict, U/ZstdDecompress.cs:2300) ----------------
static ZSTD_DDict* create_ddict(const void* dict, size_t dictSize, int device)
{
    if ((dictSize && !dict) || dictSize > (size_t)1 << 30) return nullptr;
    if (device < 0 || device_count() <= device) return nullptr;       // no gfx950 device: no digest
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    ZSTD_DDict_s* g = new (std::nothrow) ZSTD_DDict_s();
    if (!g) return nullptr;
    g->device = device;
    bool ok = true;
    try { g->host.resize(dictSize); } catch (...) { ok = false; }      // (nothing of a half-made DDict is left behind)
    ok = ok && (!dictSize || hipMemcpy(g->host.data(), dict, dictSize, hipMemcpyDefault) == hipSuccess);
    g->formatted = ok && is_formatted_dictionary(g->host.data(), dictSize);
    hipStream_t s = nullptr;
    if (ok && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { s = nullptr; ok = false; }
    if (ok && dictSize) {
        ok = g->dict.ensure(dictSize + 64) && g->dictInfoDev.ensure(sizeof(DictInfo)) &&
             hipMemcpyAsync(g->dict.p, g->host.data(), dictSize, hipMemcpyHostToDevice, s) == hipSuccess;
        if (ok && g->formatted) {
            launch_dict_parse((const u8*)g->dict.p, (u32)dictSize, (DictInfo*)g->dictInfoDev.p, s);
            ok = !isErr(dev_read(&g->info, g->dictInfoDev.p, sizeof(DictInfo), s)) && !g->info.err;      // (what dict_parse refuses never becomes a DDict)
            if (ok) {
                u32 logs[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu };
                ok = g->seqTabs.ensure(kDictTabWords * sizeof(u32));
                if (ok) {
                    launch_dict_seq_tables((const u8*)g->dict.p, (const DictInfo*)g->dictInfoDev.p, (u32*)g->seqTabs.p, s);
                    ok = !isErr(dev_read(logs, (const u32*)g->seqTabs.p + kDictTabLogs, sizeof logs, s)) &&
                         logs[0] != 0xFFFFFFFFu && logs[1] != 0xFFFFFFFFu && logs[2] != 0xFFFFFFFFu;
                }
            }
        }
        if (ok) ok = !isErr(stream_wait(s));
    }
    if (s) (void)hipStreamDestroy(s);
    if (!ok) { (void)hipGetLastError(); g->dict.release(); g->dictInfoDev.release(); g->seqTabs.release(); delete g; return nullptr; }
    return g;
}
ZSTD_DDict* ZSTDMI_createDDictOnDevice(const void* dict, size_t dictSize, int device) { return create_ddict(dict, dictSize, device); }
ZSTD_DDict* ZSTD_createDDict(const void* dict, size_t dictSize) { return ZSTDMI_createDDictOnDevice(dict, dictSize, 0); }
size_t ZSTD_freeDDict(ZSTD_DDict* g)
{
    if (!g) return 0;
    if (hipSetDevice(g->device) == hipSuccess) { g->dict.release(); g->dictInfoDev.release(); g->seqTabs.release(); } else (void)hipGetLastError();
    delete g;
    return 0;
}
size_t ZSTD_sizeof_DDict(const ZSTD_DDict* g) { return g ? sizeof(*g) + g->host.capacity() + g->dict.cap + g->dictInfoDev.cap + g->seqTabs.cap : 0; }
unsigned ZSTD_getDictID_fromDDict(const ZSTD_DDict* g) { return (g && g->formatted) ? g->info.dictID : 0u; }
// The context's own dictionary fields follow its reference: empty while the DDict is shared, a private copy of its bytes (uploaded by
// the next call, exactly as after ZSTD_DCtx_loadDictionary) while it cannot be.  Touches no device.
static void dctx_adopt_ddict(ZSTD_DCtx* d)
{
    d->dictGen++; d->dictDirty = true; d->dictHost.clear(); d->dictFormatted = false;
    if (!d->ddict || ddict_shared(d)) return;
    d->dictHost = d->ddict->host; d->dictFormatted = d->ddict->formatted;
}
size_t ZSTD_DCtx_refDDict(ZSTD_DCtx* d, const ZSTD_DDict* ddict)
{
    if (!d) return ZERR(kErrGeneric);
    return guarded([&]() -> size_t {
        tl_waits = &d->tally.waits;
        if (d->deviceOk && hipSetDevice(d->device) == hipSuccess) dctx_async_drain(d);      // (an enqueued batch reads the DDict it was prepared behind)
        // ZSTD_d_refMultipleDDicts: the DDict also joins the set, replacing an entry of equal dictID (U/ZstdDecompress.cs:2319-2333); a set
        // that cannot take it leaves the context as it was.  NULL clears the current DDict only (ZSTD_clearDict).  No device is touched.
        if (ddict && d->refMultiple && !d->ddictSet.insert(ZSTD_getDictID_fromDDict(ddict), ddict)) return ZERR(kErrMemoryAllocation);
        d->pfx = nullptr; d->pfxSize = 0;       // ZSTD_clearAllDicts: a loaded dictionary and a pending prefix are gone
        d->ddict = ddict;
        d->setGen++;
        dctx_adopt_ddict(d);
        return 0;
    });
}
size_t ZSTD_decompress_usingDDict(ZSTD_DCtx* d, void* dst, size_t dstCapacity, const void* src, size_t srcSize, const ZSTD_DDict* ddict)
{
    if (!d || !ddict) return ZERR(kErrGeneric);
    // the context's own dictionary or reference and a pending prefix step aside for the call and are left as found (where the DDict
    // cannot be shared, the context's bytes are uploaded again by their next use)
    return guarded([&]() -> size_t {
        d->lastDictTabBlocks = d->lastSetFrames = 0;
        const ZSTD_DDict_s* const was = d->ddict;
        const void* const pfx = d->pfx; const size_t pfxSize = d->pfxSize;
        d->pfx = nullptr; d->pfxSize = 0;
        d->ddict = ddict;
        const int multi = d->refMultiple; d->refMultiple = 0;       // ONE call behind this DDict alone: the set steps aside too (and its image stays good)
        size_t r;
        if (ddict_shared(d)) r = ZSTD_decompressDCtx_impl(d, dst, dstCapacity, src, srcSize);
        else {
            std::vector<u8> h; const bool fmt = d->dictFormatted;
            h.swap(d->dictHost);
            try { dctx_adopt_ddict(d); r = ZSTD_decompressDCtx_impl(d, dst, dstCapacity, src, srcSize); }
            catch (...) { r = ZERR(kErrMemoryAllocation); }
            d->dictHost.swap(h); d->dictFormatted = fmt; d->dictDirty = true; d->dictGen++;
        }
        d->ddict = was; d->pfx = pfx; d->pfxSize = pfxSize; d->refMultiple = multi;
        return r;
    });
}
long long ZSTDMI_debugDictUploadsD(const ZSTD_DCtx* d)
{
    if (!d) return -1;
    long long n = d->dictUploads;
    for (const ZSTD_DCtx* w : d->workers) n += w->dictUploads;
    return n;
}
long long ZSTDMI_debugLastDictTableBlocks(const ZSTD_DCtx* d) { return d ? d->lastDictTabBlocks : -1; }
long long ZSTDMI_debugLastSetFrames(const ZSTD_DCtx* d) { return d ? d->lastSetFrames : -1; }
// host memory in, no device touched (zmi_dictid.h)
unsigned ZSTD_getDictID_fromDict(const void* dict, size_t dictSize) { return dictid_from_dict((const u8*)dict, dictSize); }
unsigned ZSTD_getDictID_fromFrame(const void* src, size_t srcSize) { return dictid_from_frame((const u8*)src, srcSize); }

// ---------------- extensions ----------------
// (a referenced DDict is shared or copied by where the context runs: dctx_adopt_ddict)
size_t ZSTDMI_DCtx_setDevice(ZSTD_DCtx* d, int device) { if (d) d->paramGen++; const size_t e = ctx_set_device(d, device); if (d) d->setGen++; if (d && d->ddict) (void)guarded([&]() -> size_t { dctx_adopt_ddict(d); return 0; }); return e; }
size_t ZSTDMI_DCtx_setDevices(ZSTD_DCtx* d, const int* devices, int n)
{
    if (d) d->paramGen++;
    const size_t e = ctx_set_devices(d, devices, n, ZSTD_createDCtx, ZSTD_freeDCtx);
    if (d) d->setGen++;
    if (d && d->ddict) (void)guarded([&]() -> size_t { dctx_adopt_ddict(d); return 0; });
    return e;
}
size_t ZSTDMI_DCtx_setStream(ZSTD_DCtx* d, void* st)
{
    if (d && d->deviceOk && (st ? (hipStream_t)st : d->ownStream) != d->stream && hipSetDevice(d->device) == hipSuccess) dctx_async_drain(d);    // (the new stream is not ordered behind an enqueued batch)
    return ctx_set_stream(d, st, dctx_bind);
}
size_t ZSTDMI_DCtx_setStreamSegment(ZSTD_DCtx* d, size_t bytes)
{
    if (!d) return ZERR(kErrGeneric);
    d->segBytes = bytes; d->streamSegments = 0; d->streamPeakInput = 0; d->paramGen++;
    return 0;
}
long long ZSTDMI_debugStreamPeakInput(const ZSTD_DCtx* d) { return d ? d->streamPeakInput : -1; }
int ZSTDMI_debugStreamSegments(const ZSTD_DCtx* d) { return d ? d->streamSegments : -1; }
int ZSTDMI_debugLastWalkSerial(const ZSTD_DCtx* d) { return d ? (int)d->lastWalkSerial : -1; }
int ZSTDMI_debugLastFarPlane(const ZSTD_DCtx* d) { return d ? d->lastFarPlane : -1; }
size_t ZSTDMI_DCtx_setExecWaves(ZSTD_DCtx* d, unsigned waves) { if (!d || (waves != 0 && waves != 1 && waves != 2 && waves != 4 && waves != 8 && waves != 16)) return ZERR(kErrParameterOutOfBound); d->execWaves = (int)waves; d->paramGen++; return 0; }
size_t ZSTDMI_DCtx_setOverlap(ZSTD_DCtx* d, unsigned mode) { if (!d || mode > 2) return ZERR(kErrParameterOutOfBound); d->overlapMode = (int)mode; d->paramGen++; return 0; }
size_t ZSTDMI_DCtx_setLongFrames(ZSTD_DCtx* d, unsigned mode) { if (!d || mode > 2) return ZERR(kErrParameterOutOfBound); d->originMode = (int)mode; d->paramGen++; return 0; }
size_t ZSTDMI_DCtx_setLiteralDecoder(ZSTD_DCtx* d, unsigned mode) { if (!d || mode > 3) return ZERR(kErrParameterOutOfBound); d->litDecoder = mode; d->paramGen++; return 0; }
size_t ZSTDMI_DCtx_setProfiling(ZSTD_DCtx* d, int en) { if (!d) return ZERR(kErrGeneric); d->timer.enabled = en != 0; d->paramGen++; return 0; }
int ZSTDMI_DCtx_getStageTimes(const ZSTD_DCtx* d, float* ms, const char** names, int cap)
{
    if (!d) return 0;
    int n = d->timer.n < cap ? d->timer.n : cap;
    for (int i = 0; i < n; i++) { if (ms) ms[i] = d->timer.ms[i]; if (names) names[i] = d->timer.names[i]; }
    return n;
}

// ---------------- entry points whose host-side containers may throw: guarded (see guarded()) ----------------
size_t ZSTD_DCtx_loadDictionary(ZSTD_DCtx* d, const void* dict, size_t dictSize) { return guarded([&] { return ZSTD_DCtx_loadDictionary_impl(d, dict, dictSize); }); }
size_t ZSTD_DCtx_refPrefix(ZSTD_DCtx* d, const void* prefix, size_t prefixSize)
{
    if (!d) return ZERR(kErrGeneric);
    if (prefix && prefixSize > (size_t)1 << 30) return ZERR(kErrParameterUnsupported);
    // ZSTD_clearAllDicts: a loaded dictionary, a referenced DDict and an earlier prefix are gone
    if (d->deviceOk && hipSetDevice(d->device) == hipSuccess) dctx_async_drain(d);
    d->ddict = nullptr;
    d->dictGen++; d->dictHost.clear(); d->dictFormatted = false; d->dictDirty = true;
    d->pfx = nullptr; d->pfxSize = 0;
    if (prefix && prefixSize) { d->pfx = prefix; d->pfxSize = prefixSize; }
    return 0;
}
size_t ZSTD_findFrameCompressedSize(const void* src, size_t srcSize) { return guarded([&] { return ZSTD_findFrameCompressedSize_impl(src, srcSize); }); }
size_t ZSTD_decompressDCtx(ZSTD_DCtx* d, void* dst, size_t dstCapacity, const void* src, size_t srcSize) { return guarded([&] { if (d) d->lastDictTabBlocks = d->lastSetFrames = 0; return ZSTD_decompressDCtx_impl(d, dst, dstCapacity, src, srcSize); }); }
size_t ZSTDMI_decompressBatch(ZSTD_DCtx* d, const void* const* srcs, const size_t* srcSizes, size_t n, void* const* dsts, const size_t* dstCapacities, size_t* dstSizes)
{
    return guarded([&] { if (d) d->lastDictTabBlocks = d->lastSetFrames = 0; return decompress_batch_impl(d, srcs, srcSizes, n, dsts, dstCapacities, dstSizes); });
}
size_t ZSTDMI_batchAsyncWorkspaceD(const ZSTDMI_DBatchLimits* limits)
{
    size_t maxEntries; u64 bound; BatchLimitsD lim;
    return limits && dbatch_limits(limits, maxEntries, bound, lim) ? dbatch_needs(maxEntries, lim).sum() : 0;
}
size_t ZSTDMI_DCtx_prepareBatchAsync(ZSTD_DCtx* d, const ZSTDMI_DBatchLimits* limits) { return guarded([&] { return prepare_batch_async_d_impl(d, limits); }); }
size_t ZSTDMI_decompressBatchAsync(ZSTD_DCtx* d, const void* const* d_srcs, const size_t* d_srcSizes, size_t n, void* const* d_dsts, const size_t* d_dstCapacities, size_t* d_dstSizes)
{
    return guarded([&] { return decompress_batch_async_impl(d, d_srcs, d_srcSizes, n, d_dsts, d_dstCapacities, d_dstSizes); });
}
long long ZSTDMI_debugHostWaitsD(const ZSTD_DCtx* d) { return d ? d->tally.waits : -1; }
long long ZSTDMI_debugDeviceAllocsD(const ZSTD_DCtx* d) { return d ? d->tally.allocs : -1; }
int ZSTDMI_debugLastBatchAloneD(const ZSTD_DCtx* d) { return d ? d->lastBatchAlone : -1; }
size_t ZSTDMI_DCtx_setBatchUnsized(ZSTD_DCtx* d, unsigned mode) { if (!d || mode > 1) return ZERR(kErrParameterOutOfBound); d->batchUnsized = (int)mode; d->paramGen++; return 0; }
long long ZSTDMI_debugLastBatchWorkspace(const ZSTD_DCtx* d) { return d ? d->lastBatchWs : -1; }
size_t ZSTDMI_decompressRange(ZSTD_DCtx* d, void* dst, size_t dstCapacity, const void* src, size_t srcSize, unsigned long long offset, size_t length)
{
    if (!d) return ZERR(kErrGeneric);
    return guarded([&] { d->lastDictTabBlocks = d->lastSetFrames = 0; return decompress_range_impl(d, dst, dstCapacity, src, srcSize, offset, length); });
}
int ZSTDMI_debugLastRangeFrames(const ZSTD_DCtx* d) { return d ? d->lastRangeFrames : -1; }
long long ZSTDMI_debugLastRangeStaged(const ZSTD_DCtx* d) { return d ? d->lastRangeStaged : -1; }
size_t ZSTDMI_decompressRanges(ZSTD_DCtx* d, const void* src, size_t srcSize, const unsigned long long* offsets, const size_t* lengths, size_t n,
                               void* const* dsts, const size_t* dstCapacities, size_t* dstSizes)
{
    return guarded([&] { if (d) d->lastDictTabBlocks = d->lastSetFrames = 0; return decompress_ranges_impl(d, src, srcSize, offsets, lengths, n, dsts, dstCapacities, dstSizes); });
}
size_t ZSTDMI_rangesAsyncWorkspaceD(const ZSTDMI_DRangesLimits* limits, size_t tableEntries)
{
    BatchLimitsD lim; u32 nRows;
    return limits && dranges_limits(limits, tableEntries, lim, nRows) ? dranges_needs(limits->maxRanges, (u32)tableEntries, nRows, lim).sum() : 0;
}
size_t ZSTDMI_DCtx_prepareRangesAsync(ZSTD_DCtx* d, const void* d_src, size_t srcSize, const ZSTDMI_DRangesLimits* limits)
{
    return guarded([&] { return prepare_ranges_async_impl(d, d_src, srcSize, limits); });
}
size_t ZSTDMI_DCtx_getRangesAsyncPlan(const ZSTD_DCtx* d, size_t* tableEntries, unsigned long long* totalContent)
{
    if (!d) return ZERR(kErrGeneric);
    const DRangesPrep* const P = d->rangesPrep;
    if (!prep_valid(d, P)) return ZERR(kErrStageWrong);
    if (tableEntries) *tableEntries = P->n;
    if (totalContent) *totalContent = P->total;
    return 0;
}
size_t ZSTDMI_decompressRangesAsync(ZSTD_DCtx* d, const unsigned long long* d_offsets, const size_t* d_lengths, size_t n, void* const* d_dsts,
                                    const size_t* d_dstCapacities, size_t* d_dstSizes)
{
    return guarded([&] { return decompress_ranges_async_impl(d, d_offsets, d_lengths, n, d_dsts, d_dstCapacities, d_dstSizes); });
}
int ZSTDMI_debugLastRangesFrames(const ZSTD_DCtx* d) { return d ? d->lastRangesFrames : -1; }
int ZSTDMI_debugLastRangesAlone(const ZSTD_DCtx* d) { return d ? d->lastRangesAlone : -1; }
long long ZSTDMI_debugLastRangesStaged(const ZSTD_DCtx* d) { return d ? d->lastRangesStaged : -1; }
size_t ZSTDMI_decompressDevice(ZSTD_DCtx* d, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize) { return guarded([&] { if (d) d->lastDictTabBlocks = d->lastSetFrames = 0; return ZSTDMI_decompressDevice_impl(d, d_dst, dstCapacity, d_src, srcSize); }); }
size_t ZSTD_decompressStream(ZSTD_DCtx* d, ZSTD_outBuffer* output, ZSTD_inBuffer* input) { return guarded([&] { if (d) d->lastDictTabBlocks = d->lastSetFrames = 0; return ZSTD_decompressStream_impl(d, output, input); }); }
unsigned long long ZSTD_decompressBound(const void* src, size_t srcSize)
{
    try { return ZSTD_decompressBound_impl(src, srcSize); } catch (...) { return (unsigned long long)0 - 2; }      /* ZSTD_CONTENTSIZE_ERROR */
}
unsigned long long ZSTD_getFrameContentSize(const void* src, size_t srcSize)
{
    try { return ZSTD_getFrameContentSize_impl(src, srcSize); } catch (...) { return (unsigned long long)0 - 2; }      /* ZSTD_CONTENTSIZE_ERROR */
}

} // extern "C"
