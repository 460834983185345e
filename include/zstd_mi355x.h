/*
 * zstd_mi355x.h — C ABI of libzstd_mi355x.so, the MI355X (gfx950) block compressor/decompressor that sits
 * behind ZstdSharp's one-shot path (Compressor.Wrap / Decompressor.Unwrap).
 *
 * Every ZSTD_* entry point below keeps the name, argument order, types and error convention of the function the
 * reference calls at that point, so the reference's own P/Invoke precedent
 * (/root/reference/src/Zstd.Extern/ExternMethods.cs:8-42: cdecl, IntPtr contexts/buffers, nuint sizes, 32-bit
 * enums) binds to this library unchanged, and a `Methods`-shaped shim lets Compressor.cs / Decompressor.cs
 * compile as they are.  Citations: S/ = src/ZstdSharp/, U/ = src/ZstdSharp/Unsafe/.
 *
 * Return convention (U/ErrorPrivate.cs:10-24): size_t result; it is an error iff > (size_t)-120, and then
 * (0 - result) is a ZSTD_ErrorCode (U/ZSTD_ErrorCode.cs).  A too-small destination yields exactly (size_t)-70,
 * which TryWrap/TryUnwrap test for (S/Compressor.cs:116-120, S/Decompressor.cs:105-109).
 *
 * Buffers may be host memory (as the C# callers pass, pinned only for the call) or device memory (HBM): the
 * library asks the HIP runtime which it is and stages host buffers itself.  Nothing is retained after return.
 * One context is used by one thread at a time; any number of contexts may be used concurrently.
 */
#ifndef ZSTD_MI355X_H
#define ZSTD_MI355X_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ZSTD_CCtx_s ZSTD_CCtx;
typedef struct ZSTD_DCtx_s ZSTD_DCtx;
typedef struct ZSTD_CDict_s ZSTD_CDict;
typedef struct ZSTD_DDict_s ZSTD_DDict;

/* U/ZSTD_cParameter.cs / U/ZSTD_dParameter.cs values that the safe API uses */
enum {
    ZSTD_c_compressionLevel = 100, ZSTD_c_windowLog = 101, ZSTD_c_hashLog = 102, ZSTD_c_chainLog = 103,
    ZSTD_c_searchLog = 104, ZSTD_c_minMatch = 105, ZSTD_c_targetLength = 106, ZSTD_c_strategy = 107,
    ZSTD_c_enableLongDistanceMatching = 160, ZSTD_c_ldmHashLog = 161, ZSTD_c_ldmMinMatch = 162, ZSTD_c_ldmBucketSizeLog = 163,
    ZSTD_c_ldmHashRateLog = 164,
    ZSTD_c_contentSizeFlag = 200, ZSTD_c_checksumFlag = 201, ZSTD_c_dictIDFlag = 202, ZSTD_c_nbWorkers = 400,
    ZSTD_d_windowLogMax = 100,
    ZSTD_d_refMultipleDDicts = 1003         /* ZSTD_d_experimentalParam4, as in the reference */
};
/* U/ZSTD_refMultipleDDicts_e.cs: the values of ZSTD_d_refMultipleDDicts */
enum { ZSTD_rmd_refSingleDDict = 0, ZSTD_rmd_refMultipleDDicts = 1 };
/* U/ZSTD_paramSwitch_e.cs: the values of ZSTD_c_enableLongDistanceMatching */
enum { ZSTD_ps_auto = 0, ZSTD_ps_enable = 1, ZSTD_ps_disable = 2 };

/* ---- compression context: S/Compressor.cs:32,60,138 -> U/ZstdCompress.cs:24-27, 43-62, 137-160 ---- */
ZSTD_CCtx* ZSTD_createCCtx(void);
size_t     ZSTD_freeCCtx(ZSTD_CCtx* cctx);                                   /* NULL is accepted */
/* S/Compressor.cs:48-54 -> U/ZstdCompress.cs:819-884, 1270-1283.  compressionLevel (negative levels included: fast strategy
 * with a probing step and raw literals, as U/ZstdCompress.cs:7915-7920 + U/ZstdCompressInternal.cs:146-173), checksumFlag,
 * dictIDFlag, strategy (1..9, mapped onto the three finders) and targetLength are honoured; windowLog >= 16, contentSizeFlag = 1,
 * nbWorkers = 0, and for hashLog / minMatch / chainLog / searchLog the value the kernels implement (13; 6 or 5; the level's
 * own) are accepted; anything else within bounds returns parameter_unsupported — nothing is silently ignored.
 * Long-distance matching (U/ZstdLdm.cs, U/ZstdCompress.cs:560-595, 1106-1160): ZSTD_c_enableLongDistanceMatching = ZSTD_ps_enable
 * adds matches at any distance inside a window (ZSTD_c_windowLog, default 2^27 under LDM, shrunk to the input) to what the block
 * finders find.  A frame then holds min(window, 512 MiB, one pass) of content; windows below 2^17 and inputs of one block
 * (<= 64 KiB) are written as without LDM.  ldmHashLog (6..30), ldmMinMatch (4..4096), ldmBucketSizeLog (1..8) and ldmHashRateLog
 * (0..25) follow ZSTD_ldm_adjustParameters when 0; ldmHashRateLog 1..4 returns parameter_unsupported (the split workspace holds at
 * most one split per 16 bytes), and a derived one below 5 is raised to 5.  ZSTD_ps_auto (the default) and ZSTD_ps_disable write
 * exactly what a context that never set the switch writes: the reference's auto rule (on for btopt and above at windowLog >= 27,
 * U/ZstdCompress.cs:276-284) is deliberately not adopted, so that no level's output changes.  ZSTD_compressCCtx ignores the switch
 * (level-only parameters, as the reference).  With a dictionary loaded (ZSTD_CCtx_loadDictionary), an LDM call of more than one block
 * returns parameter_unsupported from ZSTD_compress2 (ZSTD_CCtx_refPrefix is the way to match into a second buffer); ZSTD_compressStream2 finds LDM matches inside each 16 MiB batch, not across batches
 * unless the session writes one frame with a sliding window (ZSTDMI_CCtx_setSingleFrame with ZSTDMI_CCtx_setSlidingLdm, below). */
size_t     ZSTD_CCtx_setParameter(ZSTD_CCtx* cctx, int param, int value);
size_t     ZSTD_CCtx_getParameter(const ZSTD_CCtx* cctx, int param, int* value);
/* S/Compressor.cs:43-56 (dictionary load) -> U/ZstdCompress.cs:1286-1330, 5465-5503.  RAW-CONTENT dictionaries (any bytes
 * that do not start with the magic 0xEC30A437): history in front of every frame, no dictID.  FORMATTED dictionaries (the
 * magic, a dictID, entropy tables, repcodes, content — what the trainer returns): the content is the history, the frames
 * carry the dictID (unless ZSTD_c_dictIDFlag = 0) and start from the dictionary's repcodes; its entropy tables are not
 * used by default (every block carries its own — valid for any decoder holding the dictionary); ZSTDMI_CCtx_setDictEntropy(1)
 * turns them on.  A malformed header ->
 * dictionary_corrupted (at this call when a device is bound, else at first use).  NULL/0 = no dictionary; under 8 bytes =
 * ignored, as in the reference.  The pointer may be host or device memory; the bytes are copied. */
size_t     ZSTD_CCtx_loadDictionary(ZSTD_CCtx* cctx, const void* dict, size_t dictSize);
/* U/ZstdCompress.cs:1723-1765: compress the next frame as a delta of `prefix` (the older version of the buffer; what zstd --patch-from
 * is built on).  The prefix is RAW CONTENT whatever it starts with, host or device memory, REFERENCED, not copied: it must stay valid
 * and unchanged until the consuming call returns (a device prefix is read in place, a host prefix is staged to HBM inside that call).
 * Any call, NULL/0 included, cancels a loaded dictionary and an earlier prefix; ZSTD_CCtx_loadDictionary cancels a pending prefix.  The
 * call touches no device.  NULL context: GENERIC; above 1 GiB: parameter_unsupported.
 * SINGLE USE: the next ZSTD_compress2 or ZSTDMI_compressDevice consumes it, whatever that call returns; the call after that writes what
 * a context without a prefix writes.  ZSTD_compressCCtx ignores it and leaves it pending.  While it is pending, ZSTD_compressStream2,
 * ZSTDMI_compressBatch, a context with the seek-table switch on and a context with several device workers: parameter_unsupported.
 * The consuming call writes ONE frame (ZSTD_DCtx_refPrefix serves one):
 *   under 8 bytes      ignored, as in the reference;
 *   short form         round_up(prefixSize, 4 KiB) + srcSize <= 64 KiB: exactly the bytes of ZSTD_CCtx_loadDictionary(the same raw
 *                      bytes) followed by the same call;
 *   long form          everything else: one single-segment frame with the content size, in the blocks of the long-distance framing for
 *                      the level.  The block finders see no prefix; the long-distance stage indexes prefix and source as one window and
 *                      runs unless ZSTD_c_enableLongDistanceMatching is ZSTD_ps_disable (ZSTD_ps_auto means ON here); its parameters
 *                      left at 0 derive from windowLog = ceil_log2(prefixSize + srcSize), at least 17.
 * The long form refuses with parameter_unsupported, before any byte is read: ZSTD_ps_disable, prefixSize + srcSize > 512 MiB (with
 * ZSTDMI_CCtx_setFarOffsets on: > 2^31), a source of more than one pass (ZSTDMI_CCtx_setPassChunks), ZSTD_c_contentSizeFlag = 0, and a set
 * ZSTD_c_windowLog below ceil_log2(prefixSize + srcSize).  The bytes written depend on the prefix's and the source's bytes alone. */
size_t     ZSTD_CCtx_refPrefix(ZSTD_CCtx* cctx, const void* prefix, size_t prefixSize);
/* S/Compressor.cs:73-76 -> U/ZstdCompress.cs:19-22 */
size_t     ZSTD_compressBound(size_t srcSize);
/* S/Compressor.cs:94 -> U/ZstdCompress.cs:7138-7177 */
size_t     ZSTD_compress2(ZSTD_CCtx* cctx, void* dst, size_t dstCapacity, const void* src, size_t srcSize);
/* B/Benchmark.cs:67, X/ExternMethods.cs:17-18 -> U/ZstdCompress.cs:5751-5776: the level alone — default frame parameters, no
 * dictionary even if one is loaded; the context's sticky parameters and dictionary are left as they are */
size_t     ZSTD_compressCCtx(ZSTD_CCtx* cctx, void* dst, size_t dstCapacity, const void* src, size_t srcSize, int compressionLevel);
/* S/Compressor.cs:8-9 -> U/ZstdCompress.cs:7762-7770 */
int        ZSTD_minCLevel(void);
int        ZSTD_maxCLevel(void);
int        ZSTD_defaultCLevel(void);

/* ---- decompression context: S/Decompressor.cs:12,25,124 -> U/ZstdDecompress.cs:326-395 ---- */
ZSTD_DCtx* ZSTD_createDCtx(void);
size_t     ZSTD_freeDCtx(ZSTD_DCtx* dctx);
size_t     ZSTD_DCtx_setParameter(ZSTD_DCtx* dctx, int param, int value);   /* S/Decompressor.cs:41-46 */
size_t     ZSTD_DCtx_getParameter(ZSTD_DCtx* dctx, int param, int* value);
/* S/Decompressor.cs:36-48 -> U/ZstdDecompress.cs:1909-1931, 1758-1875: raw-content dictionaries (history in front of every
 * frame) and formatted ones (frames start from the dictionary's Huffman/FSE tables and repcodes and must name its dictID or
 * none; a malformed header -> dictionary_corrupted) */
size_t     ZSTD_DCtx_loadDictionary(ZSTD_DCtx* dctx, const void* dict, size_t dictSize);
/* U/ZstdDecompress.cs:2164-2202: decode the next call's frames behind `prefix` as raw-content history (any size, any first bytes).
 * Referenced like ZSTD_CCtx_refPrefix's — a device prefix is read where it lies, no host copy is made — and cancels / is cancelled by
 * ZSTD_DCtx_loadDictionary in the same way.  SINGLE USE: the next ZSTD_decompressDCtx or ZSTDMI_decompressDevice consumes it.  It
 * applies to EVERY frame of that call, as ZSTD_decompress_usingDict does; the reference applies it to the first frame only (a prefix
 * compressor writes one frame, so the two agree on what ZSTD_CCtx_refPrefix produced).  While it is pending, ZSTD_decompressStream,
 * ZSTDMI_decompressBatch, ZSTDMI_decompressRange and a context with several device workers: parameter_unsupported. */
size_t     ZSTD_DCtx_refPrefix(ZSTD_DCtx* dctx, const void* prefix, size_t prefixSize);
/* S/Decompressor.cs:53 -> U/ZstdDecompress.cs:971-993 ; error = (unsigned long long)-2 (S/ThrowHelper.cs:7-8) */
unsigned long long ZSTD_decompressBound(const void* src, size_t srcSize);
unsigned long long ZSTD_getFrameContentSize(const void* src, size_t srcSize);
size_t     ZSTD_findFrameCompressedSize(const void* src, size_t srcSize);
/* S/Decompressor.cs:86 -> U/ZstdDecompress.cs:1365-1368 */
size_t     ZSTD_decompressDCtx(ZSTD_DCtx* dctx, void* dst, size_t dstCapacity, const void* src, size_t srcSize);

/* ---- digested dictionaries: U/ZstdCompress.cs:1700, 5984-6205; U/ZstdDdict.cs:178-279; U/ZstdDecompress.cs:2014-2067, 2300 ----
 * A dictionary digested ONCE and shared: what ZSTD_CCtx_loadDictionary / ZSTD_DCtx_loadDictionary make per context and per load — the
 * upload, the validation of a formatted dictionary, its tables — a ZSTD_CDict / ZSTD_DDict makes at its creation, on a stream of its
 * own, and never writes again.  Any number of contexts and threads may then reference one object at the same time without a lock;
 * referencing it and switching between several touches no device and uploads nothing.  Lifetime is the caller's, as in libzstd: an
 * object must outlive every context that references it, and ZSTD_freeCCtx / ZSTD_freeDCtx never touch it.
 * Not provided: ZSTD_createCDict_byReference / ZSTD_createDDict_byReference (the bytes are always copied), the *_advanced
 * constructors and ZSTD_estimateCDictSize; a DDict set for segmented streams and a DDict set with several device workers.  (The
 * compressor's side of ZSTD_d_refMultipleDDicts, below, is ZSTDMI_compressBatchCDicts: a CDict per entry of a batch.)
 *
 * ZSTD_createCDict: `dict` is host or device memory; the bytes are copied.  compressionLevel 0 means 3 (U/ZstdCompress.cs:5991).  It is
 * created on the device a fresh context binds (ordinal 0; ZSTDMI_createCDictOnDevice for another) and holds there the staged tail, the
 * content with 64 readable bytes behind it, the fast finder's index and the dual finder's two tables over it (what every combination of
 * ZSTDMI_CCtx_setDictIndex / setDictIndexStrategy / setDictIndexChain asks for) and, for a formatted dictionary, DictInfo and the
 * compression tables of ZSTDMI_CCtx_setDictEntropy; it keeps its host bytes.  NULL: without a device, on allocation failure, and for a
 * formatted dictionary whose header is refused (what ZSTD_CCtx_loadDictionary answers with dictionary_corrupted).  Under 8 bytes
 * (NULL/0 included): a CDict that is no dictionary, as in ZSTD_CCtx_loadDictionary. */
ZSTD_CDict* ZSTD_createCDict(const void* dict, size_t dictSize, int compressionLevel);
ZSTD_CDict* ZSTDMI_createCDictOnDevice(const void* dict, size_t dictSize, int compressionLevel, int device);
size_t      ZSTD_freeCDict(ZSTD_CDict* cdict);                               /* NULL is accepted; returns 0 */
size_t      ZSTD_sizeof_CDict(const ZSTD_CDict* cdict);                      /* host + device bytes held; NULL: 0 */
unsigned    ZSTD_getDictID_fromCDict(const ZSTD_CDict* cdict);               /* 0 for raw content and for NULL */
/* Sticky; the CDict is referenced, not copied; the call touches no device.  It cancels a loaded dictionary and a pending
 * ZSTD_CCtx_refPrefix, and is cancelled by ZSTD_CCtx_loadDictionary (NULL included) and by ZSTD_CCtx_refPrefix; cdict = NULL returns
 * to no dictionary; a NULL context: GENERIC; in the middle of a stream session: stage_wrong, as ZSTD_CCtx_loadDictionary.
 * While it is in force the CDict's level stands in for ZSTD_c_compressionLevel in every call that uses the dictionary
 * (U/ZstdCompress.cs:6968; ZSTD_CCtx_getParameter still reports what was set, and it counts again once the reference is gone); every
 * other sticky parameter and every ZSTDMI_CCtx_set* switch applies as with a loaded dictionary, and ZSTD_compressCCtx ignores the
 * reference as it ignores a loaded dictionary.  THE BYTES: every entry point writes exactly what the same context writes after
 * ZSTD_c_compressionLevel = the CDict's level and ZSTD_CCtx_loadDictionary(the same bytes); what is refused with a loaded dictionary
 * (long-distance matching above one block, ZSTDMI_CCtx_setSingleFrame above 64 KiB) stays refused.
 * Where the device copies cannot be shared — a context bound to another device than the CDict's, a context with several device
 * workers — the context makes a private upload from the CDict's host bytes, exactly as after ZSTD_CCtx_loadDictionary: same output,
 * never an error. */
size_t      ZSTD_CCtx_refCDict(ZSTD_CCtx* cctx, const ZSTD_CDict* cdict);
/* U/ZstdCompress.cs:6205: ONE call with the CDict's level and default frame parameters (content size on, checksum off, dictID on); the
 * context's four dictionary switches (ZSTDMI_CCtx_setDictEntropy / setDictIndex / setDictIndexStrategy / setDictIndexChain) apply.  The
 * context's sticky parameters, its dictionary or reference and a pending prefix are left as found.  Host or device buffers, as for
 * ZSTD_compress2.  NULL context or NULL cdict: GENERIC. */
size_t      ZSTD_compress_usingCDict(ZSTD_CCtx* cctx, void* dst, size_t dstCapacity, const void* src, size_t srcSize, const ZSTD_CDict* cdict);
/* ZSTD_createDDict: as ZSTD_createCDict (host or device bytes, copied; device 0 or ZSTDMI_createDDictOnDevice; NULL without a device, on
 * allocation failure and for a formatted dictionary that ZSTD_DCtx_loadDictionary refuses with dictionary_corrupted).  It holds the
 * bytes on the device, DictInfo and, for a formatted dictionary, its literal-length, offset and match-length DECODING tables ready-made
 * in the format the sequence decoder holds per block on chip: a context that references the DDict copies them for every block that
 * repeats the dictionary's tables instead of building them again from their descriptions. */
ZSTD_DDict* ZSTD_createDDict(const void* dict, size_t dictSize);
ZSTD_DDict* ZSTDMI_createDDictOnDevice(const void* dict, size_t dictSize, int device);
size_t      ZSTD_freeDDict(ZSTD_DDict* ddict);                               /* NULL is accepted; returns 0 */
size_t      ZSTD_sizeof_DDict(const ZSTD_DDict* ddict);                      /* host + device bytes held; NULL: 0 */
unsigned    ZSTD_getDictID_fromDDict(const ZSTD_DDict* ddict);               /* 0 for raw content and for NULL */
/* These relate to ZSTD_DCtx_loadDictionary and ZSTD_DCtx_refPrefix as ZSTD_CCtx_refCDict / ZSTD_compress_usingCDict relate to their
 * counterparts: sticky, referenced, no device touched; cancels and is cancelled by the other two; ddict = NULL: no dictionary; NULL
 * context: GENERIC.  Every decode entry point applies a referenced DDict exactly where it applies a loaded dictionary
 * (ZSTD_decompressDCtx, ZSTDMI_decompressDevice, ZSTDMI_decompressBatch, ZSTDMI_decompressRange(s), ZSTD_decompressStream with and
 * without ZSTDMI_DCtx_setStreamSegment): the same bytes and the same error codes, dictionary_wrong for a foreign dictID included.  A
 * context on another device or with several device workers makes a private upload of the DDict's bytes (and builds tables per block).
 * ZSTD_decompress_usingDDict (U/ZstdDecompress.cs:2300) is ONE ZSTD_decompressDCtx with that dictionary; the context's own dictionary
 * or reference and a pending prefix are left as found. */
size_t      ZSTD_DCtx_refDDict(ZSTD_DCtx* dctx, const ZSTD_DDict* ddict);
size_t      ZSTD_decompress_usingDDict(ZSTD_DCtx* dctx, void* dst, size_t dstCapacity, const void* src, size_t srcSize, const ZSTD_DDict* ddict);
/* U/ZstdDecompress.cs:2014-2060.  Host memory in, no device touched.  The dictID a formatted dictionary states (its bytes 4..7), 0 for raw
 * content, NULL and fewer than 8 bytes; the dictID a zstd frame's header names, 0 for a frame without one, a skippable frame, a wrong
 * magic and a header that is not all there. */
unsigned    ZSTD_getDictID_fromDict(const void* dict, size_t dictSize);
unsigned    ZSTD_getDictID_fromFrame(const void* src, size_t srcSize);
/* diagnostics: dictionary uploads this context itself has made since its creation (its device workers' and the private uploads of a
 * CDict / DDict it could not share included: 0 on a context that only ever referenced shareable ones); -1 without a context */
long long   ZSTDMI_debugDictUploads(const ZSTD_CCtx* cctx);
long long   ZSTDMI_debugDictUploadsD(const ZSTD_DCtx* dctx);
/* diagnostic: compressed blocks of the last decode call that took at least one sequence table from a DDict's ready-made set (0 through
 * ZSTD_DCtx_loadDictionary, with a raw-content DDict and where the DDict is not shared); -1 without a context */
long long   ZSTDMI_debugLastDictTableBlocks(const ZSTD_DCtx* dctx);
/* ---- many dictionaries, one context: ZSTD_d_refMultipleDDicts (U/ZstdDecompress.cs:8-115, 343-366, 2300-2339) ----
 * ZSTD_DCtx_setParameter(dctx, ZSTD_d_refMultipleDDicts, v): v = ZSTD_rmd_refSingleDDict (0, the default) or ZSTD_rmd_refMultipleDDicts
 * (1); anything else: parameter_outOfBound.  Sticky; ZSTD_DCtx_getParameter reads it back; neither call touches a device.
 * While it is 1, ZSTD_DCtx_refDDict(dctx, ddict) with a non-NULL DDict makes it the CURRENT DDict, as always, and also files it in
 * the context's SET; a DDict whose dictID the set holds already replaces that entry.  The set is referenced, not copied (lifetime of
 * the DDicts is the caller's, as for one reference), the call touches no device, and the set lives until ZSTD_freeDCtx.  It holds up to
 * 65 536 DDicts; beyond that, and when memory runs out, the call answers memory_allocation and leaves the context as it was.
 * ZSTD_DCtx_refDDict(NULL), ZSTD_DCtx_loadDictionary and ZSTD_DCtx_refPrefix clear the current DDict and leave the set alone.  The set is
 * consulted only while a DDict is current and the parameter is 1; with the parameter back at 0 the context is a single-DDict context
 * with its current DDict.  Raw-content DDicts (dictID 0) are kept in the set (the newest replaces), are never selected by a frame, and
 * serve only as the current DDict.
 * THE RULE, per frame and independent of the frame's neighbours: a frame whose header names a dictID != 0 that is in the set is decoded
 * behind that DDict (content as history, Huffman table, the three sequence tables, ready-made, and repcodes).  Every other frame is
 * treated exactly as the single-DDict decoder treats it with the current DDict: a frame without a dictID uses the current DDict, and a
 * dictID that is not in the set answers dictionary_wrong unless it is the current one's.
 * ONE DIFFERENCE FROM THE REFERENCE: there a selected DDict stays current for the following frames of the call, so a frame without a
 * dictID that follows a frame naming A is decoded behind A.  Here it is decoded behind the DDict of the last ZSTD_DCtx_refDDict: the
 * batch contract (entry i equals the single call on entry i) and the parallel walk both need a rule without order.
 * It applies wherever a referenced DDict applies: ZSTD_decompressDCtx and ZSTDMI_decompressDevice (a concatenation of frames naming
 * different dictionaries), ZSTDMI_decompressBatch (entries it decodes alone afterwards included), ZSTDMI_decompressRange(s), and
 * ZSTD_decompressStream without a stream segment; with every ZSTDMI_DCtx_setLongFrames / setExecWaves / setLiteralDecoder / setOverlap
 * value.  ZSTD_decompress_usingDDict stays ONE call behind that DDict alone: the set is not consulted and is left as found.
 * parameter_unsupported, before a byte is read, while the parameter is 1, a DDict is current, the set holds two or more DDicts, and:
 * the context has several device workers (ZSTDMI_DCtx_setDevices); or a DDict of the set (or the current one) lives on another device
 * than the context; or ZSTDMI_DCtx_setStreamSegment is non-zero in ZSTD_decompressStream.  A set of exactly one DDict takes the
 * single-DDict path in all of these, private upload included.
 * ZSTDMI_debugLastSetFrames: frames of the last decode call whose dictionary was found in the set by dictID (entries and frames the call
 * handed to its own single-call path included; frames of entries that end with a header-stage error are not counted), counted on the
 * device by the frame walk; 0 whenever the single-dictionary kernels ran; -1 without a context. */
long long   ZSTDMI_debugLastSetFrames(const ZSTD_DCtx* dctx);

/* ---- errors: S/ThrowHelper.cs:12-13 -> U/ErrorPrivate.cs:10-24, 35-120 ---- */
unsigned    ZSTD_isError(size_t code);
const char* ZSTD_getErrorName(size_t code);
/* S/ThrowHelper.cs:18-24 (EnsureZdictSuccess) -> U/Zdict.cs:11-19 */
unsigned    ZDICT_isError(size_t code);
const char* ZDICT_getErrorName(size_t code);

/* ---- dictionary training: S/DictBuilder.cs -> U/Zdict.cs, U/Fastcover.cs, U/Cover.cs (dict_train.hip) ----
 * The fastCover trainer on the GPU.  Host pointers in, host dictionary out; the work runs on device 0 (where a fresh ZSTD_CCtx
 * binds) on a stream of the call's own, and everything is freed before return.  Calls from any number of threads are safe and
 * give identical bytes.  The dictionary CONTENT for given (k, d, f, accel, splitPoint) is byte-identical to the reference's.
 * The entropy tables and the k choice are not: their statistics and scores come from this library's compressor (each sample
 * compressed alone against the candidate, in one batch), not from the reference's CPU parser.  Arguments are checked in the reference's order before the device is touched.
 * Refused with parameter_unsupported: f > 24 (every candidate needs its own 2^f-entry u32 frequency copy in HBM), shrinkDict = 1, and
 * training sets above 4 GiB - 8 KiB (positions are 32-bit).
 * nbThreads is accepted and ignored.  Not provided: the COVER (non-fast) trainer, the legacy trainer and
 * ZDICT_addEntropyTablesFromBuffer. */
typedef struct { int compressionLevel; unsigned notificationLevel; unsigned dictID; } ZDICT_params_t;        /* U/ZDICT_params_t.cs */
typedef struct {                                                                                              /* U/ZDICT_cover_params_t.cs */
    unsigned k; unsigned d; unsigned steps; unsigned nbThreads; double splitPoint;
    unsigned shrinkDict; unsigned shrinkDictMaxRegression; ZDICT_params_t zParams;
} ZDICT_cover_params_t;
typedef struct {                                                                                              /* U/ZDICT_fastCover_params_t.cs */
    unsigned k; unsigned d; unsigned f; unsigned steps; unsigned nbThreads; double splitPoint;
    unsigned accel; unsigned shrinkDict; unsigned shrinkDictMaxRegression; ZDICT_params_t zParams;
} ZDICT_fastCover_params_t;
/* U/Zdict.cs:591-600: ZDICT_optimizeTrainFromBuffer_fastCover with d = 8, steps = 4 (k in {50, 537, 1024, 1511, 1998}), f = 20,
 * accel = 1, compressionLevel 3 */
size_t ZDICT_trainFromBuffer(void* dictBuffer, size_t dictBufferCapacity, const void* samplesBuffer, const size_t* samplesSizes,
                             unsigned nbSamples);
/* U/Fastcover.cs:449-505: one (k, d); splitPoint is forced to 1.0 */
size_t ZDICT_trainFromBuffer_fastCover(void* dictBuffer, size_t dictBufferCapacity, const void* samplesBuffer, const size_t* samplesSizes,
                                       unsigned nbSamples, ZDICT_fastCover_params_t parameters);
/* U/Fastcover.cs:525-715: every candidate k (and d = 6 and 8 when d = 0) side by side, the smallest total compressed size of the test
 * samples wins (the first k of equal totals); *parameters receives the chosen ones */
size_t ZDICT_optimizeTrainFromBuffer_fastCover(void* dictBuffer, size_t dictBufferCapacity, const void* samplesBuffer,
                                               const size_t* samplesSizes, unsigned nbSamples, ZDICT_fastCover_params_t* parameters);
/* U/Zdict.cs:458-533: header + entropy tables + content (truncated at its end to fit, padded when under 8 bytes) */
size_t ZDICT_finalizeDictionary(void* dstDictBuffer, size_t maxDictSize, const void* dictContent, size_t dictContentSize,
                                const void* samplesBuffer, const size_t* samplesSizes, unsigned nbSamples, ZDICT_params_t parameters);
unsigned    ZSTD_versionNumber(void);        /* 10501, as U/ZstdCommon.cs:11-21 */
const char* ZSTD_versionString(void);

/* ---- streaming entry points of the safe API (S/Compressor.cs:108-116 <- S/CompressionStream.cs:130-190;
 *      S/Decompressor.cs:97-106 <- S/DecompressionStream.cs:88-162; U/ZstdCompress.cs:6632-6861, U/ZstdDecompress.cs:2816-3205).
 *      Adapters on the batched engine: input is collected on the host and goes through the one-shot
 *      pipeline in batches (compress: 16 MiB or at flush/end; decompress: every whole frame received so far).  endOp is
 *      ZSTD_EndDirective (0 continue, 1 flush, 2 end); return values follow the reference (bytes left to flush / 0 at a
 *      frame boundary / hint), including the hostage-byte rule of U/ZstdDecompress.cs:3170-3194.  Host pointers only. ---- */
typedef struct { const void* src; size_t size; size_t pos; } ZSTD_inBuffer;
typedef struct { void* dst; size_t size; size_t pos; } ZSTD_outBuffer;
size_t ZSTD_compressStream2(ZSTD_CCtx* cctx, ZSTD_outBuffer* output, ZSTD_inBuffer* input, int endOp);
/* frames whose window (or single-segment content size) exceeds 1 << ZSTD_d_windowLogMax (default 27) are refused with
 * frameParameter_windowTooLarge as soon as their header has arrived (U/ZstdDecompress.cs:2965-2969) */
size_t ZSTD_decompressStream(ZSTD_DCtx* dctx, ZSTD_outBuffer* output, ZSTD_inBuffer* input);
/* buffer sizes the stream classes ask for: S/CompressionStream.cs:41 -> U/ZstdCompress.cs:6246-6249; S/DecompressionStream.cs:41 ->
 * U/ZstdCompress.cs:6241-6244; U/ZstdDecompress.cs:2096-2104 */
size_t ZSTD_CStreamInSize(void);
size_t ZSTD_CStreamOutSize(void);
size_t ZSTD_DStreamInSize(void);
size_t ZSTD_DStreamOutSize(void);

/* =====================================================================================================
 * Extensions (not in the reference): device selection, HBM-resident calls, per-stage timing, and test hooks.
 * ===================================================================================================== */
int    ZSTDMI_deviceCount(void);                       /* number of visible MI355X devices; 0 => every call fails loudly */
size_t ZSTDMI_CCtx_setDevice(ZSTD_CCtx* cctx, int device);
size_t ZSTDMI_DCtx_setDevice(ZSTD_DCtx* dctx, int device);
/* Several GPUs behind one context (north_star: "chunks partition naturally across the 8 GPUs of one node"): one device worker per
 * entry of `devices` (an ordinal may be listed more than once).  ZSTD_compress2 / ZSTD_compressCCtx / ZSTD_decompressDCtx and the
 * device-pointer calls then deal the call's frames to the workers in contiguous shares — each stages, compresses or decodes its share on
 * its own device and stream — and copy the results one behind the other into the caller's buffer.  The bytes written do not depend on
 * the number of workers.  n <= 1 returns to a single device.  (The torch.distributed path of bench.py — one process per GPU, RCCL
 * all-gather-v of the shards — is the other way to use a node; this one needs no process group.) */
size_t ZSTDMI_CCtx_setDevices(ZSTD_CCtx* cctx, const int* devices, int n);
size_t ZSTDMI_DCtx_setDevices(ZSTD_DCtx* dctx, const int* devices, int n);
/* run on a caller-owned HIP stream (e.g. torch's current stream); NULL restores the context's own stream */
size_t ZSTDMI_CCtx_setStream(ZSTD_CCtx* cctx, void* hipStream);
size_t ZSTDMI_DCtx_setStream(ZSTD_DCtx* dctx, void* hipStream);

/* inputs larger than one pass are compressed pass by pass (default 16384 chunks = 1 GiB, which bounds the HBM workspace) */
size_t ZSTDMI_CCtx_setPassChunks(ZSTD_CCtx* cctx, unsigned chunksPerPass);

/* Cross-chunk history (the window ZSTD_compress_frameChunk's block loop carries from block to block, U/ZstdCompress.cs:4705-4807,
 * U/ZstdCompressInternal.cs:787-813): historyBytes > 0 makes the blocks 64 KiB - historyBytes long, each matching into the
 * historyBytes of input in front of it, and groups them into multi-block frames of frameBytes of content (0 = keep, default
 * 256 KiB); 0 = independent single-block 64 KiB frames; < 0 = by level (default: 16 KiB at levels 3-4, 32 KiB at levels >= 5,
 * off at levels 1-2 unless ZSTD_c_windowLog > 16 is set).  Ignored while a dictionary is loaded. */
size_t ZSTDMI_CCtx_setHistory(ZSTD_CCtx* cctx, int historyBytes, unsigned frameBytes);

/* parse of chunks that are dense in matches (text, source code, structured data): 0 = region parse (default: after a chunk's
 * first 4 KiB tile found >= 384 matches, the candidates of every later position are looked up first and one lane per 64
 * positions walks them the way ZSTD_compressBlock_fast walks a block, U/ZstdFast.cs:130-260), 1 = the tile loop for every chunk
 * (each 4 KiB tile verified position by position and selected in parallel; slower on dense data, sizes within 0.5 %).
 * Both produce valid, deterministic streams. */
size_t ZSTDMI_CCtx_setParser(ZSTD_CCtx* cctx, unsigned mode);

/* literal (Huffman) decoder: 0 = chosen by frame count (default), 1 = serial, 4 lanes per frame (highest throughput when
 * thousands of frames are in flight), 2 = self-synchronising, 256 lanes per frame (lowest latency per frame),
 * 3 = serial with compact tables (2 KiB + pair table per frame: twice the frames in flight) */
size_t ZSTDMI_DCtx_setLiteralDecoder(ZSTD_DCtx* dctx, unsigned mode);

/* match execution of long frames (the reference's Compressor writes ONE frame per call, U/ZstdCompress.cs:4690-4815): 0 = by cost
 * (default: a frame whose ordered one-wave walk would take longer than a parallel sweep of all such frames is resolved by origin
 * pointers — decode_origin.hip —, the others are walked), 1 = always the walk, 2 = origin pointers for every frame of 1 MiB or more */
size_t ZSTDMI_DCtx_setLongFrames(ZSTD_DCtx* dctx, unsigned mode);
/* the literal decoder beside the sequence decoder on a second stream (they need nothing of each other): 0 = when a call has few
 * blocks (default: neither kernel fills the chip then), 1 = never, 2 = always */
size_t ZSTDMI_DCtx_setOverlap(ZSTD_DCtx* dctx, unsigned mode);
/* waves per frame in the match-execution stage: 0 = by the number of frames in the call (default: few frames get up to 16 waves
 * each — a batch of 64 x waves sequences per round of dependent copies —, more than 2048 frames one wave each), else 1, 2, 4, 8 or 16 */
size_t ZSTDMI_DCtx_setExecWaves(ZSTD_DCtx* dctx, unsigned waves);
/* diagnostic: 1 if the last decompress call listed its frames with the exact serial walk (frames naming a dictionary, frames
 * without a content size, damaged input) instead of the parallel one, 0 if not, -1 without a context */
int ZSTDMI_debugLastWalkSerial(const ZSTD_DCtx* dctx);
/* Offsets of 2^29 and more (what zstd --long=30 / 31 or --patch-from writes for a large file).  The decoder's 8-byte sequence record
 * names 2^29 - 1 bytes of distance; a far-capable frame — content size (without one: its bound) plus the dictionary or prefix content
 * in front of it is 2^29 or more — gets a side plane of 4 bytes per sequence for the rest, and every offset the format can state is
 * decoded: by ZSTD_decompressDCtx, ZSTDMI_decompressDevice, ZSTD_decompress_usingDDict, with a loaded dictionary, a DDict or a
 * referenced prefix, by ZSTD_decompressStream without segments (ZSTD_d_windowLogMax still holds), at every setExecWaves width and on
 * the origin path of frames below 1 GiB (larger frames keep the ordered walk).  An offset beyond position + dictionary in such a
 * frame is corruption_detected; a frame that cannot reach that far keeps frameParameter_windowTooLarge for an offset of 2^29 or
 * more.  A call without a far-capable frame allocates no plane and launches the kernels it always did.  ZSTDMI_decompressBatch (and
 * Async), ZSTDMI_decompressRange(s) (and Async) and a segmented ZSTD_decompressStream (ZSTDMI_DCtx_setStreamSegment) keep the
 * refusal: frameParameter_windowTooLarge for a frame that uses such an offset.
 * diagnostic: 1 if the last single decompress call had a far plane, 0 if not, -1 without a context */
int ZSTDMI_debugLastFarPlane(const ZSTD_DCtx* dctx);

/* same contracts as ZSTD_compress2 / ZSTD_decompressDCtx, but src and dst MUST be device pointers (no staging) */
size_t ZSTDMI_compressDevice(ZSTD_CCtx* cctx, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize);
size_t ZSTDMI_decompressDevice(ZSTD_DCtx* dctx, void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize);

/* Many small buffers in one call: n independent entries, entry i from srcs[i] (srcSizes[i] bytes) to dsts[i] (dstCapacities[i] bytes).
 * The five arrays are host memory; srcs[i] and dsts[i] are device pointers as for ZSTDMI_compressDevice / ZSTDMI_decompressDevice,
 * anywhere in HBM, at any alignment, in any order; destinations must not overlap each other or any source.  Both calls return 0 when
 * they ran (n == 0: at once, without touching the device), or the error of the whole call: init_missing without a device,
 * memory_allocation, GENERIC for a NULL context or a NULL array with n > 0, parameter_unsupported on a context with several device
 * workers (ZSTDMI_*_setDevices).  dstSizes[i] = the bytes written for entry i, or its error (dstSize_tooSmall, corruption_detected
 * ...): size, error code and the bytes at dsts[i] are exactly those of the single device call on that entry alone, on the same
 * context with the same sticky parameters and dictionary — a compressed entry is a complete stream that decodes on its own.  One
 * entry's failure changes nothing of another's, nothing is written at or beyond dsts[i] + dstCapacities[i], and the context is left as
 * it was found.
 * Compress.  Entries of one block (1 byte up to 64 KiB; behind a dictionary 64 KiB minus the dictionary's last 60 KiB rounded up to
 * 4 KiB) — at every level, with or without a dictionary, checksum or content size, LDM enabled or not — share ONE pass through the
 * pipeline per class of resolved parameters (the cParams tiers at 16 KiB, 128 KiB and 256 KiB), ZSTDMI_CCtx_setPassChunks blocks at
 * most: a gather kernel stages them from the pointer array, the kernels of the single call run once over all of them, and a placement
 * kernel sends each result straight to its destination; the sizes come back in one copy per pass.  So do entries of several blocks
 * below 4 MiB, at every level: independent 64 KiB frames (behind a dictionary, or with ZSTDMI_CCtx_setHistory(0)), and multi-block
 * frames whose blocks match into history held on chip — the 64 KiB frames of four 16 KiB blocks that levels 1-2 write for calls up to
 * 32 MiB, and the 48 KiB or 32 KiB blocks in 240-256 KiB frames of the levels >= 3 (or of ZSTDMI_CCtx_setHistory(h > 0) at a level
 * whose finder is the dual-hash or the chain finder), also under ZSTD_c_windowLog >= 16; the kernels then take each block's place in
 * its frame from a per-chunk table.  Everything else — empty entries, LDM above one block, ZSTD_c_windowLog 10 .. 15 above one
 * window, entries of 4 MiB and more (the sparse-input probe decides per call there), entries of more blocks than a pass, and the
 * fast strategy's full 64 KiB blocks with far candidates (levels 1-2 with ZSTDMI_CCtx_setHistory(h > 0) or a window above 2^16) — is
 * handed to the single-call path one entry at a time, after the batched passes, in entry order.
 * Decompress.  One lane per entry walks that entry's frames exactly as the single call's serial walk does (every frame, skippable
 * frames, trailing bytes, a dictID that is not the loaded one); the frames and blocks of all entries then go through the decoder ONCE,
 * with as many host synchronisations as a single call makes.  An entry's error is its first failing block's first error.  Entries
 * that hold a frame without a content size (unless ZSTDMI_DCtx_setBatchUnsized), and entries of more than 4 MiB compressed, are
 * decoded by the single-call path one at a time afterwards. */
size_t ZSTDMI_compressBatch(ZSTD_CCtx* cctx, const void* const* srcs, const size_t* srcSizes, size_t n,
                            void* const* dsts, const size_t* dstCapacities, size_t* dstSizes);
size_t ZSTDMI_decompressBatch(ZSTD_DCtx* dctx, const void* const* srcs, const size_t* srcSizes, size_t n,
                              void* const* dsts, const size_t* dstCapacities, size_t* dstSizes);
/* diagnostics: entries of the last batch call that did NOT take the batched pass (handed to the single-call path); -1 without a context */
int ZSTDMI_debugLastBatchAlone(const ZSTD_CCtx* cctx);
int ZSTDMI_debugLastBatchAloneD(const ZSTD_DCtx* dctx);
/* ---- frames without a content size in the shared pass (what streaming encoders write; ZSTD_c_contentSizeFlag = 0) ----
 * 0 = off (default): an entry holding a frame without a content size is decoded alone, after the shared pass (as before).
 * 1 = such entries take the shared pass.  Sticky; touches no device.  NULL context or mode > 1: parameter_outOfBound
 * (as ZSTDMI_DCtx_setOverlap answers).  Acts on ZSTDMI_decompressBatch and, through their shared core, on ZSTDMI_decompressRange(s).
 * The contract does not change, only the path: dstSizes[i] and the bytes at dsts[i] are what ZSTDMI_decompressDevice gives for the
 * entry alone — the regenerated size when it is at most dstCapacities[i] (which may be far below the frame's bound), dstSize_tooSmall
 * when it is more, a failing block's error in front of dstSize_tooSmall — and nothing is written at or beyond dsts[i] +
 * dstCapacities[i].  An entry's first frame starts at dsts[i] whatever its header says; the frames behind an unsized one are placed
 * per entry, from the regenerated sizes, before any of their bytes is written.  The literal scratch of such an entry is bounded by its
 * capacity, not by its frames' bounds.  Entries of more than 4 MiB compressed still go alone: the alone counters then count only those. */
size_t    ZSTDMI_DCtx_setBatchUnsized(ZSTD_DCtx* dctx, unsigned mode);
/* device bytes the last batch / range(s) call ASKED its work buffers for (frame and block lists, block keys, literal scratch,
 * sequence records): what it requested, not what the context has retained from earlier calls; -1 without a context */
long long ZSTDMI_debugLastBatchWorkspace(const ZSTD_DCtx* dctx);
/* ---- a CDict per entry: many dictionaries, one compress pass (the compressor's side of ZSTD_d_refMultipleDDicts) ----
 * The arrays and pointers are those of ZSTDMI_compressBatch; cdicts is a host array of n entries, cdicts[i] == NULL: entry i has no
 * dictionary.  Per entry, dstSizes[i] (a size or an error code) and the bytes at dsts[i] are exactly what ZSTD_CCtx_refCDict(cctx,
 * cdicts[i]) followed by ZSTDMI_compressBatch on entry i alone gives: the context's sticky parameters and its four dictionary switches
 * (ZSTDMI_CCtx_setDictEntropy / setDictIndex / setDictIndexStrategy / setDictIndexChain) apply, the CDict's level stands in for
 * ZSTD_c_compressionLevel, a NULL entry runs at the context's own level without a dictionary.  The context's own loaded dictionary,
 * CDict reference or set is never consulted, and it and every other state is left as found.  One entry's failure changes nothing of
 * another's.
 * How.  Entries share a pass by what has to be equal for their blocks to share a kernel launch — the block size (behind a staged
 * dictionary tail: 64 KiB minus the tail rounded up to 4 KiB), blocks per frame, indexed or not, and the parameters the CDict's level
 * resolves to — not by the dictionary: a pass behind two or more CDicts uploads one record per CDict and one index per block, and
 * every stage that takes the dictionary as launch constants runs an instance that reads it per block from there.  (Entries of which
 * nothing is staged or indexed — no dictionary, a CDict under 8 bytes — run the plain finder and share passes per CDict.)  A pass
 * behind one CDict launches what ZSTDMI_compressBatch launches.
 * Whole-call answers: n == 0: 0, no device is touched.  A NULL context, or any NULL array (cdicts included) with n > 0: GENERIC.  No
 * device: init_missing.  memory_allocation.  parameter_unsupported, before a byte is read: several device workers, the seek-table
 * switch, a pending ZSTD_CCtx_refPrefix (which stays pending), more than 65536 distinct CDicts (NULL entries are no CDict and do not
 * count), or two or more distinct non-NULL CDicts of which one lives on another device than the context (a single such CDict beside
 * NULL entries is served by the context's private upload of it, as after ZSTD_CCtx_refCDict).  A call whose entries all name one CDict (or all NULL) IS ZSTD_CCtx_refCDict +
 * ZSTDMI_compressBatch — the same kernels, the private upload where the digest cannot be shared — after which the context's own
 * reference is back. */
size_t ZSTDMI_compressBatchCDicts(ZSTD_CCtx* cctx, const void* const* srcs, const size_t* srcSizes, size_t n,
                                  void* const* dsts, const size_t* dstCapacities, size_t* dstSizes,
                                  const ZSTD_CDict* const* cdicts);
long long ZSTDMI_debugLastBatchPasses(const ZSTD_CCtx* cctx);     /* passes through the pipeline the last batch call made (either entry point; entries that went alone are ZSTDMI_debugLastBatchAlone's); -1 without a context */
long long ZSTDMI_debugLastBatchSetChunks(const ZSTD_CCtx* cctx);  /* chunks of the last batch call that ran in set instances; 0 whenever the single-dictionary kernels ran; -1 without a context */
/* ---- a batch enqueued from the device: descriptors in HBM, no host round trip ----
 * ZSTDMI_compressBatch reads its five arrays on the host and waits for the sizes.  These two calls split that: the prepare does
 * everything that needs the host (it may allocate, upload the dictionary and synchronise), the async call only enqueues.
 * ZSTDMI_CCtx_prepareBatchAsync resolves the context's sticky parameters and the dictionary in force (loaded, ZSTD_CCtx_refCDict, the
 * switches ZSTDMI_CCtx_setDictEntropy / setDictIndex / setDictIndexStrategy / setDictIndexChain) as ZSTDMI_compressBatch would for an
 * entry of exactly srcSizeBound bytes, uploads the dictionary, and sizes every workspace a pass of maxEntries blocks needs.  It returns
 * 0, or: GENERIC (NULL context), init_missing, memory_allocation, dictionary_corrupted, the error every single call would answer for
 * the sticky parameters, and parameter_unsupported for what the one-block batched pass does not cover: a bound of 0; a bound that resolves
 * to more than one block or to a multi-block frame (above 64 KiB; behind a staged dictionary tail above 64 KiB minus the tail rounded
 * up to 4 KiB; under ZSTD_c_windowLog 10 .. 15 above one window); several device workers; the seek-table switch; a pending
 * ZSTD_CCtx_refPrefix (which stays pending); maxEntries above the pass limit (ZSTDMI_CCtx_setPassChunks, at most 16384).  A refused or
 * failed prepare leaves the context without a valid one.
 * ZSTDMI_compressBatchAsync: all five arrays and everything they point to are DEVICE memory.  The call makes no device allocation, no
 * host wait, no copy between host and device and no host read of the arrays; it enqueues kernels on the context's stream
 * (ZSTDMI_CCtx_setStream) and returns: 0 once enqueued (n == 0: 0, nothing is touched); GENERIC for a NULL context, or a NULL array with
 * n > 0; stage_wrong if there is no valid prepare, n > maxEntries, or a parameter, dictionary, CDict reference or switch changed since
 * the prepare (any setter invalidates it, whatever value it sets; only a generation counter is compared).  Stage timing
 * (ZSTDMI_CCtx_setProfiling) is off for the length of the call.
 * The arrays, the sources and the destinations must stay valid and unchanged until the stream has passed the work, and so must a
 * referenced CDict; d_dstSizes and the destinations hold their results from then on.  Work is in flight when the call returns: the
 * context waits for it by itself wherever it frees or regrows one of its buffers (ZSTD_freeCCtx, a later call that needs more room,
 * ZSTDMI_CCtx_setStream to another stream, ZSTD_CCtx_loadDictionary, ZSTD_CCtx_refCDict, a dictionary's re-upload); a later call on the
 * same stream is ordered by the stream.  Capturing the call into a hipGraph is neither claimed nor tested.
 * Per entry, d_dstSizes[i] is the compressed size or a zstd error code, with the convention of ZSTDMI_compressBatch: srcSize_wrong when
 * d_srcSizes[i] > srcSizeBound, or when the source is NULL with a non-zero size; dstBuffer_null (capacity > 0) or dstSize_tooSmall
 * (capacity 0) for a NULL destination; dstSize_tooSmall, with nothing written, when the result exceeds the capacity.  A size of 0 writes
 * the empty frame the single call writes under these parameters.  One entry's failure changes nothing of another's.  Nothing is
 * written at or beyond d_dsts[i] + d_dstCapacities[i].
 * Bytes.  Every entry is compressed with the framing and parameters that srcSizeBound resolves to.  Every result is a complete zstd
 * stream that decodes on its own.  For an entry whose own size resolves to the same framing and parameters as the bound, the bytes are
 * exactly those of ZSTDMI_compressBatch.  The level tables change at 16 KiB, 128 KiB and 256 KiB.  A staged dictionary tail changes
 * with the size (up to 60 KiB of it in front of an entry that fits one block behind it, else 32 KiB).  An entry in another tier is
 * valid but may differ from the synchronous call's bytes.  It is the price of the host never seeing a size. */
size_t ZSTDMI_CCtx_prepareBatchAsync(ZSTD_CCtx* cctx, size_t maxEntries, size_t srcSizeBound);
size_t ZSTDMI_compressBatchAsync(ZSTD_CCtx* cctx, const void* const* d_srcs, const size_t* d_srcSizes, size_t n,
                                 void* const* d_dsts, const size_t* d_dstCapacities, size_t* d_dstSizes);
/* ---- entries of several blocks: the second prepare ----
 * ZSTDMI_CCtx_prepareBatchAsyncLimits is the prepare above for a bound of up to 4 MiB - 1, shaped like the decoder's limits; the call
 * itself is ZSTDMI_compressBatchAsync, which serves whichever prepare is valid.  A context holds one prepare; a later one of either
 * kind replaces it.  ZSTDMI_CCtx_prepareBatchAsync keeps its behaviour exactly, its refusal of a bound above one block included.
 * The prepare resolves parameters, dictionary and framing for an entry of exactly srcSizeBound bytes, as ZSTDMI_compressBatch would,
 * and accepts the bound wherever that call would put such an entry into a shared pass: blocks behind LDS history in multi-block frames
 * (16 KiB blocks in 64 KiB frames at levels 1-2, 48 / 32 KiB blocks in frames of 240-256 KiB at levels >= 3,
 * ZSTDMI_CCtx_setHistory(h > 0) above level 2, ZSTD_c_windowLog >= 16), and independent frames behind a dictionary (staged tail, the
 * dictionary index at each of its settings, a referenced CDict, dictionary entropy tables).  A chunk is one block.  The entries of a
 * call are cut into chunks ON THE DEVICE: the host computes every grid from n and the limits, min(maxChunks, n * ceil(srcSizeBound /
 * chunkBytes)) chunk slots, and reads no count back; a slot the call does not fill compresses one idle byte that is placed nowhere.
 * Workspaces are sized for maxChunks chunks (about 200 KiB of device memory each).  A bound that resolves to one block in a
 * single-block frame, with maxChunks 0 or >= maxEntries, gives exactly the state of ZSTDMI_CCtx_prepareBatchAsync (maxChunks =
 * maxEntries) and the call launches what it launches behind that prepare.
 * Returns 0, or: GENERIC (NULL context or limits); parameter_outOfBound for maxEntries 0 or above the pass limit
 * (ZSTDMI_CCtx_setPassChunks, at most 16384), a bound of 0 or >= 4 MiB, maxChunks above the pass limit or (checked behind the framing,
 * so behind the device) below the chunks one entry of the bound needs, a non-zero reserved field; parameter_unsupported for several
 * device workers, the seek-table switch, a pending ZSTD_CCtx_refPrefix (which stays pending) — these, and every out-of-bound answer but the
 * one behind the framing, are given before a device is looked for — and for everything ZSTDMI_compressBatch would compress alone at that size: long-distance matching,
 * ZSTDMI_CCtx_setSingleFrame, ZSTD_c_windowLog 10 .. 15 above one window, the fast strategy's full 64 KiB blocks with far candidates
 * (level 1-2 with ZSTDMI_CCtx_setHistory(h > 0) or ZSTD_c_windowLog > 16), dictionary entropy tables in multi-block frames, more than
 * 256 chunks per entry; and for ZSTDMI_CCtx_setEntropyCarry(1) where it would take effect (multi-block frames without a dictionary:
 * its group count is a host launch argument); else the errors of the first prepare.  A refused prepare leaves the context without one.
 * Per entry, d_dstSizes[i] is as above with this bound, and one answer more, by the decoder's rule: workSpace_tooSmall.  Count the
 * entries that pass their argument checks and are not empty, in entry order: entry i is refused iff the sum of ceil(size / chunkBytes)
 * over those entries up to and including i exceeds maxChunks, so every good entry behind a refused one is refused too; failed and empty
 * entries count for nothing and keep their own answers.  Nothing of a refused entry is written.
 * Bytes: the tier rule above, unchanged.  Every entry is cut with the bound's framing: an entry of 40 KiB under a level-1 bound of
 * 256 KiB becomes three 16 KiB blocks in one frame, not one 40 KiB block.  Valid, decodes on its own, and equal to
 * ZSTDMI_compressBatch's bytes exactly where the entry's own size resolves to the bound's framing and launch parameters.
 * ZSTDMI_CCtx_getBatchAsyncPlan: what the valid prepare (of either kind) resolved, so that a caller can size maxChunks and its
 * destinations: chunkBytes, frameBlocks (0: every chunk a frame of its own) and maxChunks, each through a pointer that may be NULL.
 * Returns 0; GENERIC for a NULL context; stage_wrong without a valid prepare. */
typedef struct {
    size_t maxEntries;    /* entries per call, > 0 */
    size_t srcSizeBound;  /* bytes of one entry, 1 .. 4 MiB - 1 */
    size_t maxChunks;     /* blocks of one call, all entries together; 0 = min(maxEntries * ceil(srcSizeBound / chunkBytes), pass limit) */
    size_t reserved[3];   /* must be 0 */
} ZSTDMI_CBatchLimits;
size_t ZSTDMI_CCtx_prepareBatchAsyncLimits(ZSTD_CCtx* cctx, const ZSTDMI_CBatchLimits* limits);
size_t ZSTDMI_CCtx_getBatchAsyncPlan(const ZSTD_CCtx* cctx, size_t* chunkBytes, size_t* frameBlocks, size_t* maxChunks);
/* diagnostics: blocking waits the compressor's host code has made for this context (stream waits, read-backs, blocking copies, the
 * wait behind an enqueued batch), and growths of its device buffers, since it was created; -1 without a context.  Neither moves
 * across ZSTDMI_compressBatchAsync. */
long long ZSTDMI_debugHostWaits(const ZSTD_CCtx* cctx);
long long ZSTDMI_debugDeviceAllocs(const ZSTD_CCtx* cctx);
/* ---- the decompress counterpart: a batch decoded with no host round trip ----
 * ZSTDMI_decompressBatch stops the host at least three times a call: to size the frame and block lists, to size the sequence records,
 * and to read the answers.  Here the caller states limits ONCE, the prepare sizes every work buffer from them, and the async call only
 * enqueues kernels that take their counts from device memory, over grids sized from the limits.
 * The limits (ZSTDMI_DBatchLimits).  maxEntries, srcSizeBound and maxContent must be stated; the other three have defaults (0), which
 * are conveniences, not measurements:
 *   maxBlocks    = maxFrames + maxContent / 16384 covers every stream THIS library writes (its smallest non-final block is 16 KiB);
 *                  a foreign stream may hold more, smaller blocks;
 *   maxSequences = maxContent / 3 + 64 is exact for valid input — a sequence regenerates at least 3 bytes — and a record costs 8 bytes,
 *                  so a caller who knows the data lowers it.
 * ZSTDMI_batchAsyncWorkspaceD: the device bytes the prepare will ask its work buffers for under these limits (host arithmetic only;
 * 0 for NULL or limits the prepare refuses as out of bound); monotone in every field.
 * ZSTDMI_DCtx_prepareBatchAsync does everything that needs the host: binds the device, uploads and validates the dictionary in force
 * (loaded, ZSTD_DCtx_refDDict, the ZSTD_d_refMultipleDDicts set) and allocates.  It returns 0, or: GENERIC (NULL context or limits);
 * parameter_outOfBound for a zero maxEntries or maxContent, a srcSizeBound of 0 or above 4 MiB, or limits beyond the lists' index range
 * (2^26 frames, 0xFFFFFFF0 blocks); parameter_unsupported for several device workers, a pending ZSTD_DCtx_refPrefix (which stays
 * pending), ZSTDMI_DCtx_setLongFrames(2), and a DDict set that cannot serve a batch; init_missing, memory_allocation,
 * dictionary_corrupted.  Refusals that need no device are answered before one is looked for.  A refused or failed prepare leaves the
 * context without a valid one.
 * ZSTDMI_decompressBatchAsync: all five arrays and everything they point to are DEVICE memory.  The call makes no device allocation, no
 * host wait, no copy between host and device and no host read of the arrays; it enqueues on the context's stream
 * (ZSTDMI_DCtx_setStream) and returns: 0 once enqueued (n == 0: 0, nothing is touched); GENERIC for a NULL context, or a NULL array with
 * n > 0; stage_wrong if there is no valid prepare, n > maxEntries, or a parameter, the dictionary, a DDict reference or the device
 * changed since the prepare (any setter but ZSTDMI_DCtx_setStream invalidates it, whatever value it sets: only a generation counter is
 * compared).  Stage timing (ZSTDMI_DCtx_setProfiling) is off for the length of the call, and ZSTDMI_debugLastBatchAloneD,
 * ZSTDMI_debugLastBatchWorkspace, ZSTDMI_debugLastDictTableBlocks and ZSTDMI_debugLastSetFrames are NOT updated by it.
 * Per entry, d_dstSizes[i] and the bytes at d_dsts[i] are exactly what ZSTDMI_decompressBatch gives on a context with
 * ZSTDMI_DCtx_setBatchUnsized(1), with four exceptions:
 *   1. d_srcSizes[i] > srcSizeBound answers srcSize_wrong — and so does an error code that ZSTDMI_compressBatchAsync left in the column,
 *      which reads as a huge size;
 *   2. an entry refused by a limit answers workSpace_tooSmall, whatever else is wrong with it.  The rule: over the entries that pass the
 *      header walk, in entry order, entry i is refused iff the inclusive sum over the entries 0 .. i of frames, of blocks or of
 *      literal-scratch bytes (a frame's content size; its bound clamped to the capacity for a frame without one) exceeds maxFrames,
 *      maxBlocks or maxContent — so every decodable entry behind a refused one is refused too.  A block whose sequence records would
 *      end beyond maxSequences (counted over the admitted blocks in list order) fails its entry the same way;
 *   3. frames without a content size always take the shared pass (ZSTDMI_DCtx_setBatchUnsized is not consulted);
 *   4. every long frame takes the ordered walk; the origin path (ZSTDMI_DCtx_setLongFrames) is never chosen.  The bytes are the same.
 * One entry's failure changes nothing of another's.  Nothing is written at or beyond d_dsts[i] + d_dstCapacities[i].
 * The arrays, the sources, the destinations and a referenced DDict must stay valid and unchanged until the stream has passed the
 * work.  Work is in flight when the call returns: the context waits for it by itself wherever it frees or regrows one of its buffers
 * (ZSTD_freeDCtx, a later call that needs more room), in ZSTDMI_DCtx_setStream to another stream, ZSTD_DCtx_loadDictionary,
 * ZSTD_DCtx_refDDict, ZSTD_DCtx_refPrefix and a dictionary's or DDict set's re-upload; a later call on the same stream is ordered by
 * the stream.  Capturing the call into a hipGraph is neither claimed nor tested. */
typedef struct {
    size_t maxEntries;     /* entries per call, > 0 */
    size_t srcSizeBound;   /* compressed bytes of one entry, 1 .. 4 MiB */
    size_t maxContent;     /* regenerated bytes of one call, all entries together, > 0: sizes the literal scratch */
    size_t maxFrames;      /* frames of one call; 0 = maxEntries */
    size_t maxBlocks;      /* blocks of one call; 0 = maxFrames + maxContent / 16384 */
    size_t maxSequences;   /* sequence records of one call; 0 = maxContent / 3 + 64 */
} ZSTDMI_DBatchLimits;
size_t ZSTDMI_batchAsyncWorkspaceD(const ZSTDMI_DBatchLimits* limits);
size_t ZSTDMI_DCtx_prepareBatchAsync(ZSTD_DCtx* dctx, const ZSTDMI_DBatchLimits* limits);
size_t ZSTDMI_decompressBatchAsync(ZSTD_DCtx* dctx, const void* const* d_srcs, const size_t* d_srcSizes, size_t n,
                                   void* const* d_dsts, const size_t* d_dstCapacities, size_t* d_dstSizes);
/* diagnostics, as ZSTDMI_debugHostWaits / ZSTDMI_debugDeviceAllocs: blocking waits the decoder's host code has made for this context and
 * growths of its device buffers since it was created; -1 without a context.  Neither moves across ZSTDMI_decompressBatchAsync. */
long long ZSTDMI_debugHostWaitsD(const ZSTD_DCtx* dctx);
long long ZSTDMI_debugDeviceAllocsD(const ZSTD_DCtx* dctx);

/* Packs: n device buffers into ONE contiguous, standard seekable stream whose frames end exactly at the entries' boundaries — the write
 * side of ZSTDMI_decompressRanges.  srcs and srcSizes are host arrays; srcs[i] and d_dst are device pointers as for ZSTDMI_compressBatch,
 * anywhere in HBM, at any alignment; d_dst overlaps no source.
 * The bytes.  For i = 0 .. n - 1 in order, exactly the frames ZSTDMI_compressDevice writes for entry i alone — on the same context with
 * its level, sticky parameters, dictionary, ZSTDMI_CCtx_setDictEntropy / setDictIndex / setSingleFrame and long-distance settings, and
 * with the seek-table switch off; an empty entry is the one empty frame —, one entry's behind the other's without a gap, and behind the
 * last frame ONE seek table in the format described under "Seekable streams" below (8-byte entries, descriptor 0): one entry per frame in
 * stream order, the (Compressed_Size, Decompressed_Size) pairs ZSTDMI_CCtx_setSeekTable(1) lists for each entry alone, one entry's pairs
 * behind the other's.  Frames written with ZSTD_c_contentSizeFlag = 0 have their true content size in the table; an entry above 64 KiB
 * under ZSTDMI_CCtx_setSingleFrame is one frame and one pair.  n == 0 writes the 17-byte empty table.  So `zstd -d` restores the
 * concatenation of the entries, any reader of the seekable format finds the frames, and ZSTDMI_decompressRanges with offsets[i] =
 * srcSizes[0] + .. + srcSizes[i - 1] and lengths[i] = srcSizes[i] returns entry i and decodes that entry's frames alone.
 * The context's own seek-table switch is not consulted, and the call leaves it and every other state of the context as it found it.
 * How.  Entries ZSTDMI_compressBatch would batch (see above) go through its passes in rounds of at most ZSTDMI_CCtx_setPassChunks blocks,
 * into an arena the context owns; the host then knows the round's size, compares it with the capacity that is left, and a gather kernel
 * moves the frames to their place; their table entries are made on the device.  An entry the batch would hand to the single-call path
 * (counted by ZSTDMI_debugLastPackAlone) is written straight to its place in the stream.  Host synchronisations depend on the number of
 * rounds, passes and alone entries, not on n; the device memory held beyond the batch's own is bounded by the round.
 * Returns the bytes written, frames plus table, or ONE error for the whole call: GENERIC for a NULL context or a NULL array with n > 0;
 * init_missing without a device; memory_allocation; parameter_unsupported on a context with several device workers, with a pending
 * ZSTD_CCtx_refPrefix (which stays pending), or when the stream would hold more than 2^27 frames; otherwise the error
 * ZSTDMI_compressDevice gives for the lowest-index entry that fails (srcSize_wrong for a NULL source with a size, a refused parameter,
 * dstBuffer_null ...); dstSize_tooSmall when frames plus table do not fit.  Nothing is ever written at or beyond d_dst + dstCapacity;
 * what lies inside the capacity after an error is unspecified.
 * ZSTDMI_packBound touches no device: the sum of ZSTD_compressBound(srcSizes[i]), + 17, + 8 * the sum of (srcSizes[i] / 4096 + 1) —
 * ZSTDMI_seekTableBound per entry, with one header and footer.  A call with that much room never returns dstSize_tooSmall.  GENERIC
 * for NULL with n > 0; srcSize_wrong when a term or the sum does not fit a size_t. */
size_t ZSTDMI_packBound(const size_t* srcSizes, size_t n);
size_t ZSTDMI_compressPack(ZSTD_CCtx* cctx, void* d_dst, size_t dstCapacity,
                           const void* const* srcs, const size_t* srcSizes, size_t n);
/* diagnostics of the last ZSTDMI_compressPack: entries the single-call path took; entries of the table written; -1 without a context */
int       ZSTDMI_debugLastPackAlone(const ZSTD_CCtx* cctx);
long long ZSTDMI_debugLastPackFrames(const ZSTD_CCtx* cctx);
/* ---- a pack enqueued from the device: a seekable stream with no host round trip ----
 * ZSTDMI_compressPack takes host arrays and stops the host per round.  ZSTDMI_compressPackAsync is the pack for a pipeline whose record
 * lengths were made by a kernel: it serves whichever of ZSTDMI_CCtx_prepareBatchAsync / ZSTDMI_CCtx_prepareBatchAsyncLimits is valid
 * (there is no prepare of its own; their refusals stand, and both size what the pack needs), and the work of one prepare serves
 * ZSTDMI_compressBatchAsync and this call in any order.  The stream is what ZSTDMI_DCtx_prepareRangesAsync / ZSTDMI_decompressRangesAsync read.
 * d_srcs, d_srcSizes, d_packSize, d_entryEnds (may be NULL) and what they point to are DEVICE memory; d_dst is a device pointer at any
 * alignment that overlaps no source; dstCapacity is a host scalar.  The call makes no device allocation, no host wait, no copy between
 * host and device and no host read of the arrays; it enqueues on the context's stream (ZSTDMI_CCtx_setStream) and returns: 0 once
 * enqueued; GENERIC for a NULL context, a NULL d_packSize, or a NULL array with n > 0; dstBuffer_null for a NULL d_dst with a non-zero
 * capacity and dstSize_tooSmall for one with capacity 0 (as ZSTDMI_compressPack); stage_wrong under the conditions of
 * ZSTDMI_compressBatchAsync (no valid prepare, n > maxEntries, anything changed since the prepare).  n == 0 with a valid prepare enqueues
 * the 17-byte empty table and *d_packSize = 17 (dstSize_tooSmall below 17 bytes of capacity).
 * The stream.  For i = 0 .. n - 1 in order, exactly the bytes ZSTDMI_compressBatchAsync writes for entry i under the same prepare (an
 * entry of size 0: the one empty frame), one entry behind the other without a gap; behind the last frame ONE seek table in the format of
 * "Seekable streams" below (8-byte rows, descriptor 0), one row per frame in stream order: (the frame's bytes, its content size) — an
 * empty entry's row is (empty-frame length, 0), and frames written with ZSTD_c_contentSizeFlag = 0 have their true content size there.
 * So a call whose entries all resolve to the bound's framing and parameters (the tier rule above) writes byte for byte what
 * ZSTDMI_compressPack writes for the same entries on a context with the same setup; entries of other tiers give a valid seekable stream
 * that may differ in bytes.  *d_packSize is the bytes written, frames plus table; d_entryEnds[i] the offset in the stream at which entry
 * i's frames end, so entry i occupies [d_entryEnds[i - 1], d_entryEnds[i]) with 0 for d_entryEnds[-1].
 * A pack is one stream, so a failure fails the whole call: *d_packSize is then ONE error code — the answer of the lowest-indexed entry
 * that fails (srcSize_wrong for a size above srcSizeBound or a NULL source with a size; workSpace_tooSmall by the maxChunks rule above),
 * otherwise dstSize_tooSmall when frames plus table exceed dstCapacity — nothing at all is written to [d_dst, d_dst + dstCapacity), and
 * d_entryEnds is not written.  In every case nothing is written outside [d_dst, d_dst + dstCapacity).
 * ZSTDMI_CCtx_packAsyncBound: host arithmetic on the valid prepare, 17 + n * (ZSTD_compressBound(srcSizeBound) + 8 * F), F = the frames
 * one entry of srcSizeBound bytes has under the prepared framing (ceil(chunks / frameBlocks); the chunk count where frameBlocks is 0; at
 * least 1).  A call of n entries with that much room never answers dstSize_tooSmall.  GENERIC for a NULL context, stage_wrong without a
 * valid prepare, srcSize_wrong if the sum overflows; it touches no device.
 * ZSTDMI_debugLastPackAlone / ZSTDMI_debugLastPackFrames are NOT updated; ZSTDMI_debugHostWaits / ZSTDMI_debugDeviceAllocs do not move
 * across the call; stage timing is off for it.  Lifetime: the rules of ZSTDMI_compressBatchAsync (arrays, sources and destination valid
 * and unchanged until the stream has passed the work; the context waits by itself wherever it frees or regrows a buffer).  Capturing the
 * call into a hipGraph is neither claimed nor tested.  Out of scope: packs of more than one pass, appending to a pack. */
size_t ZSTDMI_CCtx_packAsyncBound(const ZSTD_CCtx* cctx, size_t n);
size_t ZSTDMI_compressPackAsync(ZSTD_CCtx* cctx, void* d_dst, size_t dstCapacity,
                                const void* const* d_srcs, const size_t* d_srcSizes, size_t n,
                                size_t* d_packSize, size_t* d_entryEnds /* may be NULL */);

/* Content-defined cuts: frames that end where the CONTENT says, so that the compressed streams of two inputs that differ by an insertion
 * or a deletion share their frames again a few pieces behind the edit (what `zstd --rsyncable` is for: deduplicating and rsync-style
 * stores of compressed data).  Without the switch every frame is cut by position and one inserted byte changes all frames behind it.
 * The cut rule, version 1 — a FORMAT CONTRACT: stores depend on these cut points, a change to it is a new version.
 *   Gear table.  gear[i] = splitmix64(i): z = (i + 1) * 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB; gear[i] = z ^ (z >> 31), all mod 2^64 (the long-distance matcher's table).
 *   Hash.  After byte p of the call's source, h(p) = sum over k = 0 .. min(p, 63) of gear[src[p - k]] << k (mod 2^64):
 *     h = (h << 1) + gear[byte], started at 0 at the source's first byte.  h(p) depends on the last 64 bytes only, never on earlier cuts.
 *   Candidate.  With bits = avgLog - 1, min = 1 << (avgLog - 2) and max = 65536, position p + 1 is a candidate end iff the top `bits`
 *     bits of h(p) are zero.
 *   Selection.  From a piece start s (first s = 0), the piece ends at the smallest candidate e with e - s >= min, if e - s <= max;
 *     otherwise it ends at s + max.  The source's end ends the last piece, whatever its length.  An empty source has no piece.
 *   Range.  avgLog is 12 to 16.
 * ZSTDMI_CCtx_setContentCuts(avgLog): 0 = off (the default), 12 .. 16 = on; 1 .. 11 and above 16: parameter_outOfBound; NULL context:
 * GENERIC.  Sticky; the call touches no device.
 * Where it applies: ZSTD_compress2, ZSTDMI_compressDevice and ZSTD_compress_usingCDict, with host or device buffers.
 * The bytes.  For the pieces 0 .. n - 1 of the rule, in order, the call writes exactly the frames ZSTDMI_compressDevice writes for that
 * piece alone on the same context with the switch off — ZSTDMI_compressPack's contract (above), and its rounds —, one piece's behind the
 * other's without a gap.  With ZSTDMI_CCtx_setSeekTable(1) the pack's ONE seek table follows the last frame: the stream is byte for byte
 * ZSTDMI_compressPack of the pieces.  Without it no table is written (an empty source then writes nothing and returns 0).  Level,
 * dictionary, CDict, ZSTDMI_CCtx_setDictEntropy / setDictIndex* / setEntropyCarry, checksum and content-size flags act per piece as they
 * do in a pack (ZSTD_compress_usingCDict: the CDict's level and default frame parameters, as without the switch).  Every frame depends
 * on its piece's bytes and the context's settings only.  ZSTDMI_debugLastPackAlone / ZSTDMI_debugLastPackFrames speak of a cut call as
 * of a pack.
 * Room.  ZSTDMI_contentCutsBound(srcSize, avgLog) touches no device: with P = srcSize / min + 1 it is
 *     srcSize + (srcSize >> 8) + 64 * P + 17 + 8 * (srcSize / 4096 + P),
 * at least ZSTDMI_packBound of any piece list the rule allows, the seek table included; a call with that much room never answers
 * dstSize_tooSmall.  srcSize_wrong when it does not fit a size_t, parameter_outOfBound for an avgLog outside 12 .. 16.
 * ZSTD_compressBound is too small here (a 1 KiB raw piece costs more than 4 extra bytes).  Nothing is written at or beyond dst + dstCapacity.
 * Refused, never ignored — parameter_unsupported, before a byte is read, while the switch is on: ZSTD_compressStream2;
 * ZSTDMI_compressBatch, ZSTDMI_compressBatchCDicts, ZSTDMI_compressPack and the enqueued calls with their prepares (ZSTDMI_CCtx_prepareBatchAsync /
 * ...Limits, ZSTDMI_compressBatchAsync, ZSTDMI_compressPackAsync: their entries are the caller's cuts); ZSTDMI_debugCompressSamples; and in
 * the calls it applies to: several device workers, a pending ZSTD_CCtx_refPrefix (it stays pending), ZSTDMI_CCtx_setSingleFrame,
 * ZSTD_c_enableLongDistanceMatching = ZSTD_ps_enable, a set ZSTD_c_windowLog of 10 .. 15, srcSize above 2^32 - 1.  ZSTD_compressCCtx
 * ignores the switch, as it ignores the other sticky switches.  ZSTD_c_rsyncable stays parameter_unsupported.  A source whose candidate
 * list does not fit device memory (a hostile input can make it as long as the source) fails with memory_allocation: the list is never thinned.
 * Off (the default, or on and off again): every call launches what it launched before and writes the same bytes.
 * ZSTDMI_contentCuts is the chunker alone: the piece sizes of [d_src, d_src + srcSize) (device memory; host memory is staged) for
 * avgLog, in order, into the HOST array pieceSizes[capacity], their number into *nPieces — also when capacity is too small, which
 * answers dstSize_tooSmall and writes no size (srcSize / min + 1 entries always suffice).  The context's switch is not consulted.
 * GENERIC for a NULL context, a NULL nPieces or a NULL array with a capacity; parameter_outOfBound / parameter_unsupported as above.
 * ZSTDMI_debugLastContentCuts: pieces of the last call that was cut; 0 when none was; -1 without a context.
 * Out of scope: cuts that carry across ZSTD_compressStream2 batches, cuts inside batch or pack entries, pieces above 64 KiB. */
size_t ZSTDMI_CCtx_setContentCuts(ZSTD_CCtx* cctx, unsigned avgLog);
size_t ZSTDMI_contentCutsBound(size_t srcSize, unsigned avgLog);
size_t ZSTDMI_contentCuts(ZSTD_CCtx* cctx, const void* d_src, size_t srcSize, unsigned avgLog,
                          size_t* pieceSizes, size_t capacity, size_t* nPieces);
long long ZSTDMI_debugLastContentCuts(const ZSTD_CCtx* cctx);

/* Piece digests: the step between cutting a device-resident buffer and compressing the pieces a store does not hold yet — the key of
 * every piece, computed where the bytes are.  Two kinds: XXH64 (seed 0), the function of zstd's own frame checksum, as a cheap filter
 * key; SHA-256 (FIPS 180-4), what content-addressed stores key on, as the identity.
 * ZSTDMI_digestSize(kind): 8 for ZSTDMI_digest_xxh64, 32 for ZSTDMI_digest_sha256, 0 for any other kind; touches no device.
 * ZSTDMI_digestPieces.  Piece i is the pieceSizes[i] bytes behind piece i - 1, the first at src.  The sizes' sum may be smaller than
 * srcSize (the frames of a pack without its seek table), never larger; a piece may be empty or as long as the buffer.  src is device
 * memory (host memory is staged, as ZSTDMI_contentCuts stages it) and may be larger than 4 GiB; pieceSizes and digests are HOST arrays.
 * digests receives nPieces * ZSTDMI_digestSize(kind) bytes, piece after piece: XXH64 as the 8 bytes of the value in little-endian order
 * — its first four bytes are exactly the checksum field zstd writes behind a frame of that content —, SHA-256 as the 32 bytes of
 * FIPS 180-4 (hashlib.sha256(piece).digest()).
 * Answers, in this order, all but the last two before a device is looked for: NULL context: GENERIC; NULL pieceSizes or NULL digests
 * with nPieces > 0: GENERIC; a kind other than 1 or 2: parameter_outOfBound; nPieces == 0: 0, nothing touched;
 * digestsCapacity < nPieces * size: dstSize_tooSmall, nothing written; a sum of sizes that overflows or exceeds srcSize: srcSize_wrong;
 * NULL src with srcSize > 0: srcSize_wrong; several device workers (or 2^31 pieces and more): parameter_unsupported; then init_missing /
 * memory_allocation as elsewhere, then 0.
 * ZSTDMI_contentCutsDigests is ZSTDMI_contentCuts(cctx, src, srcSize, avgLog, ...) — its pieces, argument checks and answers — plus the
 * digest of every piece: parameter_outOfBound for the kind comes right behind the one for avgLog; *nPieces is set also when capacity or
 * digestsCapacity is too small, which answers dstSize_tooSmall and writes neither array.  The piece ends never leave the device between
 * the selection and the digest kernel, and the call makes exactly the host waits ZSTDMI_contentCuts makes on the same input.
 * Both calls use the context for its device, stream, workspaces and stage timer only (the digest stage is named digest_xxh64 /
 * digest_sha256 under ZSTDMI_CCtx_setProfiling): they consult and change no sticky parameter, dictionary, CDict reference or
 * content-cuts switch, neither consume nor refuse a pending ZSTD_CCtx_refPrefix, leave a valid ZSTDMI_CCtx_prepareBatchAsync valid and
 * ZSTDMI_debugLastContentCuts as it was.
 * Both functions are serial inside a piece: the call is fast for many pieces and a serial chain for one long piece (README "Piece digests").
 * ZSTDMI_debugDigestModel: one digest of host memory on the CPU, by the same text the kernels run (zmi_digest.h); no device;
 * parameter_outOfBound for a bad kind, GENERIC for a NULL digest or a NULL src with a size.
 * Device-array outputs and an enqueued form: ZSTDMI_contentCutsAsync below.
 * Out of scope: other kinds and keyed hashes, digests computed inside the compress calls. */
enum { ZSTDMI_digest_xxh64 = 1, ZSTDMI_digest_sha256 = 2 };
size_t ZSTDMI_digestSize(unsigned kind);
size_t ZSTDMI_digestPieces(ZSTD_CCtx* cctx, const void* src, size_t srcSize,
                           const size_t* pieceSizes, size_t nPieces, unsigned kind,
                           void* digests, size_t digestsCapacity);
size_t ZSTDMI_contentCutsDigests(ZSTD_CCtx* cctx, const void* src, size_t srcSize, unsigned avgLog, unsigned kind,
                                 size_t* pieceSizes, size_t capacity, size_t* nPieces,
                                 void* digests, size_t digestsCapacity);
size_t ZSTDMI_debugDigestModel(unsigned kind, const void* src, size_t srcSize, void* digest);

/* Cuts and digests enqueued from the device: ZSTDMI_contentCutsDigests (or, with kind 0, ZSTDMI_contentCuts) as an enqueued call in the
 * manner of ZSTDMI_compressBatchAsync — every result in device memory, no allocation, no host wait, no copy between host and device
 * and no host read of any array inside the call.  Its sizes (size_t) and sources (pointers) are the d_srcSizes and d_srcs of
 * ZSTDMI_compressBatchAsync and ZSTDMI_compressPackAsync as they stand.
 * ZSTDMI_CCtx_prepareCutsAsync does everything that needs the host: it allocates one workspace of its own (never the synchronous
 * calls' buffers) for sources up to srcSizeBound bytes cut at avgLog, with digests of `kind` (0: none) and room for maxCandidates
 * candidate ends (0: four times the expected count, 4 * (srcSizeBound >> (avgLog - 1)) + 1024; held to 2^32 - 16).
 * ZSTDMI_cutsAsyncWorkspace(limits): the bytes of that workspace, host arithmetic — with T = ceil(srcSizeBound / 16384), C = the
 * candidate room, P = srcSizeBound / (1 << (avgLog - 2)) + 1, D = ZSTDMI_digestSize(kind), B = ceil((C + 2) / 1024) and r(x) = x rounded
 * up to a multiple of 256:
 *     r(8 (T + 16) + 256) + r(4 C + 64) + 4 r(4 (C + 2)) + r(C + 2) + 2 r(4 (B + 16)) + 256 + r(4 (P + 1)) + r(P D)
 * — or the error the prepare would answer for the same limits before it looks for a device.
 * The prepare consults no sticky parameter, dictionary, CDict or switch.  A context holds one cuts prepare, independent of the batch
 * prepare: each leaves the other valid.  Compression-parameter setters, dictionary calls and the synchronous cut and digest calls leave
 * it valid; a later ZSTDMI_CCtx_prepareCutsAsync replaces it (also when it fails); ZSTDMI_CCtx_setDevice and ZSTDMI_CCtx_setDevices drop it.
 * Answers, all but the last group before a device is looked for: NULL context or NULL limits: GENERIC; srcSizeBound 0 or above 2^32 - 1,
 * avgLog outside 12 .. 16, a kind above 2 or a non-zero reserved field: parameter_outOfBound; several device workers:
 * parameter_unsupported; then init_missing / memory_allocation.
 * ZSTDMI_CCtx_getCutsAsyncPlan: what the prepare resolved (any pointer may be NULL) — maxPieces = P above, the capacity no call on this
 * prepare exceeds; the candidate room; the digest size.  stage_wrong without a prepare.
 * ZSTDMI_contentCutsAsync.  Every d_ argument is device memory; srcSize, capacity (elements of d_pieceSizes and of d_pieceSrcs) and
 * digestsCapacity (bytes) are host scalars.  It enqueues on the context's stream and returns 0, or — nothing enqueued — GENERIC (NULL
 * context, NULL d_nPieces, NULL d_status, NULL d_pieceSizes with a capacity; then, behind stage_wrong, d_digests NULL with a prepared
 * kind or not NULL without one), stage_wrong (no valid prepare), srcSize_wrong (srcSize above the bound, NULL d_src with a size).
 * Device results: *d_status is 0 or one error code (as a size_t, ZSTD_isError's form).  On success *d_nPieces is the number of pieces
 * the rule (version 1) gives for [d_src, d_src + srcSize), d_pieceSizes[i] their sizes in order, d_pieceSrcs[i] = d_src + start_i
 * where that array is given, d_digests their digests in ZSTDMI_digestPieces' byte format.  srcSize == 0: status 0, 0 pieces, no array
 * touched.  More pieces than capacity, or more digest bytes than digestsCapacity: dstSize_tooSmall, *d_nPieces the true count, no array
 * element written.  More candidates than the prepared room: workSpace_tooSmall, *d_nPieces 0, no array element written (prepare with a
 * larger maxCandidates; a list is never thinned).  Nothing is ever written outside the first *d_nPieces elements of each array.
 * ZSTDMI_debugHostWaits and ZSTDMI_debugDeviceAllocs do not move across the call; no stage is timed.  Lifetime: ZSTDMI_compressBatchAsync's
 * rules — the source and every array stay as they are until the stream has passed the work; the context's own buffers are guarded by
 * the same event.  Capture into a hipGraph is neither claimed nor tested.
 * The selection runs across the device (zmi_cut_rank.h): per candidate the candidate its piece would end at, the candidates the walk
 * from position 0 reaches by pointer doubling, every reached candidate's ends at the index a scan gives it.  The synchronous calls keep
 * their single-wave selection.  ZSTDMI_debugCutSelectParallel runs that selection alone over a HOST list of nCand ascending candidate
 * ends of a source of n bytes (synchronous; buffers of its own): *nEnds = the pieces, ends[0 .. *nEnds) their ends when they fit cap,
 * else dstSize_tooSmall; GENERIC for NULL arguments, parameter_outOfBound for avgLog, srcSize_wrong for n above 2^32 - 1 or nCand above n.
 * ZSTDMI_debugCutsAsyncStages runs the stages of one call on the prepared workspace behind events and waits (a measuring hook, not an
 * enqueued call): ms[0] = count and bounded emit, ms[1] = the selection, ms[2] = the digests, in milliseconds; GENERIC for a NULL
 * argument, stage_wrong without a prepare, srcSize_wrong for a size of 0 or above the bound or a NULL source.
 * Out of scope: a device-side entry count for ZSTDMI_compressBatchAsync / ZSTDMI_compressPackAsync (a caller reads the 8-byte count, or
 * filters with a kernel of its own); switching the synchronous calls to the parallel selection; sources above 2^32 - 1; thinning of
 * hostile candidate lists; balancing of uneven pieces in the digest kernels. */
typedef struct {
    size_t   srcSizeBound;   /* bytes of one call's source, 1 .. 2^32 - 1 */
    unsigned avgLog;         /* 12 .. 16 */
    unsigned kind;           /* 0 = no digests, ZSTDMI_digest_xxh64, ZSTDMI_digest_sha256 */
    size_t   maxCandidates;  /* 0 = 4 * (srcSizeBound >> (avgLog - 1)) + 1024 */
    size_t   reserved[3];    /* must be 0 */
} ZSTDMI_CutLimits;
size_t ZSTDMI_cutsAsyncWorkspace(const ZSTDMI_CutLimits* limits);
size_t ZSTDMI_CCtx_prepareCutsAsync(ZSTD_CCtx* cctx, const ZSTDMI_CutLimits* limits);
size_t ZSTDMI_CCtx_getCutsAsyncPlan(const ZSTD_CCtx* cctx, size_t* maxPieces, size_t* maxCandidates, size_t* digestSize);
size_t ZSTDMI_contentCutsAsync(ZSTD_CCtx* cctx, const void* d_src, size_t srcSize,
                               size_t* d_pieceSizes, const void** d_pieceSrcs, size_t capacity,
                               void* d_digests, size_t digestsCapacity,
                               size_t* d_nPieces, size_t* d_status);
size_t ZSTDMI_debugCutSelectParallel(ZSTD_CCtx* cctx, const unsigned* cands, size_t nCand, unsigned long long n, unsigned avgLog,
                                     unsigned* ends, size_t cap, size_t* nEnds);
size_t ZSTDMI_debugCutsAsyncStages(ZSTD_CCtx* cctx, const void* d_src, size_t srcSize, float* ms);

/* Seekable streams (the zstd seekable format, v0.1.0): random access at the granularity of the frame.
 * Every stream this library writes is a run of independent frames (64 KiB of content at levels 1-2, 240-256 KiB at levels >= 3, 32 KiB
 * or less behind a dictionary, one window under long-distance matching; ZSTDMI_CCtx_setHistory and ZSTD_c_windowLog change it).
 * ZSTDMI_CCtx_setSeekTable(1) makes ZSTD_compress2 and ZSTDMI_compressDevice append a seek table to exactly those bytes — a skippable
 * frame, so every zstd decoder still reads the stream; all fields little-endian:
 *     0x184D2A5E (4) | Frame_Size (4) | N entries | Number_Of_Frames (4) | descriptor (1) | 0x8F92EAB1 (4)
 *     entry: Compressed_Size (4) | Decompressed_Size (4) | [Checksum (4), only if the descriptor's bit 7 is set]
 * one entry per frame in order (a skippable frame: Decompressed_Size 0).  This library writes 8-byte entries, descriptor 0: table
 * checksums are neither written nor verified (the frames' own checksums, ZSTD_c_checksumFlag, still are).  0 = off (default); any
 * other mode: parameter_outOfBound.  The table needs ZSTDMI_seekTableBound(srcSize) bytes on top of ZSTD_compressBound(srcSize); if it
 * does not fit behind the frames the call returns dstSize_tooSmall.  With the switch on, ZSTDMI_compressBatch, ZSTD_compressStream2 and
 * a context with several device workers return parameter_unsupported (many buffers into one seekable stream: ZSTDMI_compressPack
 * above); ZSTD_compressCCtx ignores it (level-only parameters).
 * ZSTDMI_decompressRange writes content[offset, offset + length) of a stream that ends in such a table (this library's or anyone's,
 * 8- or 12-byte entries) to dst and returns the bytes written, min(length, max(total - offset, 0)); more than dstCapacity:
 * dstSize_tooSmall, nothing written.  src and dst are host or device pointers, each on its own.  Only the frames that meet the range
 * are decoded — a 1-byte read decodes one whole frame — and from a host source only the table and those frames' compressed bytes are
 * copied to the device.  The context's dictionary applies; several device workers: parameter_unsupported.  Table errors: a stream below
 * 17 bytes, a wrong footer magic, a skippable header that is missing, not ...5E, or of another size: prefix_unknown; reserved descriptor
 * bits, more than 2^27 entries, a table longer than the stream, compressed sizes that do not add up to the bytes in front of the table,
 * a frame whose content is not the size its entry names: corruption_detected. */
size_t ZSTDMI_CCtx_setSeekTable(ZSTD_CCtx* cctx, unsigned mode);
/* Code with a formatted dictionary's entropy tables (ZSTD_loadCEntropy, U/ZstdCompress.cs:5259-5400).  0 = off (the default: no
 * existing output changes; making it the default is a separate, later decision), 1 = on, any other mode: parameter_outOfBound; NULL
 * context: GENERIC.  Sticky; the call touches no device.  On, and with a FORMATTED dictionary in use, the first block of every frame
 * (behind a dictionary a frame has one block) has the dictionary's Huffman table and its three FSE tables as its previous entropy
 * state, decided as the reference decides below the lazy strategy: a treeless literals section (type 3) where the table covers the
 * literals and a tree of the block's own would not pay for its description — always up to 1024 literals; raw only up to 6 literals
 * and one stream up to 1023 when the table has no zero weight — and set_repeat (mode 3, no table description) for LL / OF / ML where
 * the dictionary's table is valid for the alphabet, defaults are allowed and the block has fewer than 1000 sequences.  Later blocks
 * of a frame describe their own tables as ever.  A Huffman table of fewer than 256 symbols or with codes above 11 bits is not used.
 * Honoured by ZSTD_compress2, ZSTDMI_compressDevice, ZSTDMI_compressBatch (bytes equal to the single call), ZSTD_compressStream2,
 * ZSTDMI_debugCompressSamples and contexts with several device workers.  Without a dictionary, with a raw-content dictionary, behind
 * ZSTD_CCtx_refPrefix and in ZSTD_compressCCtx the switch changes nothing.  Every zstd decoder holding the dictionary reads the frames. */
size_t ZSTDMI_CCtx_setDictEntropy(ZSTD_CCtx* cctx, unsigned mode);
/* Carry entropy tables and repcodes from block to block inside a frame.  0 = off (the default: a context that never turns the switch
 * on launches the kernels it launched and writes the bytes it wrote), 1 = on, any other mode: parameter_outOfBound; NULL context:
 * GENERIC.  Sticky; the call touches no device.  On, the blocks of a multi-block frame are coded in order inside carry groups: 8
 * consecutive blocks of one frame, aligned to multiples of 8 of the block's index in its frame (under ZSTDMI_CCtx_setSingleFrame: of
 * its place in the one frame; a stream batch ends a group where the batch ends).  Behind a group's first block a block may write
 * treeless literals (type 3) with the Huffman table of the latest block of the group that ended as a compressed block with a
 * Compressed_Literals section — taken when it has a code for every literal that occurs and the section is no larger than the block's
 * own; repeat mode (3) for each of LL / OF / ML where the block before described or repeated that table, every code of the block has
 * a probability in it and it costs no more bits than the description plus the block's own table would; and repcodes seeded with what
 * the block before left (a raw block leaves the decoder's history, its Huffman table and the tables it would have repeated as they
 * were; the tables it would have described are not repeated behind it).  A group's first block writes neither type 3 nor mode 3, and
 * starts from unknown repcodes unless it is the frame's first block.
 * Honoured by ZSTD_compress2, ZSTDMI_compressDevice, ZSTDMI_compressBatch (bytes equal to the single call), ZSTDMI_compressPack,
 * ZSTD_compressStream2, contexts with several device workers, the seek-table switch, long-distance matching, the long form of
 * ZSTD_CCtx_refPrefix and ZSTDMI_CCtx_setSingleFrame (the bytes of a one-shot call do not depend on ZSTDMI_CCtx_setPassChunks).
 * It changes nothing, byte for byte, where every block is a frame of its own (levels 1-2 at their default framing above 32 MiB,
 * inputs of one block), under ZSTD_c_windowLog 10 .. 15, behind a loaded dictionary or a CDict (ZSTDMI_compressBatchCDicts included),
 * in ZSTD_compressCCtx, in ZSTDMI_debugCompressSamples and the dictionary trainer.  Every zstd decoder reads the frames.
 * ZSTDMI_debugLastCarryGroups: carry groups the last call walked (over all its passes and device workers); 0 when the switch took no
 * effect; -1 without a context. */
size_t ZSTDMI_CCtx_setEntropyCarry(ZSTD_CCtx* cctx, unsigned mode);
long long ZSTDMI_debugLastCarryGroups(const ZSTD_CCtx* cctx);
/* Index a dictionary once, when it is uploaded, and match against ALL of it (the reference digests a dictionary once, ZSTD_createCDict /
 * ZSTD_loadDictionaryContent, and probes its table beside the block's own, ZSTD_compressBlock_fast_dictMatchState).  0 = off (the
 * default: no existing output changes), 1 = on, any other mode: parameter_outOfBound; NULL context: GENERIC.  Sticky; the call touches
 * no device; before or after ZSTD_CCtx_loadDictionary, a loaded dictionary is uploaded again by the next call that uses it.
 * On, with a dictionary of at least 8 bytes in use and the fast strategy resolved (levels <= 2, negative levels, ZSTD_c_strategy = 1):
 * the last min(content size, 188 KiB) bytes of the dictionary's content stay on the device behind a hash index built once per upload
 * and per device worker; no dictionary byte is staged or hashed per chunk; every position the finder probes also looks one candidate
 * up in that index.  A source of up to 64 KiB is one block in one single-segment frame (without the switch: 64 KiB minus the staged
 * dictionary tail, 4 KiB behind 60 KiB of it); larger sources are independent 64 KiB frames, each behind the dictionary.  A match
 * into the dictionary ends with the dictionary.  DictID, content size, checksum, ZSTD_c_dictIDFlag and the dictionary's repcodes are
 * as without the switch, and ZSTDMI_CCtx_setDictEntropy composes with it.  Honoured by ZSTD_compress2, ZSTDMI_compressDevice,
 * ZSTDMI_compressBatch (bytes equal to the single call; entries up to 64 KiB are one block), ZSTD_compressStream2,
 * ZSTDMI_debugCompressSamples and contexts with several device workers.  The switch changes nothing without a dictionary, at levels
 * whose finder is not the fast one (>= 3; ZSTDMI_CCtx_setDictIndexStrategy below extends it to levels 3-4), under ZSTD_c_windowLog 10 .. 15, behind ZSTD_CCtx_refPrefix and in ZSTD_compressCCtx; what
 * a dictionary is refused with (long-distance matching above one block, ZSTDMI_CCtx_setSingleFrame) stays refused.  Dictionary
 * content in front of its last 188 KiB is not matched against.  Every zstd decoder holding the dictionary reads the frames. */
size_t ZSTDMI_CCtx_setDictIndex(ZSTD_CCtx* cctx, unsigned mode);
/* The highest strategy at which an index that is switched on (ZSTDMI_CCtx_setDictIndex(1)) is used.
 * 1 = fast only (the default: exactly what ZSTDMI_CCtx_setDictIndex describes above); 2 = also doubleFast (level 3, the default
 * level, and level 4: wherever the call resolves to the dual-hash finder).  Sticky; touches no device.  NULL: GENERIC.  0 or above 2:
 * parameter_outOfBound (the chain finder of the levels >= 5 has a switch of its own, ZSTDMI_CCtx_setDictIndexChain below; this
 * setting keeps refusing 3 and above).
 * With the index off the setting changes nothing.  With it on, a change of the setting has a loaded dictionary uploaded again by
 * the next call that uses it; ZSTD_CCtx_loadDictionary, ZSTDMI_CCtx_setDictIndex and this call may come in any order, and the level
 * or ZSTD_c_strategy may change between calls without another load.  At 2 an upload builds three tables over the same bytes (the
 * fast finder's, and one per hash of the dual finder: at most 1 MiB each); a position the dual finder probes looks up one candidate
 * in each of its two, behind its four candidates in the block, and a dictionary candidate has to be longer to win.  Framing, entry
 * points, what stays unchanged (now: levels >= 5) and the refusals are those of ZSTDMI_CCtx_setDictIndex. */
size_t ZSTDMI_CCtx_setDictIndexStrategy(ZSTD_CCtx* cctx, unsigned maxStrategy);
/* The index for the chain finder: levels >= 5 and ZSTD_c_strategy >= 3.  0 = off (the default), 1 = on, any other mode:
 * parameter_outOfBound; NULL context: GENERIC.  Sticky; touches no device; any order relative to ZSTD_CCtx_loadDictionary,
 * ZSTDMI_CCtx_setDictIndex and ZSTDMI_CCtx_setDictIndexStrategy, of whose value it is independent (that setting reaches strategy 2,
 * this switch covers what lies above).  While the index is on, a change has a loaded dictionary uploaded again by the next call that
 * uses it; an upload then builds the same three tables as ZSTDMI_CCtx_setDictIndexStrategy(2), so the level may change between calls
 * without another load.  It takes effect where ZSTDMI_CCtx_setDictIndex(1) is set, a dictionary of at least 8 bytes is in use and the
 * call resolves to the chain finder: nothing of the dictionary is staged or linked into hash chains per chunk, a source of up to
 * 64 KiB is one block in one single-segment frame (without it: 64 KiB minus the staged tail), larger sources are independent 64 KiB
 * frames, and every position looks up, behind its walk down the block's chains, one candidate per hash (5 and 8 bytes) anywhere in the
 * dictionary's last 188 KiB; a dictionary candidate has to be longer than the block's best to win, and a match into the dictionary ends
 * with it.  There are no chains inside the dictionary: one candidate per hash, where the staged tail offered a chain's depth of them.
 * Header fields, dictID, repcodes, checksum, ZSTDMI_CCtx_setDictEntropy, the entry points, ZSTD_c_windowLog 10 .. 15 and the refusals
 * are those of ZSTDMI_CCtx_setDictIndex. */
size_t ZSTDMI_CCtx_setDictIndexChain(ZSTD_CCtx* cctx, unsigned mode);
/* (debug) chunks that the last pass launched by the last compress call handed to the region parse's kernel of its own (the fast
 * finder's on plain chunks, the chain finder's): 0 when it did not run, -1 without a context */
long long ZSTDMI_debugLastRegionChunks(const ZSTD_CCtx* cctx);
/* (debug) dictionary content bytes the index covers: 0 with the switch off, without a dictionary, or for a formatted dictionary no
 * call has validated on a device yet; -1 without a context */
long long ZSTDMI_debugDictIndexed(const ZSTD_CCtx* cctx);
/* One frame per call and per stream session, as the reference writes it (S/Compressor.cs Wrap, S/CompressionStream.cs).  0 = off (the
 * default: a run of independent frames, every existing output unchanged), 1 = on, any other mode: parameter_outOfBound; NULL context:
 * GENERIC.  Sticky; the call touches no device.
 * On, ZSTD_compress2 and ZSTDMI_compressDevice write a source of more than 64 KiB as exactly ONE frame: the blocks of the long-distance
 * framing for the level (full 64 KiB blocks with far candidates at the fast strategy, 48 / 32 KiB blocks behind LDS history above it)
 * without its stage, every block but the first behind the input in front of it, also across the passes of ZSTDMI_CCtx_setPassChunks —
 * the bytes depend on the input and the parameters alone.  Header: with wl = ZSTD_c_windowLog or else the level's windowLog for the
 * source size, a single segment with the content size when srcSize <= 2^wl, otherwise a window descriptor for 2^wl AND the content
 * size; ZSTD_c_contentSizeFlag = 0: a window descriptor alone.  Last_Block on the last block only; with ZSTD_c_checksumFlag the XXH64
 * of the whole content behind it (a serial chain over the input: see README "One frame per call").  Sources of at most 64 KiB, the
 * empty one included: the bytes of the switch off.  The sparse-input probe is honoured when it finds one kind of data in the whole
 * call; a mixed input is not cut into ranges and takes the level's own path as a whole.
 * ZSTD_compressStream2 writes one frame per session: a window descriptor for the level's default windowLog (or ZSTD_c_windowLog), no
 * content size; ZSTD_e_flush ends a block, ZSTD_e_end sets Last_Block (on an empty block when nothing is buffered) and appends the
 * checksum.  ZSTDMI_compressBatch: bytes equal to the single call; entries above 64 KiB go through the single-call path.
 * ZSTD_compressCCtx ignores the switch; behind ZSTD_CCtx_refPrefix, and under long-distance matching when the source fits one of
 * its frames, the output is one frame already and does not change.
 * parameter_unsupported at the consuming call, with the context left usable: a source above 2 GiB; ZSTD_c_windowLog 10 .. 17; a seek
 * table; several device workers; a loaded dictionary (sources above 64 KiB, and every stream session); long-distance matching with a
 * source of more than one of its frames (and in every stream session).
 * The trade: one long frame decodes at the long-frame rate (ZSTDMI_DCtx_setLongFrames; this library's decoder walks a frame of 1 GiB
 * or more in order), not at that of independent frames, cannot be sharded by frame, and its checksum is one serial chain (seconds per
 * GiB on both sides).  Figures: README "One frame per call". */
size_t ZSTDMI_CCtx_setSingleFrame(ZSTD_CCtx* cctx, unsigned mode);
/* Long-distance matching whose window slides with the one frame (the reference's ZSTD_ldm_* under `zstd --long`).  0 = off (the
 * default), 1 = on, any other mode: parameter_outOfBound; NULL context: GENERIC.  Sticky; the call touches no device.
 * It takes effect only with ZSTDMI_CCtx_setSingleFrame on AND ZSTD_c_enableLongDistanceMatching = ZSTD_ps_enable, in exactly the
 * calls that combination is refused in without it: every ZSTD_compressStream2 session, and a ZSTD_compress2 / ZSTDMI_compressDevice
 * whose source exceeds one long-distance frame (min(2^windowLog, 512 MiB, one pass)).  Everywhere else — a source that fits one
 * long-distance frame, ZSTD_ps_auto / ZSTD_ps_disable, single-frame off, ZSTD_compressCCtx, a pending ZSTD_CCtx_refPrefix — the
 * bytes are those of the switch off.
 * In effect: ONE frame of the single-frame blocks for the level (64 / 48 / 32 KiB), found by the same block finders, and the
 * long-distance stage adds matches at any distance up to 2^wl in front of a position, wherever a pass or a stream batch begins; wl =
 * ZSTD_c_windowLog, or 27; the stage's other parameters follow from wl as they do for aligned windows.  No offset exceeds 2^wl.
 * Header: the single-frame rules with that wl (a call: a single segment when srcSize <= 2^wl, else a window descriptor for 2^wl and
 * the content size; a stream: the descriptor alone).  The stage runs once per pass (per batch of a stream: 16 MiB, or what a flush or
 * the end finds buffered) over the up to 2^wl bytes of the frame in front of the pass — indexed, not matched again — and the pass.
 * A call reads them in place in its own source; a session keeps them on the device: it holds 2^wl bytes + one batch + 4 MiB there from
 * its first batch to its end.  The same input, parameters, pass size and flush positions give the same bytes; other than plain
 * single-frame output, the bytes MAY change with ZSTDMI_CCtx_setPassChunks and with where batches end (a step's index is its window's).
 * parameter_unsupported at the consuming call: ZSTD_c_windowLog 29 .. 31 (with ZSTDMI_CCtx_setFarOffsets on: 31 alone), and what
 * ZSTDMI_CCtx_setSingleFrame refuses otherwise.  ZSTDMI_compressBatch / ZSTDMI_compressPack: such an entry goes through the single-call
 * path.  Cost: every step indexes its window again ((2^wl + n) of stage work for n bytes).  Figures: README "Sliding long-distance window". */
size_t ZSTDMI_CCtx_setSlidingLdm(ZSTD_CCtx* cctx, unsigned mode);
/* Offsets of 2^29 and more on the compress side: delta frames beyond 512 MiB.  0 = off (the default), 1 = on, any other mode:
 * parameter_outOfBound; NULL context: GENERIC.  Sticky; the call touches no device; device workers take it with the call's parameters.
 * Off: every byte and every refusal is what it always was.  On:
 *   - the long form of ZSTD_CCtx_refPrefix accepts prefixSize + srcSize up to 2^31 (the prefix stays at most 1 GiB, the source at most
 *     one pass); its window is ceil_log2(prefixSize + srcSize), up to 31;
 *   - ZSTDMI_CCtx_setSlidingLdm accepts ZSTD_c_windowLog 29 and 30 (a pass is held to 2^31 bytes, so that window + pass stay inside the
 *     long-distance stage's 32-bit pass coordinate); 31 stays refused.
 * Aligned long-distance frames keep their 512 MiB cap in either mode, and a call that the switch does not touch writes the bytes of
 * the switch off.  Such frames state offset codes 29 and 30, for which the format has no predefined table: their offset table is
 * always described or RLE.  They decode with this library's single calls (ZSTDMI_debugLastFarPlane), with the oracle and with libzstd;
 * ZSTDMI_decompressBatch, the range calls and a segmented stream refuse them (frameParameter_windowTooLarge). */
size_t ZSTDMI_CCtx_setFarOffsets(ZSTD_CCtx* cctx, unsigned mode);
size_t ZSTDMI_seekTableBound(size_t srcSize);
size_t ZSTDMI_decompressRange(ZSTD_DCtx* dctx, void* dst, size_t dstCapacity, const void* src, size_t srcSize,
                              unsigned long long offset, size_t length);
/* diagnostics of the last ZSTDMI_decompressRange: table entries with content it decoded; bytes it copied host -> device (0 for a
 * device source); -1 without a context */
int ZSTDMI_debugLastRangeFrames(const ZSTD_DCtx* dctx);
long long ZSTDMI_debugLastRangeStaged(const ZSTD_DCtx* dctx);

/* Gather reads: n ranges of ONE seekable stream in one call.  src (host or device memory, as for ZSTDMI_decompressRange) ends in a
 * seek table; the five arrays are host memory; dsts[i] are device pointers anywhere, at any alignment and in any order, that overlap
 * neither each other nor the source (the batch's convention).  Returns 0 when the call ran (n == 0: 0, without touching the device);
 * GENERIC for a NULL context or a NULL array with n > 0, parameter_unsupported on a context with several device workers or a pending
 * ZSTD_DCtx_refPrefix, memory_allocation for n above 0xFFFFFFF0 or when the arena cannot be had, and a table error (the prefix_unknown
 * and corruption_detected cases of ZSTDMI_decompressRange, same codes) before anything is decoded.  The context's dictionary applies.
 * dstSizes[i] is exactly what ZSTDMI_decompressRange(dctx, dsts[i], dstCapacities[i], src, srcSize, offsets[i], lengths[i]) returns
 * on the same context, and the bytes at dsts[i] are the same: min(length, max(total - offset, 0)) bytes; 0 for a range past the end
 * or of length 0 (dsts[i] may then be NULL); dstSize_tooSmall, nothing written, for more than dstCapacities[i].  Ranges may overlap,
 * repeat and come in any order: every table entry with content that some served range meets is decoded ONCE, into an arena the context
 * owns, and a gather kernel hands each range its bytes.  A frame that fails — a decode error, or a content size other than its
 * entry's: corruption_detected — fails every range that meets it, with the code the single call gives; a failed range writes nothing
 * and changes nothing of the ranges that do not meet the frame.  Nothing is ever written outside [dsts[i], dsts[i] + dstSizes[i]).
 * From a host source only the table and the touched frames' compressed bytes are copied to the device, packed into one buffer.  The
 * number of host synchronisations does not depend on n.  A range of more than 4 MiB is not gathered: it is handed to the single-range
 * path after the gathered pass, in range order (its frames are decoded straight to their place).  A frame of more than 4 MiB
 * compressed, or without a content size, is decoded by the single-call path into the arena and does not make its ranges go alone. */
size_t ZSTDMI_decompressRanges(ZSTD_DCtx* dctx, const void* src, size_t srcSize,
                               const unsigned long long* offsets, const size_t* lengths, size_t n,
                               void* const* dsts, const size_t* dstCapacities, size_t* dstSizes);
/* diagnostics of the last ZSTDMI_decompressRanges: DISTINCT table entries with content the gathered pass decoded; ranges handed to the
 * single-range path; bytes copied host -> device (0 for a device source); -1 without a context */
int ZSTDMI_debugLastRangesFrames(const ZSTD_DCtx* dctx);
int ZSTDMI_debugLastRangesAlone(const ZSTD_DCtx* dctx);
long long ZSTDMI_debugLastRangesStaged(const ZSTD_DCtx* dctx);

/* ---- gather reads enqueued from the device: ZSTDMI_decompressRanges with no host round trip ----
 * ZSTDMI_decompressRanges stops the host at least three times a call (the table's footer, the plan's summary that sizes the arena, the
 * answers), takes its five arrays as host memory and indexes the whole seek table again on every call.  Here ONE seekable stream in
 * device memory is prepared once — footer read, table indexed and validated, every work buffer sized from limits — and a call only
 * enqueues kernels over the caller's device arrays.
 * The limits (ZSTDMI_DRangesLimits).  maxRanges, maxRangeBytes and maxContent must be stated; the other three have defaults (0):
 * maxFrames = the table's entry count N, and maxBlocks / maxSequences as for ZSTDMI_DBatchLimits above, with the same caveats.
 * ZSTDMI_rangesAsyncWorkspaceD: the device bytes the prepare will ask its buffers for under these limits and a table of tableEntries
 * entries (host arithmetic only; 0 for NULL or what the prepare refuses as out of bound); monotone in every field and in tableEntries.
 * ZSTDMI_DCtx_prepareRangesAsync(dctx, d_src, srcSize, limits) does everything that needs the host, once: binds the device, uploads
 * and validates the dictionary in force (loaded, ZSTD_DCtx_refDDict, the ZSTD_d_refMultipleDDicts set), reads the 9-byte footer, indexes
 * the table into buffers of its own — a synchronous ZSTDMI_decompressRange[s] on the same context between async calls neither disturbs
 * nor invalidates the prepared index —, reads the index's summary back and allocates.  It returns 0, or: GENERIC (NULL context or
 * limits); parameter_outOfBound for a zero maxRanges or maxContent, a maxRangeBytes of 0 or above 4 MiB, or limits beyond the lists'
 * index range (those of ZSTDMI_DCtx_prepareBatchAsync; with maxFrames 0, N counts); parameter_unsupported for a host d_src, several
 * device workers, a pending ZSTD_DCtx_refPrefix (which stays pending), ZSTDMI_DCtx_setLongFrames(2) and a DDict set that cannot serve
 * a batch; the table's error with the code ZSTDMI_decompressRanges gives for the same stream (no footer magic or a wrong skippable
 * header: prefix_unknown; reserved descriptor bits, more than 2^27 entries or sizes that do not add up: corruption_detected);
 * init_missing, memory_allocation, dictionary_corrupted.  Refusals that need no device are answered before one is looked for.
 * A context holds ONE async prepare of either kind: this one and ZSTDMI_DCtx_prepareBatchAsync replace each other, and the call whose
 * prepare was replaced answers stage_wrong.  A refused or failed prepare leaves none.  The stream's bytes must stay valid and
 * unchanged until the next prepare or ZSTD_freeDCtx.
 * ZSTDMI_DCtx_getRangesAsyncPlan: what the valid prepare found — the table's entry count and the stream's content bytes (either
 * pointer may be NULL) -> 0; GENERIC for a NULL context, stage_wrong without a valid prepare.
 * ZSTDMI_decompressRangesAsync: all five arrays and everything they point to are DEVICE memory.  The call makes no device allocation,
 * no host wait, no copy between host and device and no host read of the arrays; it enqueues on the context's stream
 * (ZSTDMI_DCtx_setStream) and returns: 0 once enqueued (n == 0: 0, nothing is touched); GENERIC for a NULL context, or a NULL array with
 * n > 0; stage_wrong if there is no valid prepare, n > maxRanges, or a parameter, the dictionary, a DDict reference or the device
 * changed since the prepare (any setter but ZSTDMI_DCtx_setStream, ZSTD_DCtx_loadDictionary, ZSTD_DCtx_refDDict, ZSTD_DCtx_refPrefix:
 * only a generation counter is compared).  ZSTDMI_debugHostWaitsD and ZSTDMI_debugDeviceAllocsD do not move across it; stage timing
 * is off for the length of the call; the ZSTDMI_debugLastRanges* counters are NOT updated by it.
 * Per range, d_dstSizes[i] and the bytes at d_dsts[i] are exactly those of ZSTDMI_decompressRanges on a second context with the same
 * setup — min(length, max(total - offset, 0)) bytes; 0 for an empty range (d_dsts[i] may then be NULL); dstSize_tooSmall for more
 * than the capacity, then dstBuffer_null for a NULL destination, in that order; ranges may overlap, repeat and come in any order;
 * every touched frame is decoded once; a frame that fails fails every range that meets it, with the code of the lowest-indexed
 * failing frame it meets, nothing of such a range is written and the other ranges are served — with three exceptions:
 *   1. a range that would return more than maxRangeBytes answers workSpace_tooSmall and touches no frame (maxRangeBytes sizes the
 *      gather's grid; the synchronous call hands such a range to the single-range path);
 *   2. the limits.  Take the table entries with content that some served range meets, in table order: entry j is refused iff the
 *      number of those entries up to and including j exceeds maxFrames, or the sum of their table content sizes exceeds maxContent,
 *      or the sum of their blocks exceeds maxBlocks (and, should an entry hold more frames than one, their frames maxFrames).
 *      Sequence records beyond maxSequences fail as in ZSTDMI_decompressBatchAsync.  A range that meets a refused entry answers
 *      workSpace_tooSmall; ranges that meet only admitted entries are byte for byte what they are without the cut.  No arena byte
 *      beyond maxContent is ever written, whatever the frames' own headers say;
 *   3. there is no single-call path: a touched frame of more than 4 MiB compressed fails its ranges with srcSize_wrong, frames
 *      without a content size take the shared pass, and every long frame takes the ordered walk.
 * Nothing is written at or beyond d_dsts[i] + d_dstCapacities[i].  The arrays, the stream, the destinations and a referenced DDict
 * must stay valid and unchanged until the stream has passed the work; the context waits for work in flight by itself where
 * ZSTDMI_decompressBatchAsync's does.  Every call still scans the N-entry table (its cost follows N, not the touched frames).
 * Capturing the call into a hipGraph is neither claimed nor tested. */
typedef struct {
    size_t maxRanges;      /* ranges per call, > 0 */
    size_t maxRangeBytes;  /* returned bytes of one range, 1 .. 4 MiB: sizes the gather's grid */
    size_t maxContent;     /* content bytes of all frames one call touches, > 0: sizes the arena and the literal scratch */
    size_t maxFrames;      /* distinct frames one call touches; 0 = the table's entry count */
    size_t maxBlocks;      /* 0 = maxFrames + maxContent / 16384 */
    size_t maxSequences;   /* 0 = maxContent / 3 + 64 */
} ZSTDMI_DRangesLimits;
size_t ZSTDMI_rangesAsyncWorkspaceD(const ZSTDMI_DRangesLimits* limits, size_t tableEntries);
size_t ZSTDMI_DCtx_prepareRangesAsync(ZSTD_DCtx* dctx, const void* d_src, size_t srcSize, const ZSTDMI_DRangesLimits* limits);
size_t ZSTDMI_DCtx_getRangesAsyncPlan(const ZSTD_DCtx* dctx, size_t* tableEntries, unsigned long long* totalContent);
size_t ZSTDMI_decompressRangesAsync(ZSTD_DCtx* dctx, const unsigned long long* d_offsets, const size_t* d_lengths, size_t n,
                                    void* const* d_dsts, const size_t* d_dstCapacities, size_t* d_dstSizes);

/* Segmented stream decoding: ZSTD_decompressStream decodes a frame that is still arriving in SEGMENTS — runs of whole blocks —
 * instead of collecting the whole frame first.  bytes == 0 (the default): off, ZSTD_decompressStream behaves exactly as without this
 * call.  Otherwise `bytes` is the compressed size at which a segment is cut: whenever the frame in progress has at least that many
 * bytes of whole blocks buffered, those blocks are decoded and handed out (1 = a segment per block, as blocks arrive; a segment never
 * holds more than 2048 blocks).  A frame that is whole when the call first looks at it and holds fewer than `bytes` of blocks is
 * decoded as before.  Sticky; touches no device; zeroes the two counters below; GENERIC for a NULL context.  Between segments the
 * context keeps the last window of output on the device (and the dictionary's content until the frame has produced a window), the blocks that define the Huffman and FSE tables in force (at most four, on
 * the host), the three repcodes and the running checksum; the host holds at most bytes + one block + the caller's input + those four
 * blocks of a frame in progress.  The bytes handed out are those of the one-shot call, the return values follow the same protocol
 * (0 only on a frame boundary with everything flushed); a frame checksum is verified when the last block has been decoded
 * (checksum_wrong).  On damaged input the call returns an error no later than the end of the frame; bytes handed out before the failing
 * segment stay handed out.  A match that reaches further back than the frame's declared window is corruption_detected here, as in the
 * reference's streaming decoder (the one-shot call still has those bytes and decodes it).  With several device workers on the context
 * (ZSTDMI_DCtx_setDevices) ZSTD_decompressStream returns parameter_unsupported while the switch is on. */
size_t ZSTDMI_DCtx_setStreamSegment(ZSTD_DCtx* dctx, size_t bytes);
/* diagnostics of the stream session (since the last ZSTDMI_DCtx_setStreamSegment, or the context's creation), counted while the
 * switch is on: the largest number of compressed bytes held on the host at once (the input buffer plus the carried blocks); segments
 * decoded; -1 without a context */
long long ZSTDMI_debugStreamPeakInput(const ZSTD_DCtx* dctx);
int ZSTDMI_debugStreamSegments(const ZSTD_DCtx* dctx);

/* per-stage HIP-event timing of the LAST call (enable first).  Fills up to `cap` entries, returns the count. */
size_t ZSTDMI_CCtx_setProfiling(ZSTD_CCtx* cctx, int enable);
size_t ZSTDMI_DCtx_setProfiling(ZSTD_DCtx* dctx, int enable);
int    ZSTDMI_CCtx_getStageTimes(const ZSTD_CCtx* cctx, float* ms, const char** names, int cap);
int    ZSTDMI_DCtx_getStageTimes(const ZSTD_DCtx* dctx, float* ms, const char** names, int cap);

/* test hooks (kernel-level parity against the oracle) */
typedef struct { unsigned offBase; unsigned short litLength; unsigned short mlBase; } ZSTDMI_Seq;
/* sequences + literals the match finder produced for chunk `chunkIdx` of the last ZSTDMI/ZSTD compress call */
size_t ZSTDMI_debugGetChunk(ZSTD_CCtx* cctx, size_t chunkIdx, ZSTDMI_Seq* seqs, size_t seqCap, size_t* nbSeq,
                            void* lits, size_t litCap, size_t* litSize);
/* entropy-code ONE caller-supplied seqStore with the GPU kernels; returns the compressed block body size
 * (0 = "store raw", the reference's ZSTD_entropyCompressSeqStore convention) */
size_t ZSTDMI_debugEntropyBlock(ZSTD_CCtx* cctx, void* dst, size_t dstCapacity, const ZSTDMI_Seq* seqs, size_t nbSeq,
                                const void* lits, size_t litSize, size_t srcSize);
/* the same with offsets as the match finders store them: offBase = distance + 3 in every sequence (4 at least), turned into repcodes
 * by the sequence encoder against the history rep[0..2] (0 = unknown, as in front of a later block of a frame: it equals no offset).
 * After either call ZSTDMI_debugGetChunk(cctx, 0, ...) returns the seqStore as it was coded, "store raw" verdicts included */
size_t ZSTDMI_debugEntropyBlockRaw(ZSTD_CCtx* cctx, void* dst, size_t dstCapacity, const ZSTDMI_Seq* seqs, size_t nbSeq,
                                   const void* lits, size_t litSize, size_t srcSize, const unsigned rep[3]);
/* the entropy stage of ONE chunk whose ChunkMeta is taken as given, WITHOUT the host's range checks, over a seqStore filled with the
 * byte `fill`: what a faulty match finder would hand over.  The kernels must bound every size themselves (meta_checked, the
 * bitstream room): returns the bytes the chunk's frame would take, never faults.  tests/test_gpu_boundary.py */
/* the dictionary trainer's batch: n samples (concatenated in src, host memory) each compressed as ZSTD_compress2 would compress it
 * alone with the context's parameters and dictionary, in one pass through the pipeline; outSizes[i] = sample i's compressed size */
size_t ZSTDMI_debugCompressSamples(ZSTD_CCtx* cctx, const void* src, const size_t* sizes, size_t n, size_t* outSizes);
size_t ZSTDMI_debugPoisonedChunk(ZSTD_CCtx* cctx, unsigned nbSeq, unsigned litSize, unsigned srcSize, unsigned fill);
/* the record of the long-distance stage of the last pass of the context's last compress call (a context without device workers):
 * *nSplits = its splits, and for the first min(cap, *nSplits) of them, in position order, the window's start pos[i] and the match
 * found there (mLen[i] 0 = none; mStart[i] its first byte, mOff[i] its distance).  Every position is in the stage's own coordinate:
 * the pass's byte i lies at *base + i and nothing lies below *vlo (both 0 without a referenced prefix or a sliding window).
 * parameter_unsupported when that pass ran no long-distance stage.  tests/test_gpu_ldm_model.py */
size_t ZSTDMI_debugLdmPass(ZSTD_CCtx* cctx, unsigned* pos, unsigned* mStart, unsigned* mLen, unsigned* mOff, size_t cap,
                           size_t* nSplits, unsigned* base, unsigned* vlo);
/* on != 0: the long-distance stage of the context's later calls runs up to its matches and merges nothing into the finder's
 * sequences (the call still writes a valid stream, from those): ZSTDMI_debugGetChunk then shows what the merge would have been given */
size_t ZSTDMI_debugLdmSkipMerge(ZSTD_CCtx* cctx, int on);

#ifdef __cplusplus
}
#endif
#endif
