// zmi_common.h — layouts shared by the host driver and the gfx950 kernels.
//
// Domain vocabulary follows the reference (ZstdSharp / zstd 1.5.1): chunks become frames, each frame holds
// one block; a block is a literals section + a sequences section (U/ZstdCompress.cs:3236-3354).
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace zmi {

typedef uint8_t  u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int16_t  s16;
typedef int32_t  s32;
typedef int64_t  s64;

// ---- framing: one independent zstd frame per 64 KiB chunk ----
constexpr u32 kChunkLog   = 16;
constexpr u32 kChunkSize  = 1u << kChunkLog;
// literal buffer of chunk c starts at c * kLitStride: the 320-byte skew keeps the chunks' writers and readers, which move in
// lockstep, from hitting addresses that agree in their low 16 bits (channel camping)
constexpr u32 kLitStride  = kChunkSize + 320;
constexpr u32 kSlotStride = kChunkSize + 512;      // >= ZSTD_compressBound(64 KiB) + frame/block headers + checksum
constexpr u32 kMaxSeq     = kChunkSize / 4;        // a sequence consumes >= 4 input bytes in this match finder

// one stored sequence: same meaning as the reference's seqDef_s (U/seqDef_s.cs)
struct Seq { u32 offBase; u16 litLength; u16 mlBase; };   // offBase 1..3 repcode, >=4 distance+3 ; mlBase = matchLength-3

// kLitTreeless: Huffman-coded with the formatted dictionary's table (literals type 3, no tree description; ZSTDMI_CCtx_setDictEntropy)
enum LitMode : u32 { kLitRaw = 0, kLitRle = 1, kLitCompressed = 2, kLitTreeless = 3 };

// per-chunk record that travels between the pipeline's kernels (HBM resident)
struct ChunkMeta {
    u32 srcSize;        // bytes of input in this chunk (<= 64 KiB)
    u32 nbSeq;          // sequences found by the match finder
    u32 litSize;        // literal bytes (trailing literals included)
    u32 fhSize;         // frame header bytes for this chunk
    // literals section, decided by huf_build
    u32 litMode;        // LitMode
    u32 litSingle;      // 1 = single stream
    u32 lhSize;         // literals section header bytes (1..5)
    u32 hufHdrSize;     // Huffman tree description bytes
    u32 streamSize[4];  // bytes per Huffman stream
    u32 litSectionSize; // whole literals section
    // result
    u32 bodySize;       // compressed block body (literals + sequences sections) or 0 if stored raw/RLE
    u32 blockType;      // 0 raw, 1 RLE, 2 compressed
    u32 outSize;        // frame bytes in the slot (header + block + optional checksum)
    u32 checksum;       // low 32 bits of XXH64 of the chunk when the checksum flag is set
    u32 rleByte;        // the byte of an RLE literals section
    u32 litFromSrc;     // 1 = the chunk has no sequences and its literals were never copied: they ARE the chunk's source bytes
    u32 regionCursor;   // != 0: lz_kernel stopped behind the chunk's first tile (dense data); lz_region_kernel does the rest from
                        // parse cursor regionCursor - 1 (nbSeq / litSize / litFromSrc hold the state after that tile)
};

// Huffman code table for one chunk (HBM): canonical codes as the reference assigns them (U/HufCompress.cs:750-788)
struct HufTable {
    u16 code[256];
    u8  nbBits[256];
    u8  hdr[132];       // tree description as written by HUF_writeCTable (<= 129 bytes)
    u32 maxSV, tableLog;
};

// one symbol's transform of an FSE compression table (FSE_symbolCompressionTransform, U/FseCompress.cs:13-191)
struct SymTT { s32 deltaFindState; u32 deltaNbBits; };

// A formatted dictionary's entropy tables as the compressor uses them (ZSTD_loadCEntropy, U/ZstdCompress.cs:5259-5400), built once
// per dictionary load by dict_ctables_kernel and read by every chunk of a call with ZSTDMI_CCtx_setDictEntropy on (it stays in L2).
// The Huffman table is in HufTable's layout (canonical codes as HUF_readCTable assigns them), the three FSE tables in the layout
// seq_encode_kernel keeps in LDS.  The four repeat states: hufMode, and seqValid[] in the order LL, OF, ML.
enum : u32 { kDictHufNone = 0, kDictHufCheck = 1, kDictHufValid = 2 };
struct DictCTables {
    u16 hufCode[256];
    u8  hufNbBits[256];
    u32 hufMode;            // kDictHufValid: no zero weight; kDictHufCheck: every literal of a block must have a code; kDictHufNone: the
                            // table cannot be used (fewer than 256 symbols, or codes longer than the encoder's 11 bits)
    u32 seqValid[3];        // 1 = FSE_repeat_valid: set_repeat may be chosen without looking at the block's codes
    u32 seqLog[3];          // tableLog
    u32 pad;
    u64 seqPresent[3];      // bit s: symbol s has a probability in the table
    u16 llState[512], mlState[512], ofState[256];
    SymTT llTT[36], mlTT[53], ofTT[32];
};

// ---- decoder side ----
// Literal scratch of frame f starts at its output offset + f * kLitSkew: without the skew all frames' streams write addresses
// that agree in their low 14 bits at any moment (four 16 KiB segments per 64 KiB frame, decoded in lockstep).
#ifndef ZMI_LITSKEW
#define ZMI_LITSKEW 320
#endif
constexpr u32 kLitSkew = ZMI_LITSKEW;

// A formatted dictionary as the decoder sees it (filled by dict_parse_kernel; ZSTD_loadDEntropy, U/ZstdDecompress.cs:1773-1875):
// offsets into the dictionary bytes of the Huffman description and of the three NCounts, the repcodes, where the content starts.
struct DictInfo {
    u32 err;                        // 0, or kErrDictionaryCorrupted
    u32 dictID;
    u32 hufOff, hufSize;
    u32 ofOff, mlOff, llOff;        // each NCount runs up to the next offset (llOff up to repOff)
    u32 repOff;
    u32 rep[3];
    u32 contentOff, contentSize;
    u32 pad[3];
};

// The decoder's work lists (decode_walk.hip builds them).  A frame is a run of blocks; blocks are the
// unit every parallel stage works on: a block's literals and its three FSE state chains depend on nothing but the tables the
// pre-pass resolves for it (U/ZstdDecompressBlock.cs:197-207, 1780-1786), only the LZ execution is ordered inside a frame.
struct FrameDesc {      // one per frame found by the frame walk (U/ZstdDecompress.cs:877-951)
    u64 srcOff;         // offset of the frame in the compressed input
    u64 dstOff;         // offset of its content in the output (frames without a content size: after their regenerated sizes are known)
    u64 scratchOff;     // offset of its literals in the literal scratch: the content-size (or bound) prefix sum the walk produced
    u64 srcSize;        // compressed frame size
    u64 dstSize;        // content size; for a frame without one the bound nbBlocks x blockSizeMax until the regenerated size replaces it
    u32 firstBlock, nbBlocks;
    u32 unsized;        // bit 0 (kFrameUnsized) = the header carries no content size; bit 1 (kFrameOpen), a batch entry that holds such a
                        // frame: this frame's place is not final when the lists are emitted — it is unsized, lies behind an unsized
                        // one, or the entry's capacity has yet to admit it — so nothing may write its output before batch_rescan
    u32 checksum;       // 1 = a 4-byte XXH64 checksum follows the last block
    u32 bad;            // 1 = some stage failed in this frame (its error is in the status words): later stages leave it alone
    u32 hasSeq;         // 1 = at least one block holds sequences (the ordered executor has work in this frame)
    u32 viaOrigin;      // 1 = the frame's matches are resolved by the origin path (decode_origin.hip): exec_matches only checks its checksum
    u32 dictSlot;       // its dictionary's record in the slot table (zmi_dictset.h) when the set kernels run (ZSTD_d_refMultipleDDicts); else 0, unread
    u64 originOff;      // then: index of its first entry in the origin array
};

// XXH64 of a frame that is decoded in segments (decode_stream.hip): the state between two segments.  reset: acc = the four seeds
// (P1 + P2, P2, 0, -P1), everything else zero (xxh_carry_reset, zstd_mi355x_dec.hip)
struct XxhCarry { u64 acc[4]; u64 total; u32 tailLen; u32 hash; u8 tail[32]; };

// (bit 2, set by block_link's open instances: some block of the frame found no room in the clamped literal scratch — the entry cannot fit)
enum : u32 { kFrameUnsized = 1, kFrameOpen = 2, kFrameNoRoom = 4 };

constexpr u32 kNoBlock   = 0xFFFFFFFFu;     // table source: nothing defined it (corruption, or the default where that is legal)
constexpr u32 kDictBlock = 0xFFFFFFFEu;     // table source: the formatted dictionary

// One block of a frame.  Filled in stages: the walk (position, type, size), block_parse (the sections of a compressed block),
// block_link (where repeat-mode tables and treeless literals come from, literal offsets, record offsets), seq_decode (regenerated
// size, repcode transfer), block_offsets (output offset, repcodes at the block's start).
struct BlockDesc {
    u64 srcOff;         // the block's body in the compressed input (absolute; behind its 3-byte header)
    u64 dstRel;         // output offset relative to its frame's
    u64 litRel;         // offset of its regenerated literals relative to the frame's scratch (Huffman-coded literals sections only)
    u64 seqBase;        // index of its first sequence record
    u32 frame;
    u32 bsz;            // body bytes in the input (an RLE block: 1)
    u32 outSize;        // regenerated bytes: raw/RLE from the header; compressed: litSize when it has no sequences, else from seq_decode
    u8  type, last, litType, litSingle;     // block type 0 raw 1 RLE 2 compressed; literals section type 0 raw 1 RLE 2 compressed 3 treeless
    u32 litSize, litCSize;
    u32 lhSize;         // literals section header bytes
    u32 hufSrc;         // block whose literals section holds this block's Huffman table description (itself, an earlier one, kDictBlock)
    u32 nbSeq;
    u32 modes;          // the symbol-compression-modes byte (LL << 6 | OF << 4 | ML << 2)
    u32 tblOff[3];      // LL, OF, ML table descriptions inside the body (RLE byte or NCount), where the mode has one
    u32 bitsOff;        // start of the sequence bitstream inside the body
    u32 tblSrc[3];      // block whose sequences header defines the table this block uses (itself unless repeat mode)
    // repcodes: out = f(in), slot by slot.  kind 0: the constant val; kind 1..3: max(in[kind - 1] - val, 1)  (U/ZstdDecompressBlock.cs:2387-2443)
    u32 repKind[3], repVal[3];
    u32 repIn[3];       // the three repcodes at the block's start (block_offsets)
    u32 err;            // first error found in this block (0 = none)
    u32 litInPlace;     // 1 = no sequences: the literal decoder writes the block's output itself (block_link decides; when the literal
                        // decoder runs beside seq_decode only a sized frame's first block can — the others' offsets are not known yet)
};

// One decoded sequence (U/ZstdDecompressBlock.cs:2360-2484) as seq_decode leaves it for the executors, packed into 8 bytes:
//   bits  0-16  litLength (<= 131071: LL_base[35] + 16 extra bits)
//   bits 17-33  matchLength - 3 (<= 131071: ML_base[52] + 16 extra bits - 3)
//   bits 34-63  bit 29 clear: the match offset (1 .. 2^29 - 1);
//               bit 29 set, bits 27-28 = i (1..3): a repcode left symbolic — bits 0-26 = d: the offset is max(repIn[i - 1] - d, 1)
//               bit 29 set, bits 27-28 = 0 (kRecFar): a far offset (2^29 and more, a repeat of one included) — its 32 bits are the
//               record's word of the far plane, one u32 per record, which only a call with a far-capable frame has (a frame whose
//               content plus dictionary or prefix content exceeds kRecOffMax: decompress_device).  Every other call passes no plane
//               and refuses such an offset with windowTooLarge, as do the batch, range and segmented paths.
// The output position is not stored: consumers walk a block's records in order and carry the running sum of litLength + matchLength.
struct SeqRec { u32 lo, hi; };
constexpr u32 kRecOffMax = (1u << 29) - 1;
constexpr u32 kRecFar = 1u << 29;

// A batch of independent entries (ZSTDMI_decompressBatch): what the host says of entry e, and what the batch walk finds in it.
// Offsets are relative to one base pointer each for sources and destinations (the lowest of the call); the lists of all entries
// are one FrameDesc / BlockDesc array, entry e's frames and blocks side by side from firstFrame / firstBlock.
struct BatchEntryIn { u64 srcOff, srcSize, dstOff, dstCap; };
enum : u32 { kBatchDecode = 0, kBatchDone = 1, kBatchAlone = 2 };
struct BatchEntryOut {
    u64 result;         // the entry's answer: its content size, or an error in the size_t convention (kBatchAlone: not yet known)
    u64 scratchOff;     // literal scratch of its first frame (prefix sum of the content sizes over the entries that are decoded)
    u32 firstFrame, firstBlock, nFrames, nBlocks;
    u32 state;          // kBatchDecode: its frames are in the lists; kBatchDone: `result` is final (header-stage error, dstSize_tooSmall);
    u32 open;           // kBatchAlone: the single-call path decodes it afterwards (a frame without a content size, a very large entry)
                        // open (kBatchDecode under ZSTDMI_DCtx_setBatchUnsized): 1 = it holds a frame without a content size: `result` is the
                        // literal scratch it asks for until batch_rescan_kernel puts its answer there
};

// A range of a seekable stream (ZSTDMI_decompressRange): what seek_select_kernel makes of the seek table and (offset, length), and
// what range_check_kernel finds after the decode — u64 words, read back by the host in one copy each.  "Selected" = the table entries
// from the first to the last one with content that meets the range; cLo / cHi = the compressed bytes they span.
enum : u32 { kSeekErr = 0, kSeekTotal = 1,      // the table's error (0 = none); content bytes of the whole stream
             kSeekMeet = 2,                     // entries with content that meet the range
             kSeekFirst = 3, kSeekLast = 4,     // their first and last index in the table
             kSeekCLo = 5, kSeekCHi = 6,
             kSeekDFirst = 7, kSeekSizeFirst = 8, kSeekDLast = 9, kSeekSizeLast = 10,      // content offset and size of the first and the last
             kSeekKey = 11,                     // range_check: entry index << 16 | error of the first failing entry (all ones = none)
             kSeekAlone = 12,                   // range_check: entries left to the single-call path
             kSeekWords = 16 };
// one copy of range_clip_kernel: bytes [from, from + len) of the edge buffer to dst + to
struct ClipJob { u64 from, to, len; };

// Many ranges of a seekable stream in one call (ZSTDMI_decompressRanges, decode_ranges.hip).  The host says RangeIn of range i;
// ranges_select_kernel files RangeRec: what the range returns (or its error, in the size_t convention) and, for a served range, the
// first and the last table entry with content that it meets.  Every touched entry is decoded once into its slot of an arena.
struct RangeIn { u64 offset, length, dstCap, dst; };            // dst: the device address (0 = NULL)
enum : u32 { kRangeDone = 0,        // `result` is final: an empty range, dstSize_tooSmall, dstBuffer_null
             kRangeServed = 1,      // the gathered pass decodes its entries; ranges_gather_kernel copies its bytes
             kRangeAlone = 2 };     // more than kRangesAloneAbove bytes: the single-range path takes it afterwards
struct RangeRec { u64 result; u32 first, last, state, pad; };
constexpr u64 kRangesAloneAbove = (u64)4 << 20;
constexpr u32 kRangesTile = 1024;           // table entries per workgroup of the grid-wide scans
constexpr u32 kGatherSlice = 64u << 10;     // output bytes per workgroup of ranges_gather_kernel
constexpr u32 kNoEntry = 0xFFFFFFFFu;       // decode index of a table entry that is not touched
enum : u32 { kRgErr = 0, kRgTotal = 1,      // the table's error (0 = none); content bytes of the whole stream
             kRgTouched = 2,                // distinct entries with content that the served ranges meet
             kRgArena = 3, kRgCompact = 4,  // their content bytes (the arena), their compressed bytes (a host source's staging buffer)
             kRgRuns = 5,                   // maximal runs of consecutive touched entries
             kRgAloneEntries = 6,           // touched entries the batch walk left to the single-call path (ranges_alone_kernel)
             kRgWords = 8 };
// the pass's device workspace for a table of N entries, T = N / kRangesTile + 1 tiles (ranges_ws_bytes / ranges_ws)
struct RangesWs {
    u64* cOff; u64* dOff;       // N + 1 each: exclusive prefix of the compressed sizes, of the content sizes
    u64* slot;                  // N: the entry's offset in the arena
    u64* runs;                  // N + 2 words: the runs of touched entries as compressed [lo, hi) pairs (at most (N + 1) / 2 runs)
    u64* tileIdx; u64* tileCover; u64* tilePlan;        // (T + 1) x 2, 1, 4: tile sums, then tile carries; the totals in row T
    u64* sum;                   // kRgWords
    u32* diff;                  // N + 1: +1 at a served range's first entry, -1 behind its last (mod 2^32); its prefix sum = ranges over an entry
    u32* decIdx;                // N: the entry's index in the decode table, kNoEntry = not touched
};

// status words shared by the decoder's kernels and the host
enum : u32 { kStFrames = 0, kStErr = 1, kStTotalLo = 2, kStTotalHi = 3, kStUsable = 4, kStUnsized = 5, kStBlocks = 6, kStSeqLo = 8, kStSeqHi = 9,
             kStErrKeyLo = 10, kStErrKeyHi = 11, kStActualLo = 12, kStActualHi = 13,
             kStBlockKeysLo = 7, kStBlockKeysHi = 15,   // a batch call: address of one error key per block (report_error files there too); 0 = none
             kStOriginFrames = 14,      // frames the origin path took (origin_select_kernel)
             kStOriginLo = 16, kStOriginHi = 17,        // entries of the origin array handed out so far (u64)
             kStOriginChanged = 18,     // .. 18 + kOriginRounds: round r of the pointer jumping changed something
             kStLitLo = 54, kStLitHi = 55,              // regenerated bytes of all Huffman-coded literals sections (u64; block_link)
             kStBigBins = 56,           // 12 x u64: content bytes of the frames with sequences by size class, bin k = [2^(20+k), 2^(21+k)), below 2^30
             kStDictTabBlocks = 80,     // blocks that copied a sequence table from a DDict's ready-made set (seq_decode_kernel's instance for it)
             kStSetFrames = 82,         // frames whose dictionary was found in the DDict set by dictID (the walks' set instances)
             // a batch call under ZSTDMI_DCtx_setBatchUnsized (the open instances of the walk and of block_link):
             kStOpenEntries = 84,       // entries in the lists that hold a frame without a content size
             kStRoomLo = 85, kStRoomHi = 86,            // address of one u64 per frame: the room its literals have in the scratch
             kStDumpLo = 87, kStDumpHi = 88,            // offset in the scratch of kLitDump bytes that every block without room decodes into
             // a batch enqueued from the device (ZSTDMI_decompressBatchAsync): the caller's limits, filed by batch_init_d_kernel for the
             // scans' cap instances (batch_scan: frames, blocks, literal-scratch bytes; seq_scan: sequence records)
             kStCapFrames = 90, kStCapBlocks = 91, kStCapContentLo = 92, kStCapContentHi = 93, kStCapSeqLo = 94, kStCapSeqHi = 95,
             kStWords = 96 };
// Literals of a block that has no room left in its frame's scratch (the room of an entry with unsized frames is clamped to the entry's
// capacity) still have to be decoded — a damaged stream's error outranks dstSize_tooSmall — but nobody reads them
constexpr u32 kLitDump = (128u << 10) + 512;
constexpr u32 kOriginRounds = 36;

// Stage timing (ZSTDMI_*_setProfiling): a launcher that issues several kernels marks the end of each on the context's timer, so
// that a stage time is ONE kernel's duration (bench.py prices the slowest kernel against the HBM roof).  No-op when profiling is off.
struct StageHook {
    void (*fn)(void* self, const char* name) = nullptr; void* self = nullptr;
    void operator()(const char* name) const { if (fn) fn(self, name); }
};

// Long-distance matching (ldm.hip) as a call resolves it (ZSTD_ldm_adjustParameters, U/ZstdLdm.cs:187-212)
struct LdmLaunch { u32 minMatch, hashLog, bucketLog, hashRateLog; };
// A referenced prefix in front of the pass (ZSTD_CCtx_refPrefix, ldm.hip): device pointer (nullptr = none), the source's first byte
// in the virtual coordinate (the prefix length rounded up to kLdmPrefixAlign) and the prefix's first byte there (base - prefix length)
// maxDist (0 = none): a window that slides with its frame (ZSTDMI_CCtx_setSlidingLdm): the "prefix" is the frame's content in front of
// the pass, and no match may lie further back than this many bytes
struct LdmPrefix { const u8* pre = nullptr; u32 base = 0, vlo = 0, maxDist = 0; };
constexpr u32 kLdmPrefixAlign = 16384;
constexpr u32 kLdmMinHashRateLog = 5;      // the split workspace keeps at most one split per 16 bytes: denser split rates are refused

// error codes: U/ZSTD_ErrorCode.cs
enum : u32 {
    kErrGeneric = 1, kErrPrefixUnknown = 10, kErrVersionUnsupported = 12, kErrFrameParameterUnsupported = 14,
    kErrWindowTooLarge = 16, kErrCorruption = 20, kErrChecksumWrong = 22, kErrDictionaryCorrupted = 30,
    kErrDictionaryWrong = 32, kErrDictionaryCreationFailed = 34, kErrParameterUnsupported = 40, kErrParameterOutOfBound = 42,
    kErrTableLogTooLarge = 44, kErrMaxSymbolValueTooLarge = 46, kErrMaxSymbolValueTooSmall = 48,
    kErrStageWrong = 60, kErrInitMissing = 62, kErrMemoryAllocation = 64, kErrWorkSpaceTooSmall = 66,
    kErrDstSizeTooSmall = 70, kErrSrcSizeWrong = 72, kErrDstBufferNull = 74, kErrMaxCode = 120
};

} // namespace zmi
