"""ctypes binding of libzstd_mi355x.so (the C ABI declared in include/zstd_mi355x.h).

The library is the product; there is no Python or CPU codec behind it.  If the shared object is missing or has
no gfx950 device to run on, calls fail loudly (ZstdException / OSError) — they never fall back.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libzstd_mi355x.so")

c_size_t, c_void_p, c_int, c_uint, c_ull = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong


class ZDICT_params_t(ctypes.Structure):
    _fields_ = [("compressionLevel", c_int), ("notificationLevel", c_uint), ("dictID", c_uint)]


class ZDICT_fastCover_params_t(ctypes.Structure):
    _fields_ = [("k", c_uint), ("d", c_uint), ("f", c_uint), ("steps", c_uint), ("nbThreads", c_uint),
                ("splitPoint", ctypes.c_double), ("accel", c_uint), ("shrinkDict", c_uint),
                ("shrinkDictMaxRegression", c_uint), ("zParams", ZDICT_params_t)]


class ZDICT_cover_params_t(ctypes.Structure):
    _fields_ = [("k", c_uint), ("d", c_uint), ("steps", c_uint), ("nbThreads", c_uint), ("splitPoint", ctypes.c_double),
                ("shrinkDict", c_uint), ("shrinkDictMaxRegression", c_uint), ("zParams", ZDICT_params_t)]


class ZSTDMI_Seq(ctypes.Structure):
    _fields_ = [("offBase", ctypes.c_uint32), ("litLength", ctypes.c_uint16), ("mlBase", ctypes.c_uint16)]


class DBatchLimits(ctypes.Structure):
    """ZSTDMI_DBatchLimits: what one ZSTDMI_decompressBatchAsync call may hold at most (0 in the last three = the default)."""
    _fields_ = [("maxEntries", c_size_t), ("srcSizeBound", c_size_t), ("maxContent", c_size_t), ("maxFrames", c_size_t),
                ("maxBlocks", c_size_t), ("maxSequences", c_size_t)]


class DRangesLimits(ctypes.Structure):
    """ZSTDMI_DRangesLimits: what one ZSTDMI_decompressRangesAsync call may hold at most (0 in the last three = the default)."""
    _fields_ = [("maxRanges", c_size_t), ("maxRangeBytes", c_size_t), ("maxContent", c_size_t), ("maxFrames", c_size_t),
                ("maxBlocks", c_size_t), ("maxSequences", c_size_t)]


class CBatchLimits(ctypes.Structure):
    """ZSTDMI_CBatchLimits: what one ZSTDMI_compressBatchAsync call may hold at most (maxChunks 0 = the default; reserved = 0)."""
    _fields_ = [("maxEntries", c_size_t), ("srcSizeBound", c_size_t), ("maxChunks", c_size_t), ("reserved", c_size_t * 3)]


class CutLimits(ctypes.Structure):
    """ZSTDMI_CutLimits: what one ZSTDMI_contentCutsAsync call may hold at most (maxCandidates 0 = the default; reserved = 0)."""
    _fields_ = [("srcSizeBound", c_size_t), ("avgLog", c_uint), ("kind", c_uint), ("maxCandidates", c_size_t), ("reserved", c_size_t * 3)]


# name -> (restype, argtypes); every symbol include/zstd_mi355x.h declares
SIGNATURES = {
    "ZSTD_createCCtx": (c_void_p, []),
    "ZSTD_freeCCtx": (c_size_t, [c_void_p]),
    "ZSTD_CCtx_setParameter": (c_size_t, [c_void_p, c_int, c_int]),
    "ZSTD_CCtx_getParameter": (c_size_t, [c_void_p, c_int, ctypes.POINTER(c_int)]),
    "ZSTD_CCtx_loadDictionary": (c_size_t, [c_void_p, c_void_p, c_size_t]),
    "ZSTD_CCtx_refPrefix": (c_size_t, [c_void_p, c_void_p, c_size_t]),
    "ZSTD_compressBound": (c_size_t, [c_size_t]),
    "ZSTD_compress2": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]),
    "ZSTD_compressCCtx": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_int]),
    "ZSTD_minCLevel": (c_int, []),
    "ZSTD_maxCLevel": (c_int, []),
    "ZSTD_defaultCLevel": (c_int, []),
    "ZSTD_createDCtx": (c_void_p, []),
    "ZSTD_freeDCtx": (c_size_t, [c_void_p]),
    "ZSTD_DCtx_setParameter": (c_size_t, [c_void_p, c_int, c_int]),
    "ZSTD_DCtx_getParameter": (c_size_t, [c_void_p, c_int, ctypes.POINTER(c_int)]),
    "ZSTD_DCtx_loadDictionary": (c_size_t, [c_void_p, c_void_p, c_size_t]),
    "ZSTD_DCtx_refPrefix": (c_size_t, [c_void_p, c_void_p, c_size_t]),
    "ZSTD_decompressBound": (c_ull, [c_void_p, c_size_t]),
    "ZSTD_getFrameContentSize": (c_ull, [c_void_p, c_size_t]),
    "ZSTD_findFrameCompressedSize": (c_size_t, [c_void_p, c_size_t]),
    "ZSTD_decompressDCtx": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]),
    "ZSTD_isError": (c_uint, [c_size_t]),
    "ZSTD_getErrorName": (ctypes.c_char_p, [c_size_t]),
    "ZSTD_versionNumber": (c_uint, []),
    "ZSTD_versionString": (ctypes.c_char_p, []),
    "ZSTD_compressStream2": (c_size_t, [c_void_p, c_void_p, c_void_p, c_int]),
    "ZSTD_decompressStream": (c_size_t, [c_void_p, c_void_p, c_void_p]),
    "ZSTD_CStreamInSize": (c_size_t, []),
    "ZSTD_CStreamOutSize": (c_size_t, []),
    "ZSTD_DStreamInSize": (c_size_t, []),
    "ZSTD_DStreamOutSize": (c_size_t, []),
    "ZDICT_isError": (c_uint, [c_size_t]),
    "ZDICT_getErrorName": (ctypes.c_char_p, [c_size_t]),
    "ZDICT_trainFromBuffer": (c_size_t, [c_void_p, c_size_t, c_void_p, ctypes.POINTER(c_size_t), c_uint]),
    "ZDICT_trainFromBuffer_fastCover": (c_size_t, [c_void_p, c_size_t, c_void_p, ctypes.POINTER(c_size_t), c_uint,
                                                   ZDICT_fastCover_params_t]),
    "ZDICT_optimizeTrainFromBuffer_fastCover": (c_size_t, [c_void_p, c_size_t, c_void_p, ctypes.POINTER(c_size_t), c_uint,
                                                           ctypes.POINTER(ZDICT_fastCover_params_t)]),
    "ZDICT_finalizeDictionary": (c_size_t, [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, ctypes.POINTER(c_size_t), c_uint,
                                            ZDICT_params_t]),
    "ZSTD_createCDict": (c_void_p, [c_void_p, c_size_t, c_int]),
    "ZSTDMI_createCDictOnDevice": (c_void_p, [c_void_p, c_size_t, c_int, c_int]),
    "ZSTD_freeCDict": (c_size_t, [c_void_p]),
    "ZSTD_sizeof_CDict": (c_size_t, [c_void_p]),
    "ZSTD_getDictID_fromCDict": (c_uint, [c_void_p]),
    "ZSTD_CCtx_refCDict": (c_size_t, [c_void_p, c_void_p]),
    "ZSTD_compress_usingCDict": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "ZSTD_createDDict": (c_void_p, [c_void_p, c_size_t]),
    "ZSTDMI_createDDictOnDevice": (c_void_p, [c_void_p, c_size_t, c_int]),
    "ZSTD_freeDDict": (c_size_t, [c_void_p]),
    "ZSTD_sizeof_DDict": (c_size_t, [c_void_p]),
    "ZSTD_getDictID_fromDDict": (c_uint, [c_void_p]),
    "ZSTD_DCtx_refDDict": (c_size_t, [c_void_p, c_void_p]),
    "ZSTD_decompress_usingDDict": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "ZSTD_getDictID_fromDict": (c_uint, [c_void_p, c_size_t]),
    "ZSTD_getDictID_fromFrame": (c_uint, [c_void_p, c_size_t]),
    "ZSTDMI_debugDictUploads": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugDictUploadsD": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugLastDictTableBlocks": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugLastSetFrames": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_deviceCount": (c_int, []),
    "ZSTDMI_CCtx_setDevice": (c_size_t, [c_void_p, c_int]),
    "ZSTDMI_DCtx_setDevice": (c_size_t, [c_void_p, c_int]),
    "ZSTDMI_CCtx_setDevices": (c_size_t, [c_void_p, ctypes.POINTER(c_int), c_int]),
    "ZSTDMI_DCtx_setDevices": (c_size_t, [c_void_p, ctypes.POINTER(c_int), c_int]),
    "ZSTDMI_CCtx_setStream": (c_size_t, [c_void_p, c_void_p]),
    "ZSTDMI_DCtx_setStream": (c_size_t, [c_void_p, c_void_p]),
    "ZSTDMI_CCtx_setPassChunks": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_CCtx_setHistory": (c_size_t, [c_void_p, c_int, c_uint]),
    "ZSTDMI_DCtx_setLiteralDecoder": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_DCtx_setLongFrames": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_DCtx_setOverlap": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_DCtx_setExecWaves": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_debugLastWalkSerial": (c_int, [c_void_p]),
    "ZSTDMI_debugLastFarPlane": (c_int, [c_void_p]),
    "ZSTDMI_CCtx_setParser": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_compressDevice": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]),
    "ZSTDMI_decompressDevice": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]),
    "ZSTDMI_compressBatch": (c_size_t, [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t), c_size_t,
                                        ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    "ZSTDMI_decompressBatch": (c_size_t, [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t), c_size_t,
                                          ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    "ZSTDMI_compressBatchCDicts": (c_size_t, [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t), c_size_t,
                                              ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t), ctypes.POINTER(c_void_p)]),
    "ZSTDMI_CCtx_prepareBatchAsync": (c_size_t, [c_void_p, c_size_t, c_size_t]),
    # (the five arrays are device memory: plain addresses)
    "ZSTDMI_compressBatchAsync": (c_size_t, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "ZSTDMI_CCtx_prepareBatchAsyncLimits": (c_size_t, [c_void_p, ctypes.POINTER(CBatchLimits)]),
    "ZSTDMI_CCtx_getBatchAsyncPlan": (c_size_t, [c_void_p, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    "ZSTDMI_debugHostWaits": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugDeviceAllocs": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_batchAsyncWorkspaceD": (c_size_t, [ctypes.POINTER(DBatchLimits)]),
    "ZSTDMI_DCtx_prepareBatchAsync": (c_size_t, [c_void_p, ctypes.POINTER(DBatchLimits)]),
    "ZSTDMI_decompressBatchAsync": (c_size_t, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "ZSTDMI_debugHostWaitsD": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugDeviceAllocsD": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugLastBatchAlone": (c_int, [c_void_p]),
    "ZSTDMI_debugLastBatchPasses": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugLastBatchSetChunks": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugLastBatchAloneD": (c_int, [c_void_p]),
    "ZSTDMI_DCtx_setBatchUnsized": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_debugLastBatchWorkspace": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_packBound": (c_size_t, [ctypes.POINTER(c_size_t), c_size_t]),
    "ZSTDMI_compressPack": (c_size_t, [c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t), c_size_t]),
    "ZSTDMI_CCtx_packAsyncBound": (c_size_t, [c_void_p, c_size_t]),
    "ZSTDMI_compressPackAsync": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "ZSTDMI_debugLastPackAlone": (c_int, [c_void_p]),
    "ZSTDMI_debugLastPackFrames": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_CCtx_setContentCuts": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_contentCutsBound": (c_size_t, [c_size_t, c_uint]),
    "ZSTDMI_contentCuts": (c_size_t, [c_void_p, c_void_p, c_size_t, c_uint, ctypes.POINTER(c_size_t), c_size_t, ctypes.POINTER(c_size_t)]),
    "ZSTDMI_debugLastContentCuts": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_digestSize": (c_size_t, [c_uint]),
    "ZSTDMI_digestPieces": (c_size_t, [c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_size_t), c_size_t, c_uint, c_void_p, c_size_t]),
    "ZSTDMI_contentCutsDigests": (c_size_t, [c_void_p, c_void_p, c_size_t, c_uint, c_uint, ctypes.POINTER(c_size_t), c_size_t, ctypes.POINTER(c_size_t),
                                             c_void_p, c_size_t]),
    "ZSTDMI_debugDigestModel": (c_size_t, [c_uint, c_void_p, c_size_t, c_void_p]),
    "ZSTDMI_cutsAsyncWorkspace": (c_size_t, [ctypes.POINTER(CutLimits)]),
    "ZSTDMI_CCtx_prepareCutsAsync": (c_size_t, [c_void_p, ctypes.POINTER(CutLimits)]),
    "ZSTDMI_CCtx_getCutsAsyncPlan": (c_size_t, [c_void_p, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    "ZSTDMI_contentCutsAsync": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]),
    "ZSTDMI_debugCutsAsyncStages": (c_size_t, [c_void_p, c_void_p, c_size_t, ctypes.POINTER(ctypes.c_float)]),
    "ZSTDMI_debugCutSelectParallel": (c_size_t, [c_void_p, ctypes.POINTER(c_uint), c_size_t, c_ull, c_uint, ctypes.POINTER(c_uint), c_size_t,
                                                 ctypes.POINTER(c_size_t)]),
    "ZSTDMI_CCtx_setSeekTable": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_CCtx_setDictEntropy": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_CCtx_setEntropyCarry": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_debugLastCarryGroups": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_CCtx_setDictIndex": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_CCtx_setDictIndexStrategy": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_CCtx_setDictIndexChain": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_debugLastRegionChunks": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugDictIndexed": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_CCtx_setSingleFrame": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_CCtx_setSlidingLdm": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_CCtx_setFarOffsets": (c_size_t, [c_void_p, c_uint]),
    "ZSTDMI_seekTableBound": (c_size_t, [c_size_t]),
    "ZSTDMI_decompressRange": (c_size_t, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_ull, c_size_t]),
    "ZSTDMI_debugLastRangeFrames": (c_int, [c_void_p]),
    "ZSTDMI_debugLastRangeStaged": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_decompressRanges": (c_size_t, [c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_ull), ctypes.POINTER(c_size_t), c_size_t,
                                           ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]),
    "ZSTDMI_rangesAsyncWorkspaceD": (c_size_t, [ctypes.POINTER(DRangesLimits), c_size_t]),
    "ZSTDMI_DCtx_prepareRangesAsync": (c_size_t, [c_void_p, c_void_p, c_size_t, ctypes.POINTER(DRangesLimits)]),
    "ZSTDMI_DCtx_getRangesAsyncPlan": (c_size_t, [c_void_p, ctypes.POINTER(c_size_t), ctypes.POINTER(c_ull)]),
    # (the five arrays are device memory: plain addresses)
    "ZSTDMI_decompressRangesAsync": (c_size_t, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "ZSTDMI_debugLastRangesFrames": (c_int, [c_void_p]),
    "ZSTDMI_debugLastRangesAlone": (c_int, [c_void_p]),
    "ZSTDMI_debugLastRangesStaged": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_DCtx_setStreamSegment": (c_size_t, [c_void_p, c_size_t]),
    "ZSTDMI_debugStreamPeakInput": (ctypes.c_longlong, [c_void_p]),
    "ZSTDMI_debugStreamSegments": (c_int, [c_void_p]),
    "ZSTDMI_CCtx_setProfiling": (c_size_t, [c_void_p, c_int]),
    "ZSTDMI_DCtx_setProfiling": (c_size_t, [c_void_p, c_int]),
    "ZSTDMI_CCtx_getStageTimes": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_char_p), c_int]),
    "ZSTDMI_DCtx_getStageTimes": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_char_p), c_int]),
    "ZSTDMI_debugGetChunk": (c_size_t, [c_void_p, c_size_t, ctypes.POINTER(ZSTDMI_Seq), c_size_t, ctypes.POINTER(c_size_t),
                                        c_void_p, c_size_t, ctypes.POINTER(c_size_t)]),
    "ZSTDMI_debugLdmPass": (c_size_t, [c_void_p, ctypes.POINTER(c_uint), ctypes.POINTER(c_uint), ctypes.POINTER(c_uint), ctypes.POINTER(c_uint), c_size_t,
                                       ctypes.POINTER(c_size_t), ctypes.POINTER(c_uint), ctypes.POINTER(c_uint)]),
    "ZSTDMI_debugLdmSkipMerge": (c_size_t, [c_void_p, c_int]),
    "ZSTDMI_debugCompressSamples": (c_size_t, [c_void_p, c_void_p, ctypes.POINTER(c_size_t), c_size_t, ctypes.POINTER(c_size_t)]),
    "ZSTDMI_debugPoisonedChunk": (c_size_t, [c_void_p, c_uint, c_uint, c_uint, c_uint]),
    "ZSTDMI_debugEntropyBlock": (c_size_t, [c_void_p, c_void_p, c_size_t, ctypes.POINTER(ZSTDMI_Seq), c_size_t,
                                            c_void_p, c_size_t, c_size_t]),
    "ZSTDMI_debugEntropyBlockRaw": (c_size_t, [c_void_p, c_void_p, c_size_t, ctypes.POINTER(ZSTDMI_Seq), c_size_t,
                                               c_void_p, c_size_t, c_size_t, ctypes.POINTER(c_uint)]),
}

_lib = None


def load():
    """Load the shared object and type every exported symbol.  Raises OSError if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"or `make -C zstdsharp_amd/csrc` (there is no fallback codec)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError here = ABI drift between header and library
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib
