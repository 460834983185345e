"""Mirror of ZstdSharp.Compressor (S/Compressor.cs) over libzstd_mi355x.so."""
import ctypes

from . import _ffi
from .errors import DST_SIZE_TOO_SMALL, ensure_zstd_success

ZSTD_c_compressionLevel = 100
# long-distance matching (include/zstd_mi355x.h): the switch takes ZSTD_ps_*; the others 0 = from the window
ZSTD_c_enableLongDistanceMatching = 160
ZSTD_c_ldmHashLog = 161
ZSTD_c_ldmMinMatch = 162
ZSTD_c_ldmBucketSizeLog = 163
ZSTD_c_ldmHashRateLog = 164
ZSTD_ps_auto, ZSTD_ps_enable, ZSTD_ps_disable = 0, 1, 2


def _as_buffer(data):
    """bytes / bytearray / memoryview / numpy -> (address, length, keepalive)"""
    if isinstance(data, bytes):
        return ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value if data else None, len(data), data
    mv = memoryview(data).cast("B")
    if len(mv) == 0:
        return None, 0, mv
    if mv.readonly:
        b = bytes(mv)
        return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value, len(b), b
    arr = (ctypes.c_ubyte * len(mv)).from_buffer(mv)
    return ctypes.addressof(arr), len(mv), (arr, mv)


def _as_prefix(prefix):
    """bytes-like or a contiguous CUDA uint8 tensor -> (address, length, keepalive, device to synchronise or None)"""
    if hasattr(prefix, "data_ptr"):
        import torch
        if not (prefix.is_cuda and prefix.dtype == torch.uint8 and prefix.is_contiguous()):
            raise TypeError("expected a contiguous CUDA uint8 tensor")
        return (prefix.data_ptr() if prefix.numel() else None), prefix.numel(), prefix, prefix.device
    addr, n, keep = _as_buffer(prefix if prefix is not None else b"")
    return addr, n, keep, None


class _PrefixHolder:
    """The referenced prefix of a context: kept alive until the consuming call has returned."""

    _prefix_keep = None
    _prefix_device = None

    def _hold_prefix(self, keep, device):
        self._prefix_keep, self._prefix_device = keep, device

    def _prefix_ready(self):
        # the library runs on a stream of its own: what torch has queued for a device prefix must have finished
        if self._prefix_device is not None:
            import torch
            torch.cuda.synchronize(self._prefix_device)

    def _release_prefix(self):
        self._prefix_keep, self._prefix_device = None, None


class Compressor(_PrefixHolder):
    """S/Compressor.cs:7-163.  One instance is used by one thread at a time."""

    def __init__(self, level: int = 0, device: int = None):
        self._lib = _ffi.load()
        self.cctx = self._lib.ZSTD_createCCtx()          # S/Compressor.cs:32
        if not self.cctx:
            raise MemoryError("ZSTD_createCCtx")
        if device is not None:
            ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setDevice(self.cctx, device))
        self._level = 0
        self._seek_table = False
        self._dict_entropy = False
        self._entropy_carry = False
        self._dict_index = False
        self._dict_index_strategy = 1
        self._dict_index_chain = False
        self._single_frame = False
        self._sliding_ldm = False
        self._far_offsets = False
        self._content_cuts = 0
        self._cdict = None              # the CDict RefCDict holds
        self.Level = level if level else self.DefaultCompressionLevel

    # ---- static members (S/Compressor.cs:8-10) ----
    @staticmethod
    def _static(name):
        return getattr(_ffi.load(), name)()

    MinCompressionLevel = property(lambda self: self._lib.ZSTD_minCLevel())
    MaxCompressionLevel = property(lambda self: self._lib.ZSTD_maxCLevel())
    DefaultCompressionLevel = 3

    # ---- Level (S/Compressor.cs:16-27) ----
    @property
    def Level(self):
        return self._level

    @Level.setter
    def Level(self, value):
        if self._level != value:
            self._level = value
            self.SetParameter(ZSTD_c_compressionLevel, value)

    level = Level

    def SetParameter(self, parameter: int, value: int):      # S/Compressor.cs:46-50
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTD_CCtx_setParameter(self.cctx, int(parameter), int(value)))

    def GetParameter(self, parameter: int) -> int:            # S/Compressor.cs:52-57
        self._ensure_not_disposed()
        v = ctypes.c_int(0)
        ensure_zstd_success(self._lib, self._lib.ZSTD_CCtx_getParameter(self.cctx, int(parameter), ctypes.byref(v)))
        return v.value

    def LoadDictionary(self, dict_bytes):                     # S/Compressor.cs:36-43
        self._ensure_not_disposed()
        addr, n, keep = _as_buffer(dict_bytes if dict_bytes is not None else b"")
        self._release_prefix()          # (ZSTD_CCtx_loadDictionary cancels a pending prefix)
        self._cdict = None              # (and a referenced CDict)
        ensure_zstd_success(self._lib, self._lib.ZSTD_CCtx_loadDictionary(self.cctx, addr, n))

    def RefCDict(self, cdict):
        """ZSTD_CCtx_refCDict: compress against a digested dictionary (dictionaries.CDict) from now on, at ITS level; None = no
        dictionary.  Nothing is uploaded: the CDict is shared.  Cancels a loaded dictionary and a pending prefix.  The object is kept
        referenced here so that it cannot be collected while the context uses it."""
        self._ensure_not_disposed()
        if cdict is not None:
            cdict._ensure_not_disposed()
        self._release_prefix()
        ensure_zstd_success(self._lib, self._lib.ZSTD_CCtx_refCDict(self.cctx, cdict.handle if cdict is not None else None))
        self._cdict = cdict

    def WrapUsingCDict(self, src, cdict):
        """ZSTD_compress_usingCDict: src -> bytes, ONE call with the CDict's level and default frame parameters; this object's
        parameters, dictionary and reference are left as they are."""
        self._ensure_not_disposed()
        cdict._ensure_not_disposed()
        saddr, sn, skeep = _as_buffer(src)
        cap = self._wrap_bound(sn) if self._content_cuts else self.GetCompressBound(sn)
        out = ctypes.create_string_buffer(max(cap, 1))
        n = ensure_zstd_success(self._lib, self._lib.ZSTD_compress_usingCDict(self.cctx, out, cap, saddr, sn, cdict.handle))
        return out.raw[:n]

    def RefPrefix(self, prefix):
        """ZSTD_CCtx_refPrefix: the next Wrap / TryWrap compresses its source as a delta of `prefix` (bytes-like or a contiguous CUDA
        uint8 tensor; raw content whatever it starts with) and writes ONE frame, which decodes behind Decompressor.RefPrefix(prefix).
        Single use; cancels a loaded dictionary.  The object is referenced, not copied: it is kept alive here until the consuming
        call has returned and must not change before."""
        self._ensure_not_disposed()
        addr, n, keep, device = _as_prefix(prefix)
        self._release_prefix()
        self._cdict = None              # (ZSTD_CCtx_refPrefix cancels a referenced CDict)
        ensure_zstd_success(self._lib, self._lib.ZSTD_CCtx_refPrefix(self.cctx, addr, n))
        self._hold_prefix(keep, device)

    @staticmethod
    def GetCompressBound(length: int) -> int:                  # S/Compressor.cs:72-76
        return _ffi.load().ZSTD_compressBound(length)

    # ---- seek table (ZSTDMI_CCtx_setSeekTable): Wrap appends one, Decompressor.unwrap_range reads ranges through it ----
    @property
    def seek_table(self) -> bool:
        return self._seek_table

    @seek_table.setter
    def seek_table(self, on):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setSeekTable(self.cctx, 1 if on else 0))
        self._seek_table = bool(on)

    # ---- dictionary entropy tables (ZSTDMI_CCtx_setDictEntropy): code first blocks with a formatted dictionary's tables; off by default ----
    @property
    def dict_entropy(self) -> bool:
        return self._dict_entropy

    @dict_entropy.setter
    def dict_entropy(self, on):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setDictEntropy(self.cctx, 1 if on else 0))
        self._dict_entropy = bool(on)

    # ---- entropy state carried across blocks (ZSTDMI_CCtx_setEntropyCarry): later blocks of a frame may reuse the Huffman table, the FSE
    # tables and the repcodes of the blocks before them; off by default ----
    @property
    def entropy_carry(self) -> bool:
        return self._entropy_carry

    @entropy_carry.setter
    def entropy_carry(self, on):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setEntropyCarry(self.cctx, 1 if on else 0))
        self._entropy_carry = bool(on)

    # ---- dictionary index (ZSTDMI_CCtx_setDictIndex): the whole dictionary indexed once at upload, nothing staged per chunk; off by default ----
    @property
    def dict_index(self) -> bool:
        return self._dict_index

    @dict_index.setter
    def dict_index(self, on):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setDictIndex(self.cctx, 1 if on else 0))
        self._dict_index = bool(on)

    # ---- how far up the strategies dict_index reaches (ZSTDMI_CCtx_setDictIndexStrategy): 1 = fast only (default), 2 = also doubleFast (level 3) ----
    @property
    def dict_index_strategy(self) -> int:
        return self._dict_index_strategy

    @dict_index_strategy.setter
    def dict_index_strategy(self, max_strategy):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setDictIndexStrategy(self.cctx, int(max_strategy)))
        self._dict_index_strategy = int(max_strategy)

    # ---- dict_index for the chain finder, levels 5 and up (ZSTDMI_CCtx_setDictIndexChain); off by default ----
    @property
    def dict_index_chain(self) -> bool:
        return self._dict_index_chain

    @dict_index_chain.setter
    def dict_index_chain(self, on):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setDictIndexChain(self.cctx, 1 if on else 0))
        self._dict_index_chain = bool(on)

    # ---- one frame per Wrap and per stream session (ZSTDMI_CCtx_setSingleFrame), as the reference writes; off by default ----
    @property
    def single_frame(self) -> bool:
        return self._single_frame

    @single_frame.setter
    def single_frame(self, on):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setSingleFrame(self.cctx, 1 if on else 0))
        self._single_frame = bool(on)

    # ---- under single_frame, a long-distance window that slides with the frame (ZSTDMI_CCtx_setSlidingLdm); off by default ----
    @property
    def sliding_ldm(self) -> bool:
        return self._sliding_ldm

    @sliding_ldm.setter
    def sliding_ldm(self, on):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setSlidingLdm(self.cctx, 1 if on else 0))
        self._sliding_ldm = bool(on)

    # ---- offsets of 2^29 and more: RefPrefix up to prefix + source = 2^31, sliding_ldm at windowLog 29 and 30 (ZSTDMI_CCtx_setFarOffsets); off by default ----
    @property
    def far_offsets(self) -> bool:
        return self._far_offsets

    @far_offsets.setter
    def far_offsets(self, on):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setFarOffsets(self.cctx, 1 if on else 0))
        self._far_offsets = bool(on)

    # ---- content-defined cuts (ZSTDMI_CCtx_setContentCuts): 0 = off (default), 12 .. 16 = Wrap cuts its source by content, avgLog ----
    @property
    def content_cuts(self) -> int:
        return self._content_cuts

    @content_cuts.setter
    def content_cuts(self, avg_log):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_setContentCuts(self.cctx, int(avg_log)))
        self._content_cuts = int(avg_log)

    def _wrap_bound(self, length: int) -> int:
        """the room Wrap(src) without dest asks for: frames plus, where a switch adds one, the seek table"""
        if self._content_cuts:
            return ensure_zstd_success(self._lib, self._lib.ZSTDMI_contentCutsBound(length, self._content_cuts))
        return self.GetCompressBound(length) + (self._lib.ZSTDMI_seekTableBound(length) if self._seek_table else 0)

    # ---- batches enqueued from the device (ZSTDMI_CCtx_prepareBatchAsync; batch.compress_batch_async runs them) ----
    def PrepareBatchAsync(self, max_entries: int, src_size_bound: int):
        """Everything compress_batch_async needs the host for, once: resolves this object's parameters and dictionary for an entry of
        src_size_bound bytes, uploads the dictionary and sizes the workspaces for max_entries entries.  Any later SetParameter,
        LoadDictionary, RefCDict or switch invalidates it.  Raises ZstdException (parameter_unsupported) for what the one-block pass does
        not cover."""
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_prepareBatchAsync(self.cctx, int(max_entries), int(src_size_bound)))

    def PrepareBatchAsyncLimits(self, max_entries: int, src_size_bound: int, max_chunks: int = 0):
        """ZSTDMI_CCtx_prepareBatchAsyncLimits: PrepareBatchAsync for entries of up to 4 MiB - 1 bytes, cut into blocks on the device.
        max_chunks: the blocks one call may hold, all entries together (0 = max_entries entries of the bound, at most the pass limit);
        entries beyond it answer -66 (workSpace_tooSmall).  Replaces an earlier prepare of either kind.  Raises ZstdException
        (parameter_outOfBound, parameter_unsupported) as the header states."""
        self._ensure_not_disposed()
        lim = _ffi.CBatchLimits(int(max_entries), int(src_size_bound), int(max_chunks))
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_prepareBatchAsyncLimits(self.cctx, ctypes.byref(lim)))

    @property
    def batch_async_plan(self):
        """ZSTDMI_CCtx_getBatchAsyncPlan -> (chunk_bytes, frame_blocks, max_chunks) of the valid prepare; ZstdException (stage_wrong)
        without one."""
        self._ensure_not_disposed()
        cb, fb, mc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_getBatchAsyncPlan(self.cctx, ctypes.byref(cb), ctypes.byref(fb), ctypes.byref(mc)))
        return cb.value, fb.value, mc.value

    def pack_async_bound(self, n: int) -> int:
        """ZSTDMI_CCtx_packAsyncBound: the room with which batch.compress_pack_async of n entries never answers dstSize_tooSmall under
        the valid prepare (host arithmetic); ZstdException (stage_wrong) without one."""
        self._ensure_not_disposed()
        return ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_packAsyncBound(self.cctx, int(n)))

    prepare_batch_async, prepare_batch_async_limits = PrepareBatchAsync, PrepareBatchAsyncLimits

    # ---- cuts and digests enqueued from the device (ZSTDMI_CCtx_prepareCutsAsync; content_cuts_async runs them) ----
    def PrepareCutsAsync(self, src_size_bound: int, avg_log: int, kind=None, max_candidates: int = 0):
        """Everything content_cuts_async needs the host for, once: one workspace for sources of up to src_size_bound bytes (at most
        2^32 - 1) cut at avg_log, with digests of `kind` (None: none; "xxh64" / "sha256" or the ABI's integer) and room for
        max_candidates candidate ends (0: four times the expected count).  Independent of PrepareBatchAsync and of every parameter;
        a later PrepareCutsAsync replaces it.  Raises ZstdException (parameter_outOfBound, parameter_unsupported) as the header states."""
        self._ensure_not_disposed()
        lim = _ffi.CutLimits(int(src_size_bound), int(avg_log), 0 if kind is None else _digest_kind(kind), int(max_candidates))
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_prepareCutsAsync(self.cctx, ctypes.byref(lim)))

    def cuts_async_plan(self):
        """ZSTDMI_CCtx_getCutsAsyncPlan -> (max_pieces, max_candidates, digest_size) of the cuts prepare; ZstdException (stage_wrong)
        without one."""
        self._ensure_not_disposed()
        mp, mc, ds = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_CCtx_getCutsAsyncPlan(self.cctx, ctypes.byref(mp), ctypes.byref(mc), ctypes.byref(ds)))
        return mp.value, mc.value, ds.value

    prepare_cuts_async = PrepareCutsAsync

    # ---- Wrap (S/Compressor.cs:78-96) ----
    def Wrap(self, src, dest=None, offset: int = 0):
        """Wrap(src) -> bytes;  Wrap(src, dest[, offset]) -> number of bytes written into dest."""
        self._ensure_not_disposed()
        try:
            self._prefix_ready()
            return self._wrap(src, dest, offset)
        finally:
            self._release_prefix()      # (ZSTD_compress2 consumed it, whatever it returned)

    def _wrap(self, src, dest, offset):
        saddr, sn, skeep = _as_buffer(src)
        if dest is None:
            cap = self._wrap_bound(sn)
            out = ctypes.create_string_buffer(max(cap, 1))
            n = ensure_zstd_success(self._lib, self._lib.ZSTD_compress2(self.cctx, out, cap, saddr, sn))
            return out.raw[:n]
        daddr, dn, dkeep = _as_buffer(dest)
        if offset < 0 or offset > dn:
            raise ValueError("offset")
        return ensure_zstd_success(self._lib, self._lib.ZSTD_compress2(self.cctx, (daddr or 0) + offset if daddr else None, dn - offset, saddr, sn))

    def TryWrap(self, src, dest, offset: int = 0):             # S/Compressor.cs:98-122
        """-> (ok, written): ok is False exactly when dest is too small (ZSTD_error_dstSize_tooSmall)."""
        self._ensure_not_disposed()
        saddr, sn, skeep = _as_buffer(src)
        daddr, dn, dkeep = _as_buffer(dest)
        try:
            self._prefix_ready()
            r = self._lib.ZSTD_compress2(self.cctx, (daddr + offset) if daddr else None, dn - offset, saddr, sn)
        finally:
            self._release_prefix()
        if r == DST_SIZE_TOO_SMALL:
            return False, 0
        return True, ensure_zstd_success(self._lib, r)

    wrap, try_wrap, set_parameter, get_parameter, load_dictionary, ref_prefix = Wrap, TryWrap, SetParameter, GetParameter, LoadDictionary, RefPrefix
    ref_cdict, wrap_using_cdict = RefCDict, WrapUsingCDict

    # ---- lifetime (S/Compressor.cs:59-70, 124-147) ----
    def Dispose(self):
        if getattr(self, "cctx", None):
            self._lib.ZSTD_freeCCtx(self.cctx)
            self.cctx = None

    dispose = close = Dispose

    def _ensure_not_disposed(self):
        if not self.cctx:
            raise RuntimeError("ObjectDisposedException: Compressor")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Dispose()

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass


def _as_source(data):
    """bytes-like or a contiguous CUDA uint8 tensor (what torch has queued for it finished) -> (address, length, keepalive)"""
    if hasattr(data, "data_ptr"):
        import torch
        if not (data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()):
            raise TypeError("expected a contiguous CUDA uint8 tensor")
        torch.cuda.synchronize(data.device)
        return (data.data_ptr() if data.numel() else None), data.numel(), data
    return _as_buffer(data)


def content_cuts(compressor, data, avg_log: int):
    """ZSTDMI_contentCuts: the chunker alone -> the list of piece sizes the cut rule (include/zstd_mi355x.h "Content-defined cuts") gives
    `data` (bytes-like, or a contiguous CUDA uint8 tensor) at avg_log, in order; their sum is len(data).  The compressor lends its
    device and stream; its content_cuts switch is not consulted."""
    compressor._ensure_not_disposed()
    lib = compressor._lib
    addr, n, keep = _as_source(data)
    cap = n // 1024 + 1         # (min is 1 KiB or more: never fewer entries than pieces)
    sizes = (ctypes.c_size_t * cap)()
    got = ctypes.c_size_t(0)
    ensure_zstd_success(lib, lib.ZSTDMI_contentCuts(compressor.cctx, addr, n, int(avg_log), sizes, cap, ctypes.byref(got)))
    return list(sizes[:got.value])


DIGEST_KINDS = {"xxh64": 1, "sha256": 2}


def _digest_kind(kind) -> int:
    if isinstance(kind, str):
        if kind not in DIGEST_KINDS:
            raise ValueError(f"digest kind {kind!r}: expected one of {sorted(DIGEST_KINDS)}")
        return DIGEST_KINDS[kind]
    return int(kind)


def _split_digests(raw, count, each):
    return [raw[i * each:(i + 1) * each] for i in range(count)]


def piece_digests(compressor, data, sizes, kind="xxh64"):
    """ZSTDMI_digestPieces: the digest of every piece of `data` (bytes-like, or a contiguous CUDA uint8 tensor) -> a list of bytes, one
    per entry of `sizes`.  Piece i is the sizes[i] bytes behind piece i - 1; the sizes may add up to less than len(data), never to more.
    kind: "xxh64" (8 bytes, the value little-endian: its first four are zstd's frame checksum field), "sha256" (32 bytes, as
    hashlib.sha256(piece).digest()), or the ABI's integer.  The compressor lends its device and stream; none of its settings is
    consulted or changed."""
    compressor._ensure_not_disposed()
    lib = compressor._lib
    k = _digest_kind(kind)
    each = lib.ZSTDMI_digestSize(k)
    addr, n, keep = _as_source(data)
    sizes = [int(x) for x in sizes]
    arr = (ctypes.c_size_t * max(len(sizes), 1))(*sizes)
    out = ctypes.create_string_buffer(max(len(sizes) * each, 1))
    ensure_zstd_success(lib, lib.ZSTDMI_digestPieces(compressor.cctx, addr, n, arr, len(sizes), k, out, len(sizes) * each))
    return _split_digests(out.raw, len(sizes), each)


def content_cuts_digests(compressor, data, avg_log: int, kind="sha256"):
    """ZSTDMI_contentCutsDigests: content_cuts(compressor, data, avg_log) and the digest of every piece in one call, with no host round
    trip beyond the chunker's own -> (sizes, digests)."""
    compressor._ensure_not_disposed()
    lib = compressor._lib
    k = _digest_kind(kind)
    each = lib.ZSTDMI_digestSize(k)
    addr, n, keep = _as_source(data)
    cap = n // 1024 + 1         # (min is 1 KiB or more: never fewer entries than pieces)
    sizes = (ctypes.c_size_t * cap)()
    out = ctypes.create_string_buffer(max(cap * each, 1))
    got = ctypes.c_size_t(0)
    ensure_zstd_success(lib, lib.ZSTDMI_contentCutsDigests(compressor.cctx, addr, n, int(avg_log), k, sizes, cap, ctypes.byref(got), out, cap * each))
    return list(sizes[:got.value]), _split_digests(out.raw, got.value, each)
