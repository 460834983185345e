"""Mirror of ZstdSharp.Decompressor (S/Decompressor.cs) over libzstd_mi355x.so."""
import ctypes

from . import _ffi
from .compressor import _PrefixHolder, _as_buffer, _as_prefix
from .errors import DST_SIZE_TOO_SMALL, ZstdException, ZSTD_ErrorCode, ensure_content_size_ok, ensure_zstd_success, get_error_code, is_error


# ZSTD_DCtx_setParameter's parameters (include/zstd_mi355x.h) and the values of ZSTD_d_refMultipleDDicts
ZSTD_d_windowLogMax = 100
ZSTD_d_refMultipleDDicts = 1003
ZSTD_rmd_refSingleDDict = 0
ZSTD_rmd_refMultipleDDicts = 1


class Decompressor(_PrefixHolder):
    """S/Decompressor.cs:7-148."""

    def __init__(self, device: int = None):
        self._lib = _ffi.load()
        self.dctx = self._lib.ZSTD_createDCtx()          # S/Decompressor.cs:12
        if not self.dctx:
            raise MemoryError("ZSTD_createDCtx")
        self._stream_segment = 0
        self._batch_unsized = False
        self._ddict = None              # the DDict RefDDict holds
        self._ddict_set = {}            # ZSTD_d_refMultipleDDicts: dictID -> every DDict the context's set references (until Dispose)
        self._ranges_stream = None      # the tensor PrepareRangesAsync opened
        if device is not None:
            ensure_zstd_success(self._lib, self._lib.ZSTDMI_DCtx_setDevice(self.dctx, device))

    def SetParameter(self, parameter: int, value: int):      # S/Decompressor.cs:39-43
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTD_DCtx_setParameter(self.dctx, int(parameter), int(value)))

    def GetParameter(self, parameter: int) -> int:            # S/Decompressor.cs:45-50
        self._ensure_not_disposed()
        v = ctypes.c_int(0)
        ensure_zstd_success(self._lib, self._lib.ZSTD_DCtx_getParameter(self.dctx, int(parameter), ctypes.byref(v)))
        return v.value

    @property
    def stream_segment(self) -> int:
        """ZSTDMI_DCtx_setStreamSegment: the compressed size at which DecompressionStream / ZSTD_decompressStream cut a frame that is
        still arriving into segments and hand their content out; 0 (the default) = whole frames only."""
        return self._stream_segment

    @stream_segment.setter
    def stream_segment(self, nbytes: int):
        self._ensure_not_disposed()
        if nbytes < 0:
            raise ValueError("stream_segment must not be negative")
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_DCtx_setStreamSegment(self.dctx, int(nbytes)))
        self._stream_segment = int(nbytes)

    # ---- frames without a content size in the shared pass of decompress_batch / unwrap_range(s) (ZSTDMI_DCtx_setBatchUnsized); off by default ----
    @property
    def batch_unsized(self) -> bool:
        return self._batch_unsized

    @batch_unsized.setter
    def batch_unsized(self, on):
        self._ensure_not_disposed()
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_DCtx_setBatchUnsized(self.dctx, 1 if on else 0))
        self._batch_unsized = bool(on)

    # ---- batches enqueued from the device (ZSTDMI_DCtx_prepareBatchAsync; batch.decompress_batch_async runs them) ----
    def PrepareBatchAsync(self, max_entries: int, src_size_bound: int, max_content: int, max_frames: int = 0, max_blocks: int = 0,
                          max_sequences: int = 0):
        """Everything decompress_batch_async needs the host for, once: binds the device, uploads the dictionary in force (loaded,
        RefDDict, the ZSTD_d_refMultipleDDicts set) and sizes every work buffer for calls of at most max_entries entries of at most
        src_size_bound compressed bytes each (1 .. 4 MiB) that regenerate at most max_content bytes together.  max_frames (0 =
        max_entries), max_blocks (0 = max_frames + max_content / 16384, enough for every stream this library writes) and max_sequences
        (0 = max_content / 3 + 64, exact for valid input) bound the call's frames, blocks and sequence records; an entry beyond a limit
        answers workSpace_tooSmall (-66).  Any later setter, LoadDictionary, RefDDict or RefPrefix invalidates the prepare."""
        self._ensure_not_disposed()
        lim = _ffi.DBatchLimits(int(max_entries), int(src_size_bound), int(max_content), int(max_frames), int(max_blocks), int(max_sequences))
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_DCtx_prepareBatchAsync(self.dctx, ctypes.byref(lim)))

    prepare_batch_async = PrepareBatchAsync

    # ---- gather reads enqueued from the device (ZSTDMI_DCtx_prepareRangesAsync; batch.decompress_ranges_async runs them) ----
    def PrepareRangesAsync(self, stream_tensor, max_ranges: int, max_range_bytes: int, max_content: int, max_frames: int = 0, max_blocks: int = 0,
                           max_sequences: int = 0):
        """Everything decompress_ranges_async needs the host for, once, for ONE seekable stream (a contiguous CUDA uint8 tensor, kept
        referenced here until the next prepare or Dispose; its bytes must not change): binds the device, uploads the dictionary in
        force, reads and indexes the stream's seek table (a damaged table raises here, with unwrap_ranges' code) and sizes every work
        buffer for calls of at most max_ranges ranges of at most max_range_bytes returned bytes each (1 .. 4 MiB) that touch frames of
        at most max_content bytes of content together.  max_frames (0 = the table's entry count), max_blocks and max_sequences (0 =
        PrepareBatchAsync's defaults) bound the touched frames, their blocks and sequence records; a range beyond a limit answers
        workSpace_tooSmall (-66).  Replaces a PrepareBatchAsync and is replaced by one; any later setter, LoadDictionary, RefDDict or
        RefPrefix invalidates it."""
        self._ensure_not_disposed()
        import torch
        self._ranges_stream = None
        t = stream_tensor
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise TypeError("expected a contiguous CUDA uint8 tensor")
        lim = _ffi.DRangesLimits(int(max_ranges), int(max_range_bytes), int(max_content), int(max_frames), int(max_blocks), int(max_sequences))
        torch.cuda.synchronize(t.device)        # (the prepare reads the stream on the context's stream)
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_DCtx_prepareRangesAsync(self.dctx, t.data_ptr() if t.numel() else None, t.numel(), ctypes.byref(lim)))
        self._ranges_stream = t

    prepare_ranges_async = PrepareRangesAsync

    @property
    def ranges_async_plan(self):
        """(table_entries, total_content) of the stream the valid PrepareRangesAsync opened (ZSTDMI_DCtx_getRangesAsyncPlan)."""
        self._ensure_not_disposed()
        n, total = ctypes.c_size_t(0), ctypes.c_ulonglong(0)
        ensure_zstd_success(self._lib, self._lib.ZSTDMI_DCtx_getRangesAsyncPlan(self.dctx, ctypes.byref(n), ctypes.byref(total)))
        return n.value, total.value

    def LoadDictionary(self, dict_bytes):                     # S/Decompressor.cs:29-36
        self._ensure_not_disposed()
        addr, n, keep = _as_buffer(dict_bytes if dict_bytes is not None else b"")
        self._release_prefix()          # (ZSTD_DCtx_loadDictionary cancels a pending prefix)
        self._ddict = None              # (and a referenced DDict)
        ensure_zstd_success(self._lib, self._lib.ZSTD_DCtx_loadDictionary(self.dctx, addr, n))

    def RefDDict(self, ddict):
        """ZSTD_DCtx_refDDict: decode behind a digested dictionary (dictionaries.DDict) from now on; None = no dictionary.  Nothing is
        uploaded: the DDict is shared.  Cancels a loaded dictionary and a pending prefix.  The object is kept referenced here so that
        it cannot be collected while the context uses it."""
        self._ensure_not_disposed()
        if ddict is not None:
            ddict._ensure_not_disposed()
        self._release_prefix()
        multiple = ddict is not None and self.GetParameter(ZSTD_d_refMultipleDDicts) == ZSTD_rmd_refMultipleDDicts
        ensure_zstd_success(self._lib, self._lib.ZSTD_DCtx_refDDict(self.dctx, ddict.handle if ddict is not None else None))
        self._ddict = ddict
        if multiple:                    # the context's set took it (an equal dictID replaced): none may be collected while it may be selected
            self._ddict_set[ddict.dict_id] = ddict

    def UnwrapUsingDDict(self, src, ddict, maxDecompressedSize: int = (1 << 31) - 1):
        """ZSTD_decompress_usingDDict: src -> bytes, ONE call behind the DDict; this object's dictionary or reference is left as it is."""
        self._ensure_not_disposed()
        ddict._ensure_not_disposed()
        saddr, sn, skeep = _as_buffer(src)
        expected = self.GetDecompressedSize(src)
        if expected > maxDecompressedSize:
            raise ZstdException(ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall, f"Decompressed content size {expected} is greater than {maxDecompressedSize}")
        out = ctypes.create_string_buffer(max(expected, 1))
        n = ensure_zstd_success(self._lib, self._lib.ZSTD_decompress_usingDDict(self.dctx, out, expected, saddr, sn, ddict.handle))
        return out.raw[:n]

    def RefPrefix(self, prefix):
        """ZSTD_DCtx_refPrefix: the next Unwrap / TryUnwrap decodes its frames behind `prefix` (bytes-like or a contiguous CUDA uint8
        tensor, read where it lies) — the prefix Compressor.RefPrefix was given.  Single use; cancels a loaded dictionary.  The object is
        kept alive here until the consuming call has returned and must not change before."""
        self._ensure_not_disposed()
        addr, n, keep, device = _as_prefix(prefix)
        self._release_prefix()
        self._ddict = None              # (ZSTD_DCtx_refPrefix cancels a referenced DDict)
        ensure_zstd_success(self._lib, self._lib.ZSTD_DCtx_refPrefix(self.dctx, addr, n))
        self._hold_prefix(keep, device)

    @staticmethod
    def GetDecompressedSize(src) -> int:                      # S/Decompressor.cs:50-54
        addr, n, keep = _as_buffer(src)
        return ensure_content_size_ok(_ffi.load().ZSTD_decompressBound(addr, n))

    def Unwrap(self, src, dest=None, offset: int = 0, maxDecompressedSize: int = (1 << 31) - 1):
        """Unwrap(src[, maxDecompressedSize=..]) -> bytes;  Unwrap(src, dest[, offset]) -> bytes written (S/Decompressor.cs:56-88)."""
        self._ensure_not_disposed()
        try:
            self._prefix_ready()
            return self._unwrap(src, dest, offset, maxDecompressedSize)
        finally:
            self._release_prefix()      # (ZSTD_decompressDCtx consumed it, whatever it returned)

    def _unwrap(self, src, dest, offset, maxDecompressedSize):
        saddr, sn, skeep = _as_buffer(src)
        if dest is None:
            expected = self.GetDecompressedSize(src)
            if expected > maxDecompressedSize:
                raise ZstdException(ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall,
                                    f"Decompressed content size {expected} is greater than {maxDecompressedSize}")
            out = ctypes.create_string_buffer(max(expected, 1))
            n = ensure_zstd_success(self._lib, self._lib.ZSTD_decompressDCtx(self.dctx, out, expected, saddr, sn))
            return out.raw[:n]          # new Span<byte>(dest, 0, length): `expected` is a bound, not a promise (S/Decompressor.cs:63-75)
        daddr, dn, dkeep = _as_buffer(dest)
        return ensure_zstd_success(self._lib, self._lib.ZSTD_decompressDCtx(self.dctx, (daddr + offset) if daddr else None, dn - offset, saddr, sn))

    def TryUnwrap(self, src, dest, offset: int = 0):          # S/Decompressor.cs:90-111
        self._ensure_not_disposed()
        saddr, sn, skeep = _as_buffer(src)
        daddr, dn, dkeep = _as_buffer(dest)
        try:
            self._prefix_ready()
            r = self._lib.ZSTD_decompressDCtx(self.dctx, (daddr + offset) if daddr else None, dn - offset, saddr, sn)
        finally:
            self._release_prefix()
        if r == DST_SIZE_TOO_SMALL:
            return False, 0
        return True, ensure_zstd_success(self._lib, r)

    def unwrap_range(self, src, offset: int, length: int):
        """content[offset : offset + length] of a seekable stream (one that ends in a seek table: Compressor.seek_table) — only the
        frames that meet the range are decoded.  src: bytes-like -> bytes; a contiguous CUDA uint8 tensor -> a CUDA uint8 tensor.
        A range that runs past the end is clipped; one that starts there is empty."""
        self._ensure_not_disposed()
        if offset < 0 or length < 0:
            raise ValueError("offset and length must not be negative")
        lib = self._lib
        if hasattr(src, "data_ptr"):
            import torch
            if not (src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()):
                raise TypeError("expected a contiguous CUDA uint8 tensor")
            out = torch.empty(max(length, 1), dtype=torch.uint8, device=src.device)
            torch.cuda.synchronize(src.device)          # the library runs on a stream of its own
            n = ensure_zstd_success(lib, lib.ZSTDMI_decompressRange(self.dctx, out.data_ptr(), length, src.data_ptr() if src.numel() else None,
                                                                    src.numel(), offset, length))
            return out[:n]
        saddr, sn, skeep = _as_buffer(src)
        out = ctypes.create_string_buffer(max(length, 1))
        n = ensure_zstd_success(lib, lib.ZSTDMI_decompressRange(self.dctx, out, length, saddr, sn, offset, length))
        return out.raw[:n]

    def unwrap_ranges(self, src, ranges):
        """[content[o : o + l] for (o, l) in ranges] of a seekable stream in ONE call (ZSTDMI_decompressRanges): every frame that some
        range meets is decoded once, however many ranges meet it.  src: bytes-like -> a list of bytes; a contiguous CUDA uint8 tensor
        -> a list of CUDA uint8 tensors (slices of one buffer).  Ranges may overlap, repeat and come in any order; one that runs past
        the end is clipped.  A range that fails raises ZstdException naming its index."""
        self._ensure_not_disposed()
        import torch
        from .seekable import read_seek_table
        ranges = [(int(o), int(l)) for o, l in ranges]
        if any(o < 0 or l < 0 for o, l in ranges):
            raise ValueError("offset and length must not be negative")
        lib, n = self._lib, len(ranges)
        on_device = hasattr(src, "data_ptr")
        if on_device:
            if not (src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()):
                raise TypeError("expected a contiguous CUDA uint8 tensor")
            size, device = src.numel(), src.device
            # only the stream's tail comes back: the 9-byte footer says how long the table is
            foot = bytes(src[max(size - 9, 0):].cpu().numpy())
            tail = foot
            if size >= 17 and foot[5:] == bytes([0xB1, 0xEA, 0x92, 0x8F]):
                count, stride = int.from_bytes(foot[:4], "little"), 12 if foot[4] & 0x80 else 8
                if count <= (1 << 27) and 17 + count * stride <= size:
                    tail = bytes(src[size - (17 + count * stride):].cpu().numpy())
            entries, _ = read_seek_table(tail, front=size - len(tail))
            saddr, sn, skeep = (src.data_ptr() if size else None), size, src
        else:
            saddr, sn, skeep = _as_buffer(src)
            entries, _ = read_seek_table(src)
            device = torch.device("cuda", torch.cuda.current_device())
        if n == 0:
            return []
        total = sum(d for _, d in entries)
        want = [min(l, max(total - o, 0)) for o, l in ranges]
        starts, at = [], 0
        for w in want:
            starts.append(at)
            at += w
        out = torch.empty(max(at, 1), dtype=torch.uint8, device=device)
        base = out.data_ptr()
        offsets = (ctypes.c_ulonglong * n)(*[o for o, _ in ranges])
        lengths = (ctypes.c_size_t * n)(*[l for _, l in ranges])
        dsts = (ctypes.c_void_p * n)(*[(base + s) if w else None for s, w in zip(starts, want)])
        caps = (ctypes.c_size_t * n)(*want)
        got = (ctypes.c_size_t * n)()
        torch.cuda.synchronize(device)          # the library runs on a stream of its own
        ensure_zstd_success(lib, lib.ZSTDMI_decompressRanges(self.dctx, saddr, sn, offsets, lengths, n, dsts, caps, got))
        for i in range(n):
            if is_error(got[i]):
                raise ZstdException(get_error_code(got[i]), f"range {i}: {lib.ZSTD_getErrorName(got[i]).decode()}")
        if on_device:
            return [out[s:s + g] for s, g in zip(starts, got)]
        host = out.cpu().numpy().tobytes()      # one download for all ranges
        return [host[s:s + g] for s, g in zip(starts, got)]

    unwrap, try_unwrap, set_parameter, get_parameter, load_dictionary, get_decompressed_size, ref_prefix = \
        Unwrap, TryUnwrap, SetParameter, GetParameter, LoadDictionary, GetDecompressedSize, RefPrefix
    ref_ddict, unwrap_using_ddict = RefDDict, UnwrapUsingDDict

    def Dispose(self):                                        # S/Decompressor.cs:113-147
        if getattr(self, "dctx", None):
            self._lib.ZSTD_freeDCtx(self.dctx)
            self.dctx = None
            self._ddict = None
            self._ddict_set = {}        # (the set went with the context: its DDicts are the caller's again)
            self._ranges_stream = None  # (freeing the context waited for its work in flight)

    dispose = close = Dispose

    def _ensure_not_disposed(self):
        if not self.dctx:
            raise RuntimeError("ObjectDisposedException: Decompressor")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Dispose()

    def __del__(self):
        try:
            self.Dispose()
        except Exception:
            pass
