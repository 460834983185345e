"""Many small buffers in one call (ZSTDMI_compressBatch / ZSTDMI_decompressBatch, include/zstd_mi355x.h): every item is compressed as
Compressor.Wrap would compress it alone — a complete stream that decodes on its own — and decoded as Decompressor.Unwrap would decode
it, but the items share one pass through the GPU pipeline.  compress_pack (ZSTDMI_compressPack) writes the items as ONE seekable
stream instead: the same frames side by side, one seek table behind them; pack_ranges names record i for Decompressor.unwrap_ranges.

torch is imported inside the functions: the package imports without it.
"""
import ctypes

from . import _ffi
from .errors import ZstdException, get_error_code, is_error


_HIP_STREAM_LEGACY = 1       # hipStreamLegacy (hip_runtime_api.h): the null stream, named explicitly


def _pointer_array(values):
    return (ctypes.c_void_p * len(values))(*values)


def _size_array(values):
    return (ctypes.c_size_t * len(values))(*values)


def _gather(torch, items):
    """-> (tensors?, device, sizes, source pointers, keepalive)"""
    tensors = all(isinstance(x, torch.Tensor) for x in items)
    if tensors:
        for i, t in enumerate(items):
            if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
                raise TypeError(f"item {i}: expected a contiguous CUDA uint8 tensor")
        return True, items[0].device, [t.numel() for t in items], [t.data_ptr() if t.numel() else None for t in items], items
    if any(isinstance(x, torch.Tensor) for x in items):
        raise TypeError("items must be all tensors or all bytes-like")
    views = [memoryview(x).cast("B") for x in items]
    sizes = [len(v) for v in views]
    device = torch.device("cuda", torch.cuda.current_device())
    flat = torch.frombuffer(bytearray(b"".join(views)) or bytearray(1), dtype=torch.uint8).to(device)      # one upload
    srcs, at = [], 0
    for s in sizes:
        srcs.append(flat.data_ptr() + at if s else None)
        at += s
    return False, device, sizes, srcs, flat


def _run(torch, lib, call, ctx, device, srcs, sizes, caps, tensors):
    n = len(sizes)
    starts, at = [], 0
    for c in caps:
        starts.append(at)
        at += c
    out = torch.empty(max(at, 1), dtype=torch.uint8, device=device)
    got = (ctypes.c_size_t * n)()
    torch.cuda.synchronize(device)          # the library runs on a stream of its own
    r = call(ctx, _pointer_array(srcs), _size_array(sizes), n, _pointer_array([out.data_ptr() + s for s in starts]), _size_array(caps), got)
    if is_error(r):
        raise ZstdException(get_error_code(r), lib.ZSTD_getErrorName(r).decode())
    for i in range(n):
        if is_error(got[i]):
            raise ZstdException(get_error_code(got[i]), f"item {i}: {lib.ZSTD_getErrorName(got[i]).decode()}")
    if tensors:
        return [out[starts[i]:starts[i] + got[i]] for i in range(n)]
    host = out.cpu().numpy().tobytes()
    return [host[starts[i]:starts[i] + got[i]] for i in range(n)]


def decompress_batch(decompressor, items, sizes):
    """items as for compress_batch, each a complete compressed stream; sizes[i] = room for item i's content (its decompressed size, or
    more).  -> a list of CUDA uint8 tensors or of bytes.  Uses the decompressor's dictionary.  An item that fails — damaged, or larger
    than sizes[i] — raises ZstdException naming its index."""
    import torch
    decompressor._ensure_not_disposed()
    lib = decompressor._lib
    items, sizes = list(items), [int(x) for x in sizes]
    if len(items) != len(sizes):
        raise ValueError("one size per item")
    if not items:
        return []
    tensors, device, src_sizes, srcs, keep = _gather(torch, items)
    out = _run(torch, lib, lib.ZSTDMI_decompressBatch, decompressor.dctx, device, srcs, src_sizes, sizes, tensors)
    del keep
    return out


def compress_batch(compressor, items, cdicts=None):
    """items: a list of torch CUDA uint8 tensors (-> a list of CUDA uint8 tensors, views of one buffer) or of bytes-like objects
    (uploaded in one copy -> a list of bytes).  Uses the compressor's level, parameters and dictionary.  An item that fails raises
    ZstdException naming its index.
    cdicts (ZSTDMI_compressBatchCDicts): one dictionaries.CDict or None per item.  Item i is then written as after RefCDict(cdicts[i]) —
    at that CDict's level, behind it alone, None = no dictionary — whatever dictionary the compressor itself holds, and items behind
    different CDicts share passes.  The CDicts stay referenced until the call returns."""
    import torch
    compressor._ensure_not_disposed()
    lib = compressor._lib
    items = list(items)
    n = len(items)
    if cdicts is not None:
        cdicts = list(cdicts)
        if len(cdicts) != n:
            raise ValueError("one CDict (or None) per item")
        for d in cdicts:
            if d is not None:
                d._ensure_not_disposed()
    if n == 0:
        return []
    tensors, device, sizes, srcs, keep = _gather(torch, items)
    call = lib.ZSTDMI_compressBatch
    if cdicts is not None:
        handles = _pointer_array([d.handle if d is not None else None for d in cdicts])

        def call(ctx, srcs_, sizes_, n_, dsts_, caps_, got_):
            return lib.ZSTDMI_compressBatchCDicts(ctx, srcs_, sizes_, n_, dsts_, caps_, got_, handles)
    out = _run(torch, lib, call, compressor.cctx, device, srcs, sizes, [lib.ZSTD_compressBound(x) for x in sizes], tensors)
    del keep, cdicts
    return out


def compress_batch_async(compressor, srcs, sizes, dsts, caps, out_sizes=None):
    """ZSTDMI_compressBatchAsync after Compressor.PrepareBatchAsync or PrepareBatchAsyncLimits: srcs, sizes, dsts, caps are contiguous
    CUDA int64 tensors of n entries each (pointers as integers, e.g. base.data_ptr() + offsets computed on the device) -> out_sizes, a CUDA int64 tensor: entry
    i's compressed size, or its zstd error code as a negative value (-70 dstSize_tooSmall, -72 srcSize_wrong, -74 dstBuffer_null; after
    Compressor.PrepareBatchAsyncLimits also -66 workSpace_tooSmall for an entry beyond the prepared max_chunks).
    The work is enqueued on torch.cuda.current_stream() and the call returns: nothing is synchronised and nothing is copied to the
    host, so out_sizes and the destinations are for work queued on that stream behind it.  The tensors, the sources and the
    destinations must stay alive and unchanged until that stream has passed the work.  Raises ZstdException for the whole call's
    error (stage_wrong: no valid PrepareBatchAsync, more entries than it was prepared for, or a parameter changed since)."""
    import torch
    compressor._ensure_not_disposed()
    lib = compressor._lib
    n = sizes.numel()
    if out_sizes is None:
        out_sizes = torch.empty(n, dtype=torch.int64, device=sizes.device)
    for name, t in (("srcs", srcs), ("sizes", sizes), ("dsts", dsts), ("caps", caps), ("out_sizes", out_sizes)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == n):
            raise TypeError(f"{name}: expected a contiguous CUDA int64 tensor of {n} entries")
    if n == 0:
        return out_sizes
    stream = torch.cuda.current_stream(sizes.device)
    # (torch's default stream is the null stream, which ZSTDMI_CCtx_setStream reads as "the context's own": hipStreamLegacy names it)
    r = lib.ZSTDMI_CCtx_setStream(compressor.cctx, stream.cuda_stream or _HIP_STREAM_LEGACY)
    if not is_error(r):
        r = lib.ZSTDMI_compressBatchAsync(compressor.cctx, srcs.data_ptr(), sizes.data_ptr(), n, dsts.data_ptr(), caps.data_ptr(), out_sizes.data_ptr())
    if is_error(r):
        raise ZstdException(get_error_code(r), lib.ZSTD_getErrorName(r).decode())
    return out_sizes


def decompress_batch_async(decompressor, srcs, sizes, dsts, caps, out_sizes=None):
    """ZSTDMI_decompressBatchAsync after Decompressor.PrepareBatchAsync: srcs, sizes, dsts, caps are contiguous CUDA int64 tensors of n
    entries each (pointers as integers; `sizes` may be the out_sizes tensor compress_batch_async has just written) -> out_sizes, a CUDA
    int64 tensor: entry i's content size, or its zstd error code as a negative value (what decompress_batch raises for it; -72
    srcSize_wrong also for a size above the prepared bound, which is what a negative size reads as; -66 workSpace_tooSmall for an entry
    beyond a prepared limit).  The work is enqueued on torch.cuda.current_stream() and the call returns: nothing is synchronised and
    nothing is copied to the host.  The tensors, the sources and the destinations must stay alive and unchanged until that stream has
    passed the work.  Raises ZstdException for the whole call's error (stage_wrong: no valid PrepareBatchAsync, more entries than it
    was prepared for, or a parameter or the dictionary changed since)."""
    import torch
    decompressor._ensure_not_disposed()
    lib = decompressor._lib
    n = sizes.numel()
    if out_sizes is None:
        out_sizes = torch.empty(n, dtype=torch.int64, device=sizes.device)
    for name, t in (("srcs", srcs), ("sizes", sizes), ("dsts", dsts), ("caps", caps), ("out_sizes", out_sizes)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == n):
            raise TypeError(f"{name}: expected a contiguous CUDA int64 tensor of {n} entries")
    if n == 0:
        return out_sizes
    stream = torch.cuda.current_stream(sizes.device)
    r = lib.ZSTDMI_DCtx_setStream(decompressor.dctx, stream.cuda_stream or _HIP_STREAM_LEGACY)
    if not is_error(r):
        r = lib.ZSTDMI_decompressBatchAsync(decompressor.dctx, srcs.data_ptr(), sizes.data_ptr(), n, dsts.data_ptr(), caps.data_ptr(), out_sizes.data_ptr())
    if is_error(r):
        raise ZstdException(get_error_code(r), lib.ZSTD_getErrorName(r).decode())
    return out_sizes


def decompress_ranges_async(decompressor, offsets, lengths, dsts, caps, out_sizes=None):
    """ZSTDMI_decompressRangesAsync after Decompressor.PrepareRangesAsync: offsets, lengths, dsts, caps are contiguous CUDA int64
    tensors of n ranges each of the prepared stream's content (dsts: pointers as integers, 0 = none; all of them e.g. computed on the
    device from an index tensor) -> out_sizes, a CUDA int64 tensor: the bytes range i returned, or its zstd error code as a negative
    value (what unwrap_ranges raises for it; -66 workSpace_tooSmall for a range longer than the prepared max_range_bytes or one that
    meets a frame beyond a prepared limit; -72 srcSize_wrong for one that meets a frame of more than 4 MiB compressed).  The work is
    enqueued on torch.cuda.current_stream() and the call returns: nothing is synchronised and nothing is copied to the host.  The
    tensors and the destinations must stay alive and unchanged until that stream has passed the work.  Raises ZstdException for the
    whole call's error (stage_wrong: no valid PrepareRangesAsync, more ranges than it was prepared for, or a parameter or the
    dictionary changed since)."""
    import torch
    decompressor._ensure_not_disposed()
    lib = decompressor._lib
    n = offsets.numel()
    if out_sizes is None:
        out_sizes = torch.empty(n, dtype=torch.int64, device=offsets.device)
    for name, t in (("offsets", offsets), ("lengths", lengths), ("dsts", dsts), ("caps", caps), ("out_sizes", out_sizes)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == n):
            raise TypeError(f"{name}: expected a contiguous CUDA int64 tensor of {n} entries")
    if n == 0:
        return out_sizes
    stream = torch.cuda.current_stream(offsets.device)
    r = lib.ZSTDMI_DCtx_setStream(decompressor.dctx, stream.cuda_stream or _HIP_STREAM_LEGACY)
    if not is_error(r):
        r = lib.ZSTDMI_decompressRangesAsync(decompressor.dctx, offsets.data_ptr(), lengths.data_ptr(), n, dsts.data_ptr(), caps.data_ptr(), out_sizes.data_ptr())
    if is_error(r):
        raise ZstdException(get_error_code(r), lib.ZSTD_getErrorName(r).decode())
    return out_sizes


def compress_pack(compressor, items):
    """items as for compress_batch -> ONE seekable stream (ZSTDMI_compressPack): item i's frames as Compressor.Wrap writes them for it
    alone, one item's behind the other's, and one seek table behind the last (read_seek_table reads it).  Bytes-like items -> bytes;
    CUDA uint8 tensors -> one CUDA uint8 tensor of exactly the stream's length.  An empty list is the 17-byte empty table.  Uses the
    compressor's level, parameters and dictionary; its seek_table switch is not consulted."""
    import torch
    compressor._ensure_not_disposed()
    lib = compressor._lib
    items = list(items)
    n = len(items)
    if n:
        tensors, device, sizes, srcs, keep = _gather(torch, items)
    else:
        tensors, device, sizes, srcs, keep = False, torch.device("cuda", torch.cuda.current_device()), [], [], None
    cap = lib.ZSTDMI_packBound(_size_array(sizes), n)
    if is_error(cap):
        raise ZstdException(get_error_code(cap), lib.ZSTD_getErrorName(cap).decode())
    out = torch.empty(cap, dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)          # the library runs on a stream of its own
    r = lib.ZSTDMI_compressPack(compressor.cctx, out.data_ptr(), cap, _pointer_array(srcs), _size_array(sizes), n)
    del keep
    if is_error(r):
        raise ZstdException(get_error_code(r), lib.ZSTD_getErrorName(r).decode())
    return out[:r] if tensors else out[:r].cpu().numpy().tobytes()


def compress_pack_async(compressor, srcs, sizes, dst, out_size=None, entry_ends=None):
    """ZSTDMI_compressPackAsync after Compressor.PrepareBatchAsync or PrepareBatchAsyncLimits: srcs, sizes are contiguous CUDA int64
    tensors of n entries each (pointers as integers), dst a contiguous CUDA uint8 tensor whose numel() is the capacity
    (Compressor.pack_async_bound(n) always suffices) -> out_size, a 1-element CUDA int64 tensor: the length of the seekable stream
    written at dst — entry i's frames as compress_batch_async writes them, one entry's behind the other's, and one seek table — or
    the ONE error of the call as a negative value (-72 srcSize_wrong, -66 workSpace_tooSmall: the lowest failing entry's answer; else
    -70 dstSize_tooSmall), in which case nothing of dst has been written.  entry_ends (optional, a CUDA int64 tensor of n entries)
    receives the offset at which each entry's frames end; it is left alone on an error.
    The work is enqueued on torch.cuda.current_stream() and the call returns: nothing is synchronised and nothing is copied to the
    host.  The tensors and the sources must stay alive and unchanged until that stream has passed the work.  Raises ZstdException for
    the call's own error (stage_wrong: no valid prepare, more entries than it was prepared for, or a parameter changed since)."""
    import torch
    compressor._ensure_not_disposed()
    lib = compressor._lib
    n = sizes.numel() if isinstance(sizes, torch.Tensor) else -1
    for name, t in (("srcs", srcs), ("sizes", sizes)) + ((("entry_ends", entry_ends),) if entry_ends is not None else ()):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == n):
            raise TypeError(f"{name}: expected a contiguous CUDA int64 tensor of {n} entries")
    if not (isinstance(dst, torch.Tensor) and dst.is_cuda and dst.dtype == torch.uint8 and dst.is_contiguous()):
        raise TypeError("dst: expected a contiguous CUDA uint8 tensor")
    if out_size is None:
        out_size = torch.empty(1, dtype=torch.int64, device=dst.device)
    if not (isinstance(out_size, torch.Tensor) and out_size.is_cuda and out_size.dtype == torch.int64 and out_size.is_contiguous() and out_size.numel() == 1):
        raise TypeError("out_size: expected a contiguous CUDA int64 tensor of 1 entry")
    stream = torch.cuda.current_stream(dst.device)
    # (torch's default stream is the null stream, which ZSTDMI_CCtx_setStream reads as "the context's own": hipStreamLegacy names it)
    r = lib.ZSTDMI_CCtx_setStream(compressor.cctx, stream.cuda_stream or _HIP_STREAM_LEGACY)
    if not is_error(r):
        r = lib.ZSTDMI_compressPackAsync(compressor.cctx, dst.data_ptr() if dst.numel() else None, dst.numel(), srcs.data_ptr() if n else None,
                                         sizes.data_ptr() if n else None, n, out_size.data_ptr(), entry_ends.data_ptr() if entry_ends is not None and n else None)
    if is_error(r):
        raise ZstdException(get_error_code(r), lib.ZSTD_getErrorName(r).decode())
    return out_size


def content_cuts_async(compressor, src, sizes=None, srcs=None, digests=None):
    """ZSTDMI_contentCutsAsync after Compressor.PrepareCutsAsync: the pieces of `src` (a contiguous CUDA uint8 tensor of at most the
    prepared bound) by the cut rule, and their digests where the prepare asked for a kind, all in device memory ->
    (n_pieces, status, sizes, srcs, digests): n_pieces and status 1-element CUDA int64 tensors (status 0, or the call's zstd error code
    as a negative value: -70 dstSize_tooSmall — n_pieces is then still the true count —, -66 workSpace_tooSmall: more candidates than
    the prepared room); sizes and srcs CUDA int64 tensors whose first n_pieces entries are the pieces' sizes and addresses — the
    `sizes` and `srcs` compress_batch_async and compress_pack_async take —; digests a CUDA uint8 tensor, n_pieces digests side by side
    (None without a kind).  Tensors not given are allocated from the plan (max_pieces entries); given ones state the capacity by their
    numel().  The work is enqueued on torch.cuda.current_stream() and the call returns: nothing is synchronised and nothing is copied
    to the host.  Every tensor and `src` must stay alive and unchanged until that stream has passed the work.  Raises ZstdException for
    the call's own error (stage_wrong: no PrepareCutsAsync; srcSize_wrong: src above the bound)."""
    import torch
    compressor._ensure_not_disposed()
    lib = compressor._lib
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()):
        raise TypeError("src: expected a contiguous CUDA uint8 tensor")
    max_pieces, _, each = compressor.cuts_async_plan()
    dev = src.device
    if sizes is None:
        sizes = torch.empty(max_pieces, dtype=torch.int64, device=dev)
    if srcs is None:
        srcs = torch.empty(sizes.numel(), dtype=torch.int64, device=dev)
    if digests is None and each:
        digests = torch.empty(sizes.numel() * each, dtype=torch.uint8, device=dev)
    for name, t in (("sizes", sizes), ("srcs", srcs)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()):
            raise TypeError(f"{name}: expected a contiguous CUDA int64 tensor")
    if srcs.numel() != sizes.numel():
        raise TypeError("srcs: expected as many entries as sizes")
    if digests is not None and not (isinstance(digests, torch.Tensor) and digests.is_cuda and digests.dtype == torch.uint8 and digests.is_contiguous()):
        raise TypeError("digests: expected a contiguous CUDA uint8 tensor")
    n_pieces = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)
    r = lib.ZSTDMI_CCtx_setStream(compressor.cctx, stream.cuda_stream or _HIP_STREAM_LEGACY)
    if not is_error(r):
        cap = sizes.numel()
        r = lib.ZSTDMI_contentCutsAsync(compressor.cctx, src.data_ptr() if src.numel() else None, src.numel(), sizes.data_ptr() if cap else None,
                                        srcs.data_ptr() if cap else None, cap, digests.data_ptr() if digests is not None else None,
                                        digests.numel() if digests is not None else 0, n_pieces.data_ptr(), status.data_ptr())
    if is_error(r):
        raise ZstdException(get_error_code(r), lib.ZSTD_getErrorName(r).decode())
    return n_pieces, status, sizes, srcs, digests


def pack_ranges(sizes):
    """-> [(offset, length), ...] for Decompressor.unwrap_ranges: record i of a pack whose items had these sizes."""
    ranges, at = [], 0
    for s in sizes:
        ranges.append((at, int(s)))
        at += int(s)
    return ranges
