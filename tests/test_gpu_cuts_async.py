"""GPU tests of the enqueued cuts (include/zstd_mi355x.h "Cuts and digests enqueued from the device"; content_cuts_async.hip): sizes,
sources and digests in device memory against the numpy restatement of the rule (content_cuts_cases), hashlib's SHA-256 and the oracle's
XXH64; planted edges, small sources, crafted candidate lists through the selection alone; the capacity rule and the candidate room;
a call that neither waits nor allocates; the calls around it left as they were; and the pieces handed to compress_pack_async as they
stand.  Every output lies inside a 0xA5-filled tensor, and nothing outside the first n_pieces elements may change."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import content_cuts_cases as cc
import cuts_async_cases as ca
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

pytestmark = pytest.mark.gpu

E = ZSTD_ErrorCode
DIGEST_SIZE = {None: 0, "xxh64": 8, "sha256": 32}
PAD = 64
MIB = 1 << 20


def on_device(data, shift=0):
    """the bytes in device memory, `shift` bytes behind an allocation's start"""
    import torch
    t = torch.empty(len(data) + shift + 8, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return t[shift:shift + len(data)]


class Guarded:
    """`count` elements of `width` bytes inside a 0xA5-filled tensor with PAD guard bytes on either side"""

    def __init__(self, count, width):
        import torch
        self.count, self.width = count, width
        self.full = torch.full((2 * PAD + count * width,), 0xA5, dtype=torch.uint8, device="cuda")
        body = self.full[PAD:PAD + count * width]
        self.view = body.view(torch.int64) if width == 8 else body

    def check(self, used):
        """-> the first `used` elements' bytes; everything else must still be 0xA5"""
        raw = self.full.cpu().numpy()
        lo, hi = PAD, PAD + used * self.width
        assert (raw[:lo] == 0xA5).all() and (raw[hi:] == 0xA5).all(), "bytes outside the first n_pieces elements changed"
        return raw[lo:hi]


class Outputs:
    def __init__(self, capacity, kind, digest_bytes=None):
        each = DIGEST_SIZE[kind]
        self.each = each
        self.sizes, self.srcs = Guarded(capacity, 8), Guarded(capacity, 8)
        self.digests = Guarded(capacity * each if digest_bytes is None else digest_bytes, 1) if each else None

    def run(self, c, src):
        """-> (n_pieces, status) read back behind a synchronise"""
        import torch
        n, st, _, _, _ = z.content_cuts_async(c, src, self.sizes.view, self.srcs.view, self.digests.view if self.digests else None)
        torch.cuda.synchronize()
        return int(n.item()), int(st.item())

    def untouched(self):
        self.sizes.check(0), self.srcs.check(0)
        if self.digests:
            self.digests.check(0)

    def pieces(self, n, src):
        """-> (sizes, digests) of the first n pieces; the sources must be src + the running sum"""
        sizes = self.sizes.check(n).view(np.int64).tolist()
        srcs = self.srcs.check(n).view(np.int64).tolist()
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if n else []
        assert srcs == [src.data_ptr() + int(s) for s in starts]
        raw = self.digests.check(n * self.each).tobytes() if self.digests else b""
        return sizes, [raw[i * self.each:(i + 1) * self.each] for i in range(n)] if self.each else None


@functools.lru_cache(maxsize=None)
def want_sizes(kind, n, avg_log):
    return tuple(cc.piece_sizes(cc.base(kind)[:n], avg_log))


_want_digests = {}


def want_digests(dkind, data, sizes, oracle, key):
    if dkind is None:
        return None
    if (dkind, key) not in _want_digests:
        out, at = [], 0
        for s in sizes:
            piece = data[at:at + s]
            out.append(hashlib.sha256(piece).digest() if dkind == "sha256" else int(oracle.lib().zso_xxh64(piece, len(piece), 0)).to_bytes(8, "little"))
            at += s
        _want_digests[(dkind, key)] = out
    return _want_digests[(dkind, key)]


# ---- 1. sizes, sources and digests against the restatement ----
@pytest.mark.parametrize("avg_log", cc.AVG_LOGS)
@pytest.mark.parametrize("kind", ["rand", "text", "zipf", "mixed", "flat"])
def test_against_the_restatement(gpu_lib, oracle, kind, avg_log):
    n = 300000 if kind == "flat" else MIB
    data = cc.base(kind)[:n]
    want = list(want_sizes(kind, n, avg_log))
    srcs = [on_device(data, shift) for shift in (0, 1, 3)]          # both load paths of the mark kernel
    assert [t.data_ptr() % 4 for t in srcs] == [0, 1, 3]
    with z.Compressor(1) as c:
        for dkind in (None, "xxh64", "sha256"):
            c.PrepareCutsAsync(MIB, avg_log, dkind)
            max_pieces, max_cand, each = c.cuts_async_plan()
            assert (max_pieces, max_cand, each) == (MIB // cc.min_of(avg_log) + 1, 4 * (MIB >> (avg_log - 1)) + 1024, DIGEST_SIZE[dkind])
            wd = want_digests(dkind, data, want, oracle, (kind, n, avg_log))
            for src in srcs:
                out = Outputs(max_pieces, dkind)
                got_n, status = out.run(c, src)
                assert (got_n, status) == (len(want), 0)
                sizes, digests = out.pieces(got_n, src)
                assert sizes == want and digests == wd


# ---- 2. planted edges ----
@pytest.mark.parametrize("name,avg_log", [(name, 12) for name in cc.PLANTED] + [("min-1", 16), ("max+1", 16), ("desert", 16)])
def test_planted_cases(gpu_lib, name, avg_log):
    # (content_cuts_cases.planted cannot build the three avgLog 16 cases from its 300 000 bytes: cuts_async_cases.planted_wide)
    data = cc.planted(name, avg_log) if avg_log == 12 else ca.planted_wide(name, avg_log)
    want = cc.piece_sizes(data, avg_log)
    src = on_device(data)
    with z.Compressor(1) as c:
        c.PrepareCutsAsync(len(data), avg_log)
        out = Outputs(c.cuts_async_plan()[0], None)
        got_n, status = out.run(c, src)
        assert (got_n, status) == (len(want), 0)
        assert out.pieces(got_n, src)[0] == want


# ---- 3. small sources on a prepare whose bound is larger ----
@pytest.mark.parametrize("avg_log,dkind", [(12, "sha256"), (16, "xxh64")])
def test_small_sources(gpu_lib, oracle, avg_log, dkind):
    mn = cc.min_of(avg_log)
    base = cc.base("text")
    with z.Compressor(1) as c:
        c.PrepareCutsAsync(MIB, avg_log, dkind)
        cap = c.cuts_async_plan()[0]
        for n in (0, 1, 63, 64, 65, mn - 1, mn, mn + 1, 16383, 16384, 16385, 65535, 65536, 65537):
            data = base[:n]
            want = list(want_sizes("text", n, avg_log))
            src = on_device(data)
            out = Outputs(cap, dkind)
            got_n, status = out.run(c, src)
            assert (got_n, status) == (len(want), 0), n
            if n == 0:
                out.untouched()
                continue
            sizes, digests = out.pieces(got_n, src)
            assert sizes == want and digests == want_digests(dkind, data, want, oracle, ("text", n, avg_log)), n


# ---- 4. crafted candidate lists through the selection alone ----
def select_parallel(lib, cctx, case, slack=8):
    n, avg_log, cands = case
    want = ca.expected(case)
    cap = len(want) + slack
    arr = (ctypes.c_uint * max(len(cands), 1))(*cands)
    ends = (ctypes.c_uint * cap)(*([0xA5A5A5A5] * cap))
    got = ctypes.c_size_t(0)
    r = lib.ZSTDMI_debugCutSelectParallel(cctx, arr, len(cands), n, avg_log, ends, cap, ctypes.byref(got))
    assert r == 0, (n, avg_log, get_error_code(r))
    out = np.ctypeslib.as_array(ends)
    assert (out[got.value:] == 0xA5A5A5A5).all()
    return out[:got.value].tolist(), want


def test_crafted_lists(gpu_lib):
    with z.Compressor(1) as c:
        cases = ca.crafted() + (ca.clusters(),) + tuple(x for x in ca.real() if x[0] in (65537, 200000))
        assert any(x[0] == ca.TOP for x in cases)
        for case in cases:
            got, want = select_parallel(gpu_lib, c.cctx, case)
            assert got == want, (case[0], case[1], len(case[2]))
        # one end short: the true count, nothing written
        case = ca.crafted()[0]
        want = ca.expected(case)
        ends, got = (ctypes.c_uint * len(want))(*([7] * len(want))), ctypes.c_size_t(0)
        arr = (ctypes.c_uint * len(case[2]))(*case[2])
        r = gpu_lib.ZSTDMI_debugCutSelectParallel(c.cctx, arr, len(case[2]), case[0], case[1], ends, len(want) - 1, ctypes.byref(got))
        assert is_error(r) and get_error_code(r) == E.ZSTD_error_dstSize_tooSmall and got.value == len(want) and list(ends) == [7] * len(want)


# ---- 5. capacities and the candidate room ----
def test_capacities(gpu_lib):
    data = cc.base("rand")
    want = list(want_sizes("rand", MIB, 12))
    src = on_device(data)
    with z.Compressor(1) as c:
        c.PrepareCutsAsync(MIB, 12, "sha256")
        for out in (Outputs(len(want) - 1, "sha256"), Outputs(len(want), "sha256", 32 * len(want) - 1)):
            got_n, status = out.run(c, src)
            assert (got_n, status) == (len(want), -E.ZSTD_error_dstSize_tooSmall)
            out.untouched()
        out = Outputs(len(want), "sha256")                   # exactly enough of both
        assert out.run(c, src) == (len(want), 0) and out.pieces(len(want), src)[0] == want
        # a room of 16 candidates: refused on the device, the count 0
        c.PrepareCutsAsync(MIB, 12, "sha256", 16)
        assert c.cuts_async_plan()[1] == 16 and len(cc.candidates(data, 12)) > 16
        out = Outputs(len(want), "sha256")
        assert out.run(c, src) == (0, -E.ZSTD_error_workSpace_tooSmall)
        out.untouched()
        # the same context, room again: the refused call left nothing behind
        c.PrepareCutsAsync(MIB, 12, "sha256")
        out = Outputs(len(want), "sha256")
        assert out.run(c, src) == (len(want), 0) and out.pieces(len(want), src)[0] == want


# ---- 6. no stops ----
def test_no_host_waits_no_allocations_and_back_to_back_calls(gpu_lib):
    import torch
    a, b = cc.base("text"), cc.base("zipf")[:700001]
    wa, wb = list(want_sizes("text", MIB, 12)), list(want_sizes("zipf", 700001, 12))
    sa, sb = on_device(a), on_device(b)
    with z.Compressor(1) as c:
        c.PrepareCutsAsync(MIB, 12, "xxh64")
        cap = c.cuts_async_plan()[0]
        outs = [Outputs(cap, "xxh64") for _ in range(3)]
        torch.cuda.synchronize()
        # (the wrapper's own two 1-element tensors come from torch's allocator, not from the library)
        waits, allocs = gpu_lib.ZSTDMI_debugHostWaits(c.cctx), gpu_lib.ZSTDMI_debugDeviceAllocs(c.cctx)
        res = []
        for out, src in zip(outs, (sa, sb, sa)):            # back to back, no synchronise between them
            res.append(z.content_cuts_async(c, src, out.sizes.view, out.srcs.view, out.digests.view))
        assert (gpu_lib.ZSTDMI_debugHostWaits(c.cctx), gpu_lib.ZSTDMI_debugDeviceAllocs(c.cctx)) == (waits, allocs)
        torch.cuda.synchronize()
        for (n, st, _, _, _), out, src, want in zip(res, outs, (sa, sb, sa), (wa, wb, wa)):
            assert (int(n.item()), int(st.item())) == (len(want), 0)
            assert out.pieces(len(want), src)[0] == want
        # tensors allocated from the plan
        n, st, sizes, srcs, digests = z.content_cuts_async(c, sb)
        torch.cuda.synchronize()
        assert int(st.item()) == 0 and sizes[:int(n.item())].tolist() == wb and sizes.numel() == srcs.numel() == cap and digests.numel() == 8 * cap


# ---- 7. neighbours ----
def test_neighbours(gpu_lib):
    import torch
    data = cc.base("mixed")
    want = list(want_sizes("mixed", MIB, 12))
    src = on_device(data)
    with z.Compressor(1) as c:
        # without a prepare
        with pytest.raises(z.ZstdException) as e:
            z.content_cuts_async(c, src)
        assert e.value.code == E.ZSTD_error_stage_wrong
        c.PrepareCutsAsync(MIB, 12, "sha256")
        cap = c.cuts_async_plan()[0]
        # a synchronous fused call, a parameter setter and a batch prepare in between change nothing
        sync_sizes, sync_digests = z.content_cuts_digests(c, src, 12, "sha256")
        assert sync_sizes == want
        c.SetParameter(100, 3)                               # ZSTD_c_compressionLevel
        c.PrepareBatchAsync(8, 65536)
        out = Outputs(cap, "sha256")
        assert out.run(c, src) == (len(want), 0)
        sizes, digests = out.pieces(len(want), src)
        assert sizes == want and digests == sync_digests
        # the batch prepare is still served behind the cuts prepare and the cuts call
        items = [on_device(data[i * 60000:(i + 1) * 60000]) for i in range(8)]
        srcs = torch.tensor([t.data_ptr() for t in items], dtype=torch.int64, device="cuda")
        lens = torch.tensor([t.numel() for t in items], dtype=torch.int64, device="cuda")
        bound = gpu_lib.ZSTD_compressBound(65536)
        dst = torch.empty(8 * bound, dtype=torch.uint8, device="cuda")
        dsts = torch.tensor([dst.data_ptr() + i * bound for i in range(8)], dtype=torch.int64, device="cuda")
        caps = torch.full((8,), bound, dtype=torch.int64, device="cuda")
        got = z.compress_batch_async(c, srcs, lens, dsts, caps)
        torch.cuda.synchronize()
        with z.Decompressor() as d:
            for i, size in enumerate(got.tolist()):
                assert size > 0 and d.Unwrap(dst[i * bound:i * bound + size].cpu().numpy().tobytes()) == data[i * 60000:(i + 1) * 60000]
        # above the bound, and a digest array against the prepared kind
        with pytest.raises(z.ZstdException) as e:
            z.content_cuts_async(c, on_device(data + b"x"))
        assert e.value.code == E.ZSTD_error_srcSize_wrong
        a = out.sizes.view.data_ptr()
        r = gpu_lib.ZSTDMI_contentCutsAsync(c.cctx, src.data_ptr(), MIB, a, None, cap, None, 0, a, a)
        assert is_error(r) and get_error_code(r) == E.ZSTD_error_GENERIC
        # ZSTDMI_CCtx_setDevice drops it
        assert gpu_lib.ZSTDMI_CCtx_setDevice(c.cctx, 0) == 0
        with pytest.raises(z.ZstdException) as e:
            z.content_cuts_async(c, src)
        assert e.value.code == E.ZSTD_error_stage_wrong
        with pytest.raises(z.ZstdException) as e:
            c.cuts_async_plan()
        assert e.value.code == E.ZSTD_error_stage_wrong


def test_several_workers_are_refused_behind_the_limits(gpu_lib):
    lim = z._ffi.CutLimits
    c = gpu_lib.ZSTD_createCCtx()
    try:
        assert gpu_lib.ZSTDMI_CCtx_setDevices(c, (ctypes.c_int * 2)(0, 0), 2) == 0
        r = gpu_lib.ZSTDMI_CCtx_prepareCutsAsync(c, ctypes.byref(lim(0, 12, 0, 0)))
        assert is_error(r) and get_error_code(r) == E.ZSTD_error_parameter_outOfBound
        r = gpu_lib.ZSTDMI_CCtx_prepareCutsAsync(c, ctypes.byref(lim(MIB, 12, 0, 0)))
        assert is_error(r) and get_error_code(r) == E.ZSTD_error_parameter_unsupported
    finally:
        gpu_lib.ZSTD_freeCCtx(c)


# ---- 8. the pieces as a pack's entries ----
def test_flow_into_compress_pack_async(gpu_lib):
    import torch
    data = cc.base("text")
    want = list(want_sizes("text", MIB, 12))
    src = on_device(data)
    with z.Compressor(1) as c, z.Decompressor() as d:
        c.PrepareCutsAsync(MIB, 12)
        n, st, sizes, srcs, _ = z.content_cuts_async(c, src)
        count = int(n.item())                                # (the one read the flow needs: the entry count is a host argument)
        assert int(st.item()) == 0 and count == len(want)
        c.PrepareBatchAsync(count, 65536)
        dst = torch.empty(c.pack_async_bound(count), dtype=torch.uint8, device="cuda")
        size = z.compress_pack_async(c, srcs[:count], sizes[:count], dst)       # the returned tensors themselves
        torch.cuda.synchronize()
        stream = dst[:int(size.item())].cpu().numpy().tobytes()
        assert int(size.item()) > 0 and d.Unwrap(stream) == data
        rows = z.read_seek_table(stream)[0]
        at = 0
        for piece in want:                                  # the rows' content sizes add up, piece by piece
            got = 0
            while got < piece:
                got += rows[at][1]
                at += 1
            assert got == piece
        assert at == len(rows)
