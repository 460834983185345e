"""Gather reads against a loop of single range calls (run on the GPU box): a 1 GiB stream of Zipf bytes at level 1 (64 KiB frames) and
of text at level 3 (240 KiB frames); n = 256, 4096 and 65 536 seeded random ranges of 4 KiB and of 64 KiB at unaligned offsets, device
and host source, device destinations.  Per point:
  (a) gather : ONE ZSTDMI_decompressRanges over the n ranges
  (b) loop   : ZSTDMI_decompressRange once per range — timed on the first 256 ranges in the same run and scaled to n
  (c) full   : one ZSTDMI_decompressDevice of the whole stream (what a reader without a table pays, whatever n is)
and, for one point per stream, the gather call's stage times and diagnostics.  Best of 3 after a warm-up call of the same shape; the
host clock stops after the call's final synchronise (every call ends with one).  The input is 64 MiB of generated data repeated
(frames are independent, so the repeats are nobody's match).
python tools/ranges_time.py [MiB]
python tools/ranges_time.py --async [MiB]: instead, the same streams (device source) and the 4 KiB ranges through ZSTDMI_decompressRangesAsync,
prepared with limits of exactly what each call touches.  Per point: (a) the time until the call has returned, (b) until the stream has
drained, (c) ZSTDMI_decompressRanges with the same ranges as host arrays (the yardstick, which ends with its own synchronise)."""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen
lib = z._ffi.load()
MiB = 1 << 20
ASYNC = "--async" in sys.argv
ARGS = [a for a in sys.argv[1:] if a != "--async"]
total = (int(ARGS[0]) if ARGS else 1024) * MiB
PIECE = min(64 * MiB, total)
LOOP = 256


def stage_times(get, ctx):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = get(ctx, ms, names, 24)
    return " ".join(f"{names[i].decode()} {float(ms[i]):.3f}" for i in range(k))


def best_of(f, reps=3):
    f()                                     # warm-up: same shape, workspaces allocated
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        best = min(best, time.perf_counter() - t0)
    return best


def ok(r):
    assert not lib.ZSTD_isError(r), lib.ZSTD_getErrorName(r)
    return r


def async_points(kind, level, src, comp, csize, entries, d):
    """the --async table's rows for one stream; d: the context of the yardstick"""
    length = 4 << 10
    d_at = np.concatenate([[0], np.cumsum([dd for _, dd in entries], dtype=np.int64)])
    da = lib.ZSTD_createDCtx()
    for n in (256, 4096, 65536):
        rng = np.random.default_rng(1000 + n + length)
        offs_np = rng.integers(0, total - length, n, dtype=np.int64) | 1
        first = np.searchsorted(d_at, offs_np, side="right") - 1
        last = np.searchsorted(d_at, offs_np + length - 1, side="right") - 1
        touched = np.unique(np.concatenate([np.arange(f, l + 1) for f, l in zip(first.tolist(), last.tolist())]))
        touched = [int(j) for j in touched if entries[j][1]]
        content = sum(entries[j][1] for j in touched)
        lim = z._ffi.DRangesLimits(n, length, content, len(touched), 0, 0)       # 1x what the call touches
        torch.cuda.synchronize()
        ok(lib.ZSTDMI_DCtx_prepareRangesAsync(da, comp.data_ptr(), csize, ctypes.byref(lim)))
        out = torch.empty(n * length + 64, dtype=torch.uint8, device="cuda")
        offs_t = torch.from_numpy(offs_np).cuda()
        lens_t = torch.full((n,), length, dtype=torch.int64, device="cuda")
        dsts_t = out.data_ptr() + 1 + torch.arange(n, dtype=torch.int64, device="cuda") * length
        got_t = torch.zeros(n, dtype=torch.int64, device="cuda")
        ok(lib.ZSTDMI_DCtx_setStream(da, torch.cuda.current_stream().cuda_stream or 1))
        call = lambda: ok(lib.ZSTDMI_decompressRangesAsync(da, offs_t.data_ptr(), lens_t.data_ptr(), n, dsts_t.data_ptr(), lens_t.data_ptr(), got_t.data_ptr()))
        call(); torch.cuda.synchronize()                                         # warm-up
        t_ret = t_drain = 1e9
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            call(); t1 = time.perf_counter()
            torch.cuda.synchronize(); t2 = time.perf_counter()
            t_ret, t_drain = min(t_ret, t1 - t0), min(t_drain, t2 - t0)
        assert bool((got_t == length).all())
        for i in (0, n // 2, n - 1):
            o = int(offs_np[i])
            assert bool(torch.equal(out[1 + i * length:1 + (i + 1) * length], src[o:o + length]))
        offs = (ctypes.c_ulonglong * n)(*offs_np.tolist())
        lens = (ctypes.c_size_t * n)(*([length] * n))
        dsts = (ctypes.c_void_p * n)(*[out.data_ptr() + 1 + i * length for i in range(n)])
        got = (ctypes.c_size_t * n)()
        t_sync = best_of(lambda: ok(lib.ZSTDMI_decompressRanges(d, comp.data_ptr(), csize, offs, lens, n, dsts, lens, got)))
        assert all(g == length for g in got) and lib.ZSTDMI_debugLastRangesFrames(d) == len(touched)
        print(f"| {kind} L{level} | {n:6d} | {len(touched):6d} | {t_ret * 1e3:9.3f} | {t_drain * 1e3:9.3f} | {t_sync * 1e3:9.3f} | {t_sync / t_drain:5.2f}x |", flush=True)
        del out
    lib.ZSTD_freeDCtx(da)


print(f"{total // MiB} MiB of content per stream; ms per n ranges (GB/s of the bytes returned)", flush=True)
if ASYNC:
    print("| stream | n ranges of 4 KiB | frames touched | (a) call returned ms | (b) stream drained ms | (c) ZSTDMI_decompressRanges ms | (c) / (b) |", flush=True)
else:
    print("| stream | range | n | source | frames | gather ms (GB/s) | loop ms (GB/s) | loop / gather | full ms | staged B |", flush=True)
for kind, level in (("zipf", 1), ("text", 3)):
    src = torch.from_numpy(np.frombuffer(datagen.gen(kind, PIECE, 5), dtype=np.uint8).copy()).cuda().repeat(total // PIECE)
    cap = lib.ZSTD_compressBound(total) + lib.ZSTDMI_seekTableBound(total)
    comp = torch.empty(cap, dtype=torch.uint8, device="cuda")
    c = lib.ZSTD_createCCtx()
    lib.ZSTD_CCtx_setParameter(c, 100, level)
    ok(lib.ZSTDMI_CCtx_setSeekTable(c, 1))
    torch.cuda.synchronize()
    csize = ok(lib.ZSTDMI_compressDevice(c, comp.data_ptr(), cap, src.data_ptr(), total))
    lib.ZSTD_freeCCtx(c)
    comp = comp[:csize].clone()
    host = comp.cpu().numpy().tobytes()
    hptr = ctypes.cast(ctypes.c_char_p(host), ctypes.c_void_p).value
    entries, table_bytes = z.read_seek_table(host)
    print(f"{kind} L{level}: {csize} compressed bytes, {len(entries)} frames of {entries[0][1] // 1024} KiB, table {table_bytes} B", flush=True)
    if ASYNC:
        d = lib.ZSTD_createDCtx()
        async_points(kind, level, src, comp, csize, entries, d)
        lib.ZSTD_freeDCtx(d)
        del src, comp
        torch.cuda.empty_cache()
        continue
    full = torch.empty(total, dtype=torch.uint8, device="cuda")
    d = lib.ZSTD_createDCtx()
    t_full = best_of(lambda: ok(lib.ZSTDMI_decompressDevice(d, full.data_ptr(), total, comp.data_ptr(), csize)))
    del full
    torch.cuda.empty_cache()
    for length in (4 << 10, 64 << 10):
        for n in (256, 4096, 65536):
            rng = np.random.default_rng(1000 + n + length)
            offs_np = rng.integers(0, total - length, n, dtype=np.int64) | 1            # odd: inside a frame, unaligned
            out = torch.empty(n * length + 64, dtype=torch.uint8, device="cuda")
            offs = (ctypes.c_ulonglong * n)(*offs_np.tolist())
            lens = (ctypes.c_size_t * n)(*([length] * n))
            dsts = (ctypes.c_void_p * n)(*[out.data_ptr() + 1 + i * length for i in range(n)])
            got = (ctypes.c_size_t * n)()
            for source, sptr in (("device", comp.data_ptr()), ("host", hptr)):
                def gather():
                    ok(lib.ZSTDMI_decompressRanges(d, sptr, csize, offs, lens, n, dsts, lens, got))

                def loop():
                    for i in range(LOOP):
                        ok(lib.ZSTDMI_decompressRange(d, dsts[i], length, sptr, csize, offs[i], length))

                show = n == 4096 and source == "device"
                if show:
                    lib.ZSTDMI_DCtx_setProfiling(d, 1)
                tg = best_of(gather)
                stages = stage_times(lib.ZSTDMI_DCtx_getStageTimes, d) if show else ""
                lib.ZSTDMI_DCtx_setProfiling(d, 0)
                assert all(g == length for g in got)
                for i in (0, n // 2, n - 1):
                    o = int(offs_np[i])
                    assert bool(torch.equal(out[1 + i * length:1 + (i + 1) * length], src[o:o + length]))
                frames, staged = lib.ZSTDMI_debugLastRangesFrames(d), lib.ZSTDMI_debugLastRangesStaged(d)
                tl = best_of(loop) * (n / LOOP)
                gbs = lambda t: n * length / t / 1e9
                print(f"| {kind} L{level} | {length // 1024:3d} KiB | {n:6d} | {source:6s} | {frames:6d} | {tg * 1e3:9.3f} ({gbs(tg):6.2f}) | {tl * 1e3:10.1f} ({gbs(tl):5.2f}) "
                      f"| {tl / tg:7.1f}x | {t_full * 1e3:8.2f} | {staged:11d} |", flush=True)
                if show:
                    print(f"    gather stages ms: {stages}", flush=True)
            del out
    lib.ZSTD_freeDCtx(d)
    del src, comp
    torch.cuda.empty_cache()
