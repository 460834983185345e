"""Range reads of a seekable stream against what a caller does without a seek table (run on the GPU box): a 1 GiB stream of Zipf bytes
at level 1 (64 KiB frames) and of text at level 3 (240 KiB frames), ranges of 64 KiB, 1 MiB, 16 MiB and 256 MiB at unaligned offsets.
Per point:
  (a) full + slice : one ZSTDMI_decompressDevice (device source) / ZSTD_decompressDCtx (host source, device destination) of the
                     whole stream, then a device copy of the range — the only way to a range without the table
  (b) range        : one ZSTDMI_decompressRange into a device destination, from the device source and from the host source
  (c) the range call's stage times (ZSTDMI_DCtx_getStageTimes) and its diagnostics (frames decoded, bytes staged)
Best of 3 after a warm-up call of the same shape; the host clock stops after the call's final synchronise (every call ends with one).
The input is 64 MiB of generated data repeated (frames are independent, so the repeats are nobody's match).
python tools/range_time.py [MiB]"""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen
lib = z._ffi.load()
MiB = 1 << 20
total = (int(sys.argv[1]) if len(sys.argv) > 1 else 1024) * MiB
PIECE = min(64 * MiB, total)


def stage_times(get, ctx):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = get(ctx, ms, names, 24)
    return " ".join(f"{names[i].decode()} {float(ms[i]):.2f}" for i in range(k))


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


print(f"{total // MiB} MiB of content per stream; ms per read (GB/s of the bytes returned)", flush=True)
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
    full = torch.empty(total, dtype=torch.uint8, device="cuda")
    d = lib.ZSTD_createDCtx()
    for length in (64 << 10, MiB, 16 * MiB, 256 * MiB):
        if length >= total:
            continue
        offset = (total // 3 | 1) + 12345                  # odd, inside a frame
        out = torch.empty(length, dtype=torch.uint8, device="cuda")

        def full_dev():
            ok(lib.ZSTDMI_decompressDevice(d, full.data_ptr(), total, comp.data_ptr(), csize))
            out.copy_(full[offset:offset + length]); torch.cuda.synchronize()

        def full_host():
            ok(lib.ZSTD_decompressDCtx(d, full.data_ptr(), total, hptr, csize))
            out.copy_(full[offset:offset + length]); torch.cuda.synchronize()

        def range_dev():
            assert ok(lib.ZSTDMI_decompressRange(d, out.data_ptr(), length, comp.data_ptr(), csize, offset, length)) == length

        def range_host():
            assert ok(lib.ZSTDMI_decompressRange(d, out.data_ptr(), length, hptr, csize, offset, length)) == length

        fd, fh = best_of(full_dev), best_of(full_host)
        lib.ZSTDMI_DCtx_setProfiling(d, 1)
        rd = best_of(range_dev)
        assert bool(torch.equal(out, src[offset:offset + length]))
        stages = stage_times(lib.ZSTDMI_DCtx_getStageTimes, d)
        frames = lib.ZSTDMI_debugLastRangeFrames(d)
        out.zero_()
        rh = best_of(range_host)
        assert bool(torch.equal(out, src[offset:offset + length]))
        staged = lib.ZSTDMI_debugLastRangeStaged(d)
        lib.ZSTDMI_DCtx_setProfiling(d, 0)
        gbs = lambda t: length / t / 1e9
        print(f"| {kind} L{level} | {length // 1024:6d} KiB | {frames:5d} | {fd * 1e3:8.2f} | {rd * 1e3:7.3f} ({gbs(rd):6.2f}) | {fd / rd:6.1f}x "
              f"| {fh * 1e3:8.2f} | {rh * 1e3:7.3f} ({gbs(rh):6.2f}) | {fh / rh:6.1f}x | {staged:10d} |", flush=True)
        print(f"    range stages ms (device source): {stages}", flush=True)
        del out
    lib.ZSTD_freeDCtx(d)
    del src, comp, full
    torch.cuda.empty_cache()
