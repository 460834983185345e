"""Delta compression (ZSTD_CCtx_refPrefix / ZSTD_DCtx_refPrefix), run on the GPU box: a new version against the old one.  Inputs are
device-resident; every figure is the best of 3 after a warm-up, the host clock stopped after the final synchronise.  Per case: ratio,
compress GB/s, decompress GB/s with long frames forced to walk (ZSTDMI_DCtx_setLongFrames(1)) and to origin (2), stage times.
Cases: an old version of [MiB] (default 256) and a new version of [MiB] - 64 KiB = the old one with seeded edits (replace / insert /
delete spans), kinds rand, Zipf and text at levels 1 and 3; the same new version with long-distance matching and no prefix; one
16 MiB + 16 MiB text case.  python tools/prefix_time.py [MiB] [edits]"""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen
lib = z._ffi.load()
MiB = 1 << 20
big = (int(sys.argv[1]) if len(sys.argv) > 1 else 256) * MiB
edits = int(sys.argv[2]) if len(sys.argv) > 2 else 2000


def distinct(kind, n, seed):
    """n bytes in pieces of 64 MiB, each with a seed of its own (nothing repeats inside a version)"""
    return np.concatenate([np.frombuffer(datagen.gen(kind, min(64 * MiB, n - k), seed + k // MiB), dtype=np.uint8) for k in range(0, n, 64 * MiB)])


def edited(old, seed, count, n):
    """the first n bytes of: old with `count` seeded edits at ascending places, each a span of 1..2000 bytes replaced by random bytes,
    that many random bytes inserted, or the span deleted"""
    rng = np.random.default_rng(seed)
    at = np.sort(rng.integers(0, len(old) - 4096, count))
    parts, pos = [], 0
    for p in at:
        p = int(p)
        if p < pos:
            continue
        span, kind = int(rng.integers(1, 2001)), int(rng.integers(0, 3))
        parts.append(old[pos:p])
        if kind != 2:
            parts.append(rng.integers(0, 256, span, dtype=np.uint8))
        pos = p if kind == 1 else p + span
    parts.append(old[pos:])
    return np.concatenate(parts)[:n]


def stage_times(get, ctx):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = get(ctx, ms, names, 24)
    return {names[i].decode(): round(float(ms[i]), 3) for i in range(k)}


def best_of(f):
    f()
    best = 1e9
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
    return best, r


def run(name, old, new, level, use_prefix):
    pre = torch.from_numpy(old).cuda() if use_prefix else None
    src = torch.from_numpy(new).cuda()
    n = src.numel()
    dst = torch.empty(n + n // 64 + MiB, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    c = lib.ZSTD_createCCtx()
    lib.ZSTD_CCtx_setParameter(c, 100, level)
    if not use_prefix:
        lib.ZSTD_CCtx_setParameter(c, 160, 1)
    lib.ZSTDMI_CCtx_setProfiling(c, 1)

    def comp():
        if use_prefix:
            assert lib.ZSTD_CCtx_refPrefix(c, pre.data_ptr(), pre.numel()) == 0
        r = lib.ZSTDMI_compressDevice(c, dst.data_ptr(), dst.numel(), src.data_ptr(), n)
        assert not lib.ZSTD_isError(r), lib.ZSTD_getErrorName(r)
        return r
    ct, r = best_of(comp)
    cst = stage_times(lib.ZSTDMI_CCtx_getStageTimes, c)
    lib.ZSTD_freeCCtx(c)
    line = f"{name:22s} L{level} {'prefix' if use_prefix else 'ldm only'}: ratio {r / n:.5f}  compress {n / ct / 1e9:6.2f} GB/s"
    dsts = {}
    for mode, label in ((1, "walk"), (2, "origin")):
        d = lib.ZSTD_createDCtx()
        lib.ZSTDMI_DCtx_setLongFrames(d, mode)
        lib.ZSTDMI_DCtx_setProfiling(d, 1)

        def dec():
            if use_prefix:
                assert lib.ZSTD_DCtx_refPrefix(d, pre.data_ptr(), pre.numel()) == 0
            rr = lib.ZSTDMI_decompressDevice(d, out.data_ptr(), n, dst.data_ptr(), r)
            assert rr == n, lib.ZSTD_getErrorName(rr)
        dt, _ = best_of(dec)
        dsts[label] = stage_times(lib.ZSTDMI_DCtx_getStageTimes, d)
        lib.ZSTD_freeDCtx(d)
        assert bool(torch.equal(out, src)), "round trip"
        out.zero_()
        line += f"  decompress/{label} {n / dt / 1e9:6.2f} GB/s"
    print(line, flush=True)
    print(f"    compress stages ms {cst}", flush=True)
    for label, st in dsts.items():
        print(f"    decompress/{label} stages ms {st}", flush=True)
    del pre, src, dst, out
    torch.cuda.empty_cache()


old = distinct("text", 16 * MiB, 40)
run("text 16+16 MiB", old, edited(old, 41, max(1, edits * 16 * MiB // big), 16 * MiB - 65536), 3, True)
for kind in ("rand", "zipf", "text"):
    old = distinct(kind, big, 50)
    new = edited(old, 51, edits, big - 65536)
    for level in (1, 3):
        run(f"{kind} {big // MiB}+{big // MiB} MiB", old, new, level, True)
        run(f"{kind} {big // MiB} MiB", None, new, level, False)
