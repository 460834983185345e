"""Long-distance matching, on vs off (run on the GPU box): stage times per GiB (the ldm_* stages separately), compress and decompress
GB/s of device-resident calls, ratio.  Inputs: 1 GiB Zipf at level 1; 1 GiB of 64 MiB random blocks each repeated once, 64 MiB
apart, at level 1; 1 GiB text at level 3.  python tools/ldm_time.py [MiB]"""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen
lib = z._ffi.load()
MiB = 1 << 20
total = (int(sys.argv[1]) if len(sys.argv) > 1 else 1024) * MiB


def distinct(kind, n, seed):
    """n bytes of pieces of 64 MiB, each with a seed of its own (no repeats for LDM to find)"""
    return np.concatenate([np.frombuffer(datagen.gen(kind, min(64 * MiB, n - k), seed + k // MiB), dtype=np.uint8) for k in range(0, n, 64 * MiB)])


def repeats(n):
    parts = []
    for k in range(0, n, 128 * MiB):
        b = np.frombuffer(datagen.gen("rand", 64 * MiB, 100 + k // MiB), dtype=np.uint8)
        parts += [b, b]
    return np.concatenate(parts)[:n]


def stage_times(c):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = lib.ZSTDMI_CCtx_getStageTimes(c, ms, names, 24)
    return {names[i].decode(): float(ms[i]) for i in range(k)}


cases = [("zipf L1", lambda: distinct("zipf", total, 7), 1), ("64 MiB repeats L1", lambda: repeats(total), 1), ("text L3", lambda: distinct("text", total, 8), 3)]
for name, make, level in cases:
    src = torch.from_numpy(make().copy()).cuda()
    n = src.numel()
    dst = torch.empty(n + n // 64 + (1 << 20), dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    for ldm in (0, 1):
        c = lib.ZSTD_createCCtx()
        lib.ZSTD_CCtx_setParameter(c, 100, level)
        lib.ZSTD_CCtx_setParameter(c, 160, ldm)
        lib.ZSTDMI_CCtx_setProfiling(c, 1)
        best = 1e9
        for rep in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = lib.ZSTDMI_compressDevice(c, dst.data_ptr(), dst.numel(), src.data_ptr(), n)
            best = min(best, time.perf_counter() - t0)
            assert not lib.ZSTD_isError(r), lib.ZSTD_getErrorName(r)
        st = stage_times(c)
        lib.ZSTD_freeCCtx(c)
        d = lib.ZSTD_createDCtx()
        dbest = 1e9
        for rep in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            rr = lib.ZSTDMI_decompressDevice(d, out.data_ptr(), n, dst.data_ptr(), r)
            dbest = min(dbest, time.perf_counter() - t0)
            assert rr == n, lib.ZSTD_getErrorName(rr)
        lib.ZSTD_freeDCtx(d)
        ok = bool(torch.equal(out, src))
        gib = n / (1 << 30)
        ldm_ms = {k: round(v / gib, 3) for k, v in st.items() if k.startswith("ldm_")}
        print(f"{name:18s} ldm {ldm}: ratio {r / n:.4f}  compress {n / best / 1e9:7.1f} GB/s  decompress {n / dbest / 1e9:7.1f} GB/s  exact {ok}"
              f"  stages sum {sum(st.values()) / gib:.2f} ms/GiB  ldm stages ms/GiB {ldm_ms}", flush=True)
    del src, dst, out
    torch.cuda.empty_cache()
