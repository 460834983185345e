"""One frame per call (ZSTDMI_CCtx_setSingleFrame) against the default run of frames (run on the GPU box): device-resident input,
Zipf bytes at level 1 and text at levels 1, 3 and 5; per point the switch off and on, and both again with ZSTD_c_checksumFlag = 1 (the
single frame's checksum is one serial chain over the whole input: its cost per GiB is the difference of the two rows).  Per row:
ratio, compress GB/s, decompress GB/s of that output with ZSTDMI_DCtx_setLongFrames 1 (walk) and 2 (origin), and the compress call's
stage times.  Best of 3 after a warm-up call of the same shape; the host clock stops after the call's final synchronise.  The input is
16 MiB of generated data repeated; Zipf bytes repeat nothing a finder reaches, text repeats at 16 MiB, beyond every finder here.
Last, the sizes of 1 MiB of text at levels 1, 3 and 5 — switch on, switch off, the oracle's one-frame output.
(The decoder's origin-pointer path takes frames below 1 GiB; a single frame of exactly 1 GiB is walked in order.  A second run at
512 MiB shows the rates of the origin path.)
python tools/single_frame_time.py [MiB] [--sizes-only] [--no-checksum]
  --sizes-only  : only the 1 MiB sizes
  --no-checksum : skip the rows with ZSTD_c_checksumFlag = 1 (the serial hash takes seconds per GiB)"""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen, oracle_lib
lib = z._ffi.load()
MiB = 1 << 20
FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
assert all(f in ("--sizes-only", "--no-checksum") for f in FLAGS), FLAGS
total = (int(ARGS[0]) if ARGS else 1024) * MiB


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


def sizes_of_one_mib():
    data = datagen.gen("text", MiB, 11)
    print("1 MiB of text: bytes with the switch on | off | the oracle's one frame")
    for level in (1, 3, 5):
        out = []
        for single in (1, 0):
            with z.Compressor(level) as c:
                c.single_frame = bool(single)
                out.append(len(c.Wrap(data)))
        print(f"| {level} | {out[0]} | {out[1]} | {len(oracle_lib.compress(data, level))} |", flush=True)


if "--sizes-only" not in FLAGS:
    print(f"{total // MiB} MiB per point", flush=True)
    for kind, level in (("zipf", 1), ("text", 1), ("text", 3), ("text", 5)):
        src = torch.from_numpy(np.frombuffer(datagen.gen(kind, 16 * MiB, 5), dtype=np.uint8).copy()).cuda().repeat(total // (16 * MiB))
        dst = torch.empty(lib.ZSTD_compressBound(total), dtype=torch.uint8, device="cuda")
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        for checksum in ((0,) if "--no-checksum" in FLAGS else (0, 1)):
            for single in (0, 1):
                c = lib.ZSTD_createCCtx()
                ok(lib.ZSTD_CCtx_setParameter(c, 100, level)); ok(lib.ZSTD_CCtx_setParameter(c, 201, checksum)); ok(lib.ZSTDMI_CCtx_setSingleFrame(c, single))
                lib.ZSTDMI_CCtx_setProfiling(c, 1)
                got = [0]

                def comp():
                    got[0] = ok(lib.ZSTDMI_compressDevice(c, dst.data_ptr(), dst.numel(), src.data_ptr(), total))

                tc = best_of(comp)
                stages = stage_times(lib.ZSTDMI_CCtx_getStageTimes, c)
                td = []
                for mode in (1, 2):
                    d = lib.ZSTD_createDCtx()
                    ok(lib.ZSTDMI_DCtx_setLongFrames(d, mode))
                    td.append(best_of(lambda: ok(lib.ZSTDMI_decompressDevice(d, out.data_ptr(), total, dst.data_ptr(), got[0]))))
                    assert bool(torch.equal(out, src))
                    lib.ZSTD_freeDCtx(d)
                gbs = lambda t: total / t / 1e9
                print(f"| {kind} L{level} | checksum {checksum} | single {single} | {got[0] / total:.4f} | {gbs(tc):7.2f} | {gbs(td[0]):7.2f} | {gbs(td[1]):7.2f} |", flush=True)
                print(f"    compress stages ms: {stages}", flush=True)
                lib.ZSTD_freeCCtx(c)
        del src, dst, out
        torch.cuda.empty_cache()
sizes_of_one_mib()
