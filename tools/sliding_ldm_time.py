"""A long-distance window that slides with one frame (ZSTDMI_CCtx_setSlidingLdm) against plain long-distance matching (aligned windows,
a frame each) and plain single-frame output (run on the GPU box).  Device-resident inputs: Zipf bytes at level 1; 64 MiB random blocks
each repeated once, 64 MiB apart, behind 96 MiB of filler so that every first copy STRADDLES an aligned 128 MiB window (level 1);
text at level 3, 16 MiB of generated text repeated (a repeat 16 MiB back: beyond every block finder, inside every window).
Per row: ratio, compress GB/s, decompress GB/s of that output with ZSTDMI_DCtx_setLongFrames 1 (walk) and 2 (origin), and the compress
call's ldm_* stage times.  Best of 3 after a warm-up call of the same shape; the host clock stops after the call's final synchronise.
Last, a host stream of 256 MiB of the text in 1 MiB writes through ZSTD_compressStream2 as one frame, without and with the switch
(the second with ZSTD_ps_enable): GB/s and ratio.
(The decoder's origin-pointer path takes frames below 1 GiB: at 1024 MiB a single frame is walked in both columns.)
python tools/sliding_ldm_time.py [MiB] [--no-stream]"""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer
lib = z._ffi.load()
MiB = 1 << 20
FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
assert all(f in ("--no-stream",) for f in FLAGS), FLAGS
total = (int(ARGS[0]) if ARGS else 1024) * MiB
MODES = (("plain ldm", 0, 1, 0), ("single frame", 1, 0, 0), ("sliding", 1, 1, 1))       # name, single, ldm, sliding


def ok(r):
    assert not lib.ZSTD_isError(r), lib.ZSTD_getErrorName(r)
    return r


def best_of(f, reps=3):
    f()                                     # warm-up: same shape, workspaces allocated
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        best = min(best, time.perf_counter() - t0)
    return best


def gen_dev(kind, n, seed):
    return torch.from_numpy(np.frombuffer(datagen.gen(kind, n, seed), dtype=np.uint8).copy()).cuda()


def zipf(n):
    return torch.cat([gen_dev("zipf", min(64 * MiB, n - k), 7 + k // MiB) for k in range(0, n, 64 * MiB)])


def straddling_repeats(n):
    parts = [gen_dev("rand", min(96 * MiB, n), 99)]
    k = 0
    while sum(p.numel() for p in parts) < n:
        b = gen_dev("rand", 64 * MiB, 100 + k); k += 1
        parts += [b, b]
    return torch.cat(parts)[:n].contiguous()


def text(n):
    return gen_dev("text", 16 * MiB, 5).repeat((n + 16 * MiB - 1) // (16 * MiB))[:n].contiguous()


def ldm_stages(c):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = lib.ZSTDMI_CCtx_getStageTimes(c, ms, names, 24)
    return " ".join(f"{names[i].decode()} {float(ms[i]):.2f}" for i in range(k) if names[i].decode().startswith("ldm_"))


def new_cctx(level, single, ldm, sliding):
    c = lib.ZSTD_createCCtx()
    ok(lib.ZSTD_CCtx_setParameter(c, 100, level)); ok(lib.ZSTD_CCtx_setParameter(c, 160, ldm))
    ok(lib.ZSTDMI_CCtx_setSingleFrame(c, single)); ok(lib.ZSTDMI_CCtx_setSlidingLdm(c, sliding))
    return c


print(f"{total // MiB} MiB per point; | input | mode | ratio | compress GB/s | decompress walk GB/s | decompress origin GB/s |", flush=True)
for name, make, level in (("zipf L1", zipf, 1), ("straddling 64 MiB repeats L1", straddling_repeats, 1), ("text L3", text, 3)):
    src = make(total)
    dst = torch.empty(lib.ZSTD_compressBound(total), dtype=torch.uint8, device="cuda")
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    for mode, single, ldm, sliding in MODES:
        c = new_cctx(level, single, ldm, sliding)
        lib.ZSTDMI_CCtx_setProfiling(c, 1)
        got = [0]

        def comp():
            got[0] = ok(lib.ZSTDMI_compressDevice(c, dst.data_ptr(), dst.numel(), src.data_ptr(), total))

        tc = best_of(comp)
        stages = ldm_stages(c)
        lib.ZSTD_freeCCtx(c)
        td = []
        for long_frames in (1, 2):
            d = lib.ZSTD_createDCtx()
            ok(lib.ZSTDMI_DCtx_setLongFrames(d, long_frames))
            td.append(best_of(lambda: ok(lib.ZSTDMI_decompressDevice(d, out.data_ptr(), total, dst.data_ptr(), got[0]))))
            assert bool(torch.equal(out, src))
            lib.ZSTD_freeDCtx(d)
        gbs = lambda t: total / t / 1e9
        print(f"| {name} | {mode} | {got[0] / total:.4f} | {gbs(tc):7.2f} | {gbs(td[0]):7.2f} | {gbs(td[1]):7.2f} |   ldm stages ms: {stages}", flush=True)
    del src, dst, out
    torch.cuda.empty_cache()

if "--no-stream" not in FLAGS:
    n = 256 * MiB
    data = datagen.gen("text", 16 * MiB, 5) * (n // (16 * MiB))
    room = ctypes.create_string_buffer(32 * MiB)
    print("a 256 MiB host stream of the text in 1 MiB writes, one frame; | switch | ratio | GB/s |", flush=True)
    for sliding in (0, 1):
        c = new_cctx(3, 1, sliding, sliding)
        best, size = 1e9, 0
        for rep in range(4):
            size = 0
            t0 = time.perf_counter()
            for at in range(0, n + 1, MiB):
                piece = data[at:at + MiB]
                keep = ctypes.create_string_buffer(piece, len(piece)) if piece else None
                inb = ZSTD_inBuffer(ctypes.addressof(keep) if piece else None, len(piece), 0)
                op = 2 if at == n else 0
                while True:
                    ob = ZSTD_outBuffer(ctypes.addressof(room), len(room), 0)
                    r = ok(lib.ZSTD_compressStream2(c, ctypes.byref(ob), ctypes.byref(inb), op))
                    size += ob.pos
                    if (r == 0) if op else (inb.pos == inb.size):
                        break
            if rep:                         # (the first session warms up)
                best = min(best, time.perf_counter() - t0)
        lib.ZSTD_freeCCtx(c)
        print(f"| {sliding} | {size / n:.4f} | {n / best / 1e9:7.3f} |", flush=True)
