"""ZSTD_decompressStream over ONE long frame, whole-frame against segmented (ZSTDMI_DCtx_setStreamSegment; run on the GPU box): the
oracle's level-5 frame of text and its level-1 frame of Zipf bytes (one frame each, with a checksum), streamed in 1 MiB reads into a
1 MiB output buffer, with the switch off and with segments of 4, 16 and 64 MiB.  Per row:
  GB/s of content, the time to the first output byte, ZSTDMI_debugStreamPeakInput, what the context holds on the device when the
  stream has ended (the device's free memory before the context's first call minus after its last: its buffers only grow), and for
  one point the stage times of the last segment (ZSTDMI_DCtx_getStageTimes).
Best of 3 after a warm-up pass on the same context; the host clock stops after the last read has returned.  Reports, asserts only that
the bytes are right.
python tools/stream_segment_time.py [MiB] [--off-only] [--root DIR]     (--root: the package of another checkout, e.g. the parent commit's,
which knows no switch: use with --off-only)"""
import ctypes, sys, os, time
args = [a for a in sys.argv[1:]]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = ROOT
if "--root" in args:
    PKG = os.path.abspath(args[args.index("--root") + 1]); del args[args.index("--root"):args.index("--root") + 2]
OFF_ONLY = "--off-only" in args
args = [a for a in args if a != "--off-only"]
sys.path.insert(0, PKG); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen, oracle_lib
from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer
lib = z._ffi.load()
MiB = 1 << 20
total = (int(args[0]) if args else 256) * MiB
READ = MiB


def stage_times(ctx):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = lib.ZSTDMI_DCtx_getStageTimes(ctx, ms, names, 24)
    return " ".join(f"{names[i].decode()} {float(ms[i]):.2f}" for i in range(k))


def stream(d, blob_buf, n, out_buf, check=None):
    """-> seconds for the whole stream, seconds to the first output byte, content bytes"""
    base, daddr = ctypes.addressof(blob_buf), ctypes.addressof(out_buf)
    inp, out = ZSTD_inBuffer(), ZSTD_outBuffer(daddr, READ, 0)
    pin, pout = ctypes.byref(inp), ctypes.byref(out)
    got, first, fed, r = 0, None, 0, 1
    t0 = time.perf_counter()
    while fed < n:
        k = min(READ, n - fed)
        inp.src, inp.size, inp.pos = base + fed, k, 0
        fed += k
        while True:
            out.pos = 0
            r = lib.ZSTD_decompressStream(d, pout, pin)
            assert not lib.ZSTD_isError(r), lib.ZSTD_getErrorName(r)
            if out.pos:
                if first is None:
                    first = time.perf_counter() - t0
                if check is not None:
                    assert ctypes.string_at(daddr, out.pos) == check[got:got + out.pos], f"wrong bytes at {got}"
                got += out.pos
            if inp.pos >= inp.size and out.pos < READ:
                break
    t = time.perf_counter() - t0
    assert r == 0
    return t, first, got


print(f"{total // MiB} MiB of content in one frame; 1 MiB reads", flush=True)
print("| input | segment | GB/s | first byte ms | peak host input | device bytes held |", flush=True)
for kind, level in (("text", 5), ("zipf", 1)):
    piece = datagen.gen(kind, min(64 * MiB, total), 5)
    data = piece * (total // len(piece))              # (one frame: the repeats are 64 MiB apart, beyond these levels' windows)
    blob = oracle_lib.compress(data, level, 1, 0)
    assert isinstance(blob, bytes)
    n = len(blob)
    blob_buf = ctypes.create_string_buffer(blob, n)
    out_buf = ctypes.create_string_buffer(READ)
    for seg in ((0,) if OFF_ONLY else (0, 4 * MiB, 16 * MiB, 64 * MiB)):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        d = lib.ZSTD_createDCtx()
        if seg:
            assert lib.ZSTDMI_DCtx_setStreamSegment(d, seg) == 0
        _, _, got = stream(d, blob_buf, n, out_buf, check=data)        # warm-up, and the bytes are checked here
        assert got == total
        best, first = 1e9, 1e9
        for _ in range(3):
            t, f, got = stream(d, blob_buf, n, out_buf)
            best, first = min(best, t), min(first, f)
        held = free0 - torch.cuda.mem_get_info()[0]
        peak_s = f"{lib.ZSTDMI_debugStreamPeakInput(d)}" if seg else f"{n} (the frame)"      # (the counter runs while the switch is on)
        print(f"| {kind} L{level} ({n} B) | {seg // MiB if seg else 'off':>3} | {total / best / 1e9:6.3f} | {first * 1e3:9.2f} | {peak_s} | {held} |", flush=True)
        if seg == 16 * MiB and kind == "text":
            lib.ZSTDMI_DCtx_setProfiling(d, 1)
            stream(d, blob_buf, n, out_buf)
            print(f"    stages of the last segment, ms: {stage_times(d)}  ({lib.ZSTDMI_debugStreamSegments(d)} segments in 5 passes)", flush=True)
        lib.ZSTD_freeDCtx(d)
    del data, blob, blob_buf
