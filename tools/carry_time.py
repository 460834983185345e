"""Entropy state carried across blocks (ZSTDMI_CCtx_setEntropyCarry) against the default coding (run on the GPU box).
Sizes: per input, level and framing the bytes with the switch off and on, the oracle's bytes at the same frame size and as one frame,
and of the blocks written with the switch on the share that is treeless and that repeats 1, 2 or 3 tables.
Time: device-resident input (16 MiB of generated text repeated; text repeats at 16 MiB, beyond every finder here), the whole call
with the switch off and on — best of 3 after a warm-up call of the same shape, the host clock stopped after the call's final
synchronise, profiling off — then one more call each with profiling on for the seq_encode / huf_tree / huf_encode stage times, and
the decompress GB/s of both outputs; every output is decoded and compared.  With --parent the parent commit's library runs the
"off" row beside this one's in the same session.
python tools/carry_time.py [--sizes-only | --time-only] [--mib N] [--parent /path/to/libzstd_mi355x.so]
  --mib N : bytes per timed point at levels 3 and 5 (default 1024)"""
import argparse, ctypes, lzma, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen, oracle_lib, zstd_blocks as zb
from zstdsharp_amd import _ffi
lib = _ffi.load()
MiB = 1 << 20
ap = argparse.ArgumentParser()
ap.add_argument("--sizes-only", action="store_true"); ap.add_argument("--time-only", action="store_true")
ap.add_argument("--mib", type=int, default=1024); ap.add_argument("--parent", default=None)
args = ap.parse_args()


def load_other(path):
    """another build of the library, typed as far as it has the symbols"""
    other = ctypes.CDLL(path)
    for name, (res, argt) in _ffi.SIGNATURES.items():
        if hasattr(other, name):
            fn = getattr(other, name); fn.restype, fn.argtypes = res, argt
    return other


def ok(L, r):
    assert not L.ZSTD_isError(r), L.ZSTD_getErrorName(r)
    return r


def pysrc(n):
    return lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "pysrc_4m.xz"), "rb").read())[:n]


def best_of(f, reps=3):
    f()                                     # warm-up: same shape, workspaces allocated
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        best = min(best, time.perf_counter() - t0)
    return best


def stage_ms(L, ctx, wanted=("seq_encode", "huf_tree", "huf_encode")):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = L.ZSTDMI_CCtx_getStageTimes(ctx, ms, names, 24)
    got = {names[i].decode(): float(ms[i]) for i in range(k)}
    return " ".join(f"{w} {got.get(w, float('nan')):.2f}" for w in wanted)


# ---------------------------------------------------------------- sizes ----------------------------------------------------------------
def frame_bytes(level, params, single, n):
    """content bytes of one frame of the framing the row runs with (for the oracle at the same frame size)"""
    if single:
        return n
    if level == 1:
        return (128 << 10) if params else (64 << 10)      # windowLog 17: two 64 KiB blocks; small calls: four 16 KiB blocks
    return (240 << 10) if level < 5 else (256 << 10)


def sizes():
    print("| input | level | off | on | on / off | oracle, same frames | oracle, one frame | blocks | treeless | 1 / 2 / 3 tables repeated |")
    rows = [(kind, 4 * MiB, level, params, False) for kind in ("text", "pysrc") for level, params in ((1, {101: 17}), (3, None), (5, None), (9, None))]
    rows += [("text", 10 * MiB, 1, None, False), ("text", 4 * MiB, 3, None, True), ("text", 4 * MiB, 5, None, True)]
    for kind, n, level, params, single in rows:
        data = pysrc(n) if kind == "pysrc" else datagen.gen(kind, n, 5)
        out = []
        for carry in (False, True):
            with z.Compressor(level) as c:
                for k, v in (params or {}).items():
                    c.SetParameter(k, v)
                c.single_frame = single
                c.entropy_carry = carry
                out.append(c.Wrap(data))
        for blob in out:
            with z.Decompressor() as d:
                assert d.Unwrap(blob, maxDecompressedSize=n) == data
        blocks = [b for f in zb.check_stream_state(out[1], 8) for b in f]
        assert not any(b.carried for f in zb.check_stream_state(out[0]) for b in f)
        rep = [sum(1 for b in blocks if b.repeats == k) for k in (1, 2, 3)]
        same = len(oracle_lib.compress(data, level, 0, frame_bytes(level, params, single, n))) if not single else len(oracle_lib.compress(data, level))
        one = len(oracle_lib.compress(data, level))
        tag = f"{level}" + (" w17" if params else "") + (" single frame" if single else "")
        print(f"| {kind} {n // MiB} MiB | {tag} | {len(out[0])} | {len(out[1])} | {len(out[1]) / len(out[0]):.4f} | {same} | {one} | {len(blocks)} | "
              f"{sum(b.treeless for b in blocks) / len(blocks):.3f} | {rep[0] / len(blocks):.3f} / {rep[1] / len(blocks):.3f} / {rep[2] / len(blocks):.3f} |", flush=True)


# ---------------------------------------------------------------- time ----------------------------------------------------------------
def time_point(L, name, level, total, carry, src, dst, out):
    c = L.ZSTD_createCCtx()
    ok(L, L.ZSTD_CCtx_setParameter(c, 100, level))
    if carry is not None:
        ok(L, L.ZSTDMI_CCtx_setEntropyCarry(c, 1 if carry else 0))
    got = [0]

    def comp():
        got[0] = ok(L, L.ZSTDMI_compressDevice(c, dst.data_ptr(), dst.numel(), src.data_ptr(), total))
    tc = best_of(comp)
    L.ZSTDMI_CCtx_setProfiling(c, 1)
    comp()                                  # one more call, traced: the stage times
    stages = stage_ms(L, c)
    d = lib.ZSTD_createDCtx()
    td = best_of(lambda: ok(lib, lib.ZSTDMI_decompressDevice(d, out.data_ptr(), total, dst.data_ptr(), got[0])))
    assert bool(torch.equal(out, src)), "every output is decoded and compared"
    lib.ZSTD_freeDCtx(d)
    L.ZSTD_freeCCtx(c)
    print(f"| text {total // MiB} MiB L{level} | {name} | {got[0]} | {tc * 1e3:.2f} ms | {total / tc / 1e9:.2f} GB/s | {stages} | decompress {total / td / 1e9:.2f} GB/s |", flush=True)


def times():
    parent = load_other(args.parent) if args.parent else None
    print("| point | library, switch | bytes | whole call | rate | stage ms | decoding that output |")
    for level, total in ((3, args.mib * MiB), (5, args.mib * MiB), (1, 10 * MiB)):
        unit = min(16 * MiB, total)
        src = torch.from_numpy(np.frombuffer(datagen.gen("text", unit, 5), dtype=np.uint8).copy()).cuda()
        src = src.repeat(total // unit) if total > unit else src[:total].clone()
        dst = torch.empty(lib.ZSTD_compressBound(total), dtype=torch.uint8, device="cuda")
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        if parent is not None:
            time_point(parent, "parent", level, total, None, src, dst, out)
        time_point(lib, "off", level, total, False, src, dst, out)
        time_point(lib, "on", level, total, True, src, dst, out)
        if parent is not None:              # (once more, the other way round: the order is not the difference)
            time_point(lib, "off", level, total, False, src, dst, out)
            time_point(parent, "parent", level, total, None, src, dst, out)
        del src, dst, out
        torch.cuda.empty_cache()


if not args.time_only:
    sizes()
if not args.sizes_only:
    times()
