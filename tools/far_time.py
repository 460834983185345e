"""Delta frames beyond 512 MiB (ZSTDMI_CCtx_setFarOffsets) against the same construction just under it.

A random prefix on the device, and a source of fresh random bytes followed by the prefix's first 32 MiB: every match lies prefix + fresh
bytes back.  Rows: 384 + 162 MiB (matches 514 MiB back: needs the switch and the decoder's far plane) and 384 + 127 MiB (matches 479 MiB
back, 511 MiB in all: what the library always did).  Per row: compress GB/s, decompress GB/s on the ordered walk and on the origin path
(source bytes per second; best of 3 after a warm-up call; the host clock stops after the call's final synchronise).

python tools/far_time.py [--lib PATH] [--rows far,near]
--lib: another build of libzstd_mi355x.so (one without the switch runs the second row only); --rows near: that row alone, as such a build runs it"""
import argparse
import ctypes
import os
import sys
import time

import torch

MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zstdsharp_amd", "libzstd_mi355x.so"))
    ap.add_argument("--rows", default="far,near", help="which rows to run (a row's buffers lie where the rows before it left them)")
    args = ap.parse_args()
    torch.zeros(1, device="cuda")
    lib = ctypes.CDLL(args.lib)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    for name, res, at in (("ZSTD_createCCtx", vp, []), ("ZSTD_createDCtx", vp, []), ("ZSTD_freeCCtx", sz, [vp]), ("ZSTD_freeDCtx", sz, [vp]),
                          ("ZSTD_compressBound", sz, [sz]), ("ZSTD_CCtx_setParameter", sz, [vp, ctypes.c_int, ctypes.c_int]),
                          ("ZSTD_CCtx_refPrefix", sz, [vp, vp, sz]), ("ZSTD_DCtx_refPrefix", sz, [vp, vp, sz]),
                          ("ZSTDMI_compressDevice", sz, [vp, vp, sz, vp, sz]), ("ZSTDMI_decompressDevice", sz, [vp, vp, sz, vp, sz]),
                          ("ZSTDMI_DCtx_setLongFrames", sz, [vp, ctypes.c_uint]), ("ZSTD_isError", ctypes.c_uint, [sz])):
        f = getattr(lib, name)
        f.restype, f.argtypes = res, at
    has_switch = hasattr(lib, "ZSTDMI_CCtx_setFarOffsets")
    if has_switch:
        lib.ZSTDMI_CCtx_setFarOffsets.restype, lib.ZSTDMI_CCtx_setFarOffsets.argtypes = sz, [vp, ctypes.c_uint]

    def ok(r):
        assert not lib.ZSTD_isError(r), r
        return r

    def best_of(f):
        f()
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return min(ts)

    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rnd = lambda n: torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    prefix = rnd(384 * MiB)
    print(f"library: {args.lib} (switch: {has_switch})")
    print("| prefix + source | matches back | ratio | compress GB/s | decompress GB/s, walk | decompress GB/s, origin |")
    for fresh, far in ((130, True), (95, False)):
        if (far and not has_switch) or ("far" if far else "near") not in args.rows.split(","):
            continue
        src = torch.cat([rnd(fresh * MiB), prefix[:32 * MiB]])
        n = src.numel()
        cap = lib.ZSTD_compressBound(n)
        dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        c = lib.ZSTD_createCCtx()
        ok(lib.ZSTD_CCtx_setParameter(c, 100, 1))
        if far:
            ok(lib.ZSTDMI_CCtx_setFarOffsets(c, 1))
        got = [0]

        def comp():
            ok(lib.ZSTD_CCtx_refPrefix(c, prefix.data_ptr(), prefix.numel()))
            got[0] = ok(lib.ZSTDMI_compressDevice(c, dst.data_ptr(), cap, src.data_ptr(), n))
        tc = best_of(comp)
        lib.ZSTD_freeCCtx(c)
        td = []
        for mode in (1, 2):
            d = lib.ZSTD_createDCtx()
            ok(lib.ZSTDMI_DCtx_setLongFrames(d, mode))

            def dec():
                ok(lib.ZSTD_DCtx_refPrefix(d, prefix.data_ptr(), prefix.numel()))
                assert ok(lib.ZSTDMI_decompressDevice(d, out.data_ptr(), n, dst.data_ptr(), got[0])) == n
            td.append(best_of(dec))
            assert bool(torch.equal(out, src))
            out.zero_()
            lib.ZSTD_freeDCtx(d)
        print(f"| 384 + {fresh + 32} MiB | {(384 + fresh)} MiB | {got[0] / n:.4f} | {n / tc / 1e9:.2f} | {n / td[0] / 1e9:.2f} | {n / td[1] / 1e9:.2f} |", flush=True)
        del src, dst, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    sys.exit(main())
