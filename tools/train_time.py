"""Wall time of GPU dictionary training (ZDICT_trainFromBuffer, default capacity 112640) on text records, the chosen k, the
dictionary size and the held-out ratio with and without the dictionary.  libzstd's single-thread time on the same host is
reported only when a libzstd shared object is already installed there.
usage: python tools/train_time.py [MiB ...]   (default: 4)"""
import ctypes, glob, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_train as mgt
import zstdsharp_amd as z
from zstdsharp_amd import _ffi


def corpus(mib, seed):
    sizes = [180, 420, 260, 900, 140]
    return mgt.samples(dict(kind="text", seed=seed, sizes=sizes, count=int(mib * (1 << 20) / (sum(sizes) / len(sizes)))))


def main():
    lib = _ffi.load()
    libzstd = (glob.glob("/usr/local/lib/python3*/dist-packages/pillow.libs/libzstd*") + glob.glob("/usr/lib/x86_64-linux-gnu/libzstd.so*"))
    for mib in [float(a) for a in sys.argv[1:]] or [4.0]:
        recs = corpus(mib, 31)
        flat = b"".join(recs)
        sizes = (ctypes.c_size_t * len(recs))(*[len(r) for r in recs])
        src = ctypes.create_string_buffer(flat, len(flat)); dst = ctypes.create_string_buffer(112640)
        p = _ffi.ZDICT_fastCover_params_t(); p.d = 8; p.steps = 4; p.zParams.compressionLevel = 3
        t = time.perf_counter()
        n = lib.ZDICT_optimizeTrainFromBuffer_fastCover(dst, 112640, src, sizes, len(recs), ctypes.byref(p))
        wall = time.perf_counter() - t
        assert not lib.ZDICT_isError(n), lib.ZDICT_getErrorName(n)
        dic = dst.raw[:n]
        held = corpus(1, 77)[:2000]
        with z.Compressor(3) as c:
            none = sum(len(c.Wrap(r)) for r in held)
            c.LoadDictionary(dic)
            withd = sum(len(c.Wrap(r)) for r in held)
        raw = sum(len(r) for r in held)
        line = (f"{mib:g} MiB, {len(recs)} samples: {wall:.3f} s, k={p.k}, dict {n} B, held-out ratio {withd / raw:.4f} "
                f"with / {none / raw:.4f} without")
        if libzstd:
            l = ctypes.CDLL(libzstd[0]); l.ZDICT_trainFromBuffer.restype = ctypes.c_size_t
            l.ZDICT_trainFromBuffer.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint]
            t = time.perf_counter(); l.ZDICT_trainFromBuffer(dst, 112640, src, sizes, len(recs)); line += f"; libzstd {time.perf_counter() - t:.3f} s"
        else:
            line += "; no libzstd shared object found on this host"
        print(line, flush=True)


if __name__ == "__main__":
    main()
