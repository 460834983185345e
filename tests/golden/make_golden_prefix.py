"""Generates the delta fixtures (tests/golden/prefix_*.zst + manifest_prefix.json): frames written by libzstd's ZSTD_CCtx_refPrefix +
ZSTD_compress2, i.e. what the reference's U/ZstdCompress.cs:1723-1765 writes (its T/ZstdTest.cs:69-90 treats native libzstd as its
byte-for-byte equal).  Run ONCE in the authoring container (needs the third-party libzstd 1.5.7 shared object bundled with Pillow
there); only the compressed frames are committed, prefixes and contents are rebuilt from seeds by tests/prefix_cases.py."""
import ctypes, glob, hashlib, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import prefix_cases

sz, vp, ci = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int


def load():
    path = glob.glob("/usr/local/lib/python3*/dist-packages/pillow.libs/libzstd*")[0]
    l = ctypes.CDLL(path)
    l.ZSTD_versionNumber.restype = ctypes.c_uint
    l.ZSTD_compressBound.restype = sz; l.ZSTD_compressBound.argtypes = [sz]
    l.ZSTD_createCCtx.restype = vp
    l.ZSTD_freeCCtx.argtypes = [vp]
    l.ZSTD_CCtx_setParameter.restype = sz; l.ZSTD_CCtx_setParameter.argtypes = [vp, ci, ci]
    l.ZSTD_CCtx_refPrefix.restype = sz; l.ZSTD_CCtx_refPrefix.argtypes = [vp, vp, sz]
    l.ZSTD_compress2.restype = sz; l.ZSTD_compress2.argtypes = [vp, vp, sz, vp, sz]
    l.ZSTD_isError.restype = ctypes.c_uint; l.ZSTD_isError.argtypes = [sz]
    return l


def main():
    l = load()
    assert l.ZSTD_versionNumber() == 10507
    cases = []
    for name, (_, kind, level, ldm, window_log) in prefix_cases.CASES.items():
        prefix, content = prefix_cases.build(name)
        # distinct buffer objects: the same buffer for both would be one contiguous segment to libzstd, which then finds nothing
        pbuf = ctypes.create_string_buffer(prefix, len(prefix)); cbuf = ctypes.create_string_buffer(content, len(content))
        c = l.ZSTD_createCCtx()
        for param, value in ((100, level), (101, window_log), (160, 1 if ldm else 2), (201, 1)):
            assert not l.ZSTD_isError(l.ZSTD_CCtx_setParameter(c, param, value))
        assert not l.ZSTD_isError(l.ZSTD_CCtx_refPrefix(c, pbuf, len(prefix)))
        cap = l.ZSTD_compressBound(len(content)) + 64; dst = ctypes.create_string_buffer(cap)
        r = l.ZSTD_compress2(c, dst, cap, cbuf, len(content)); assert not l.ZSTD_isError(r)
        l.ZSTD_freeCCtx(c)
        f = f"prefix_{name}_l{level}.zst"
        open(os.path.join(HERE, f), "wb").write(dst.raw[:r])
        cases.append(dict(file=f, case=name, kind=kind, prefix_n=len(prefix), n=len(content), level=level, ldm=ldm, windowLog=window_log,
                          checksum=1, seeds=prefix_cases.SEEDS[name], csize=r, prefix_sha256=hashlib.sha256(prefix).hexdigest(),
                          sha256=hashlib.sha256(content).hexdigest(), libzstd=10507))
        print(f, r)
    json.dump(dict(generator="tests/golden/make_golden_prefix.py", cases=cases), open(os.path.join(HERE, "manifest_prefix.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
