"""Generates tests/golden/forge_*.zst + manifest_forge.json from tests/forge_cases.py.  Run ONCE in the authoring container (it needs
the two libzstd shared objects of make_golden.py: 1.4.8 system, 1.5.7 bundled with Pillow); the outputs are committed, the GPU box and
the test-suite only read them.

The frames are written by tests/zstd_forge.py, field by field, and their expected content by its plain LZ executor.  Each is then
shown to three decoders — both libzstd versions and the oracle (oracle/zso_dec.c, the reference's decoder restated) — and their
verdicts are stored beside it:

    "equal"                        accepted, the executor's bytes
    "different:<size>:<sha256>"    accepted, other bytes (for a case the forge holds invalid: any bytes)
    "rejected:<code>"              refused, with the ZSTD_ErrorCode

A case the forge holds valid is AGREED when all three say "equal"; one it holds invalid, when all three refuse it.  Every other case
is CONTESTED: it stays, with its verdicts, and there the GPU decoder must do what the oracle does.  Every tag of
forge_cases.TAGS must keep at least one agreed case — asserted below, before anything is written.

To add a corner: describe it in tests/forge_cases.py, rerun this script, and look at what it prints for the new case.
"""
import ctypes, glob, hashlib, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import forge_cases
import oracle_lib


def load(path):
    l = ctypes.CDLL(path)
    l.ZSTD_decompress.restype = ctypes.c_size_t
    l.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    l.ZSTD_isError.argtypes = [ctypes.c_size_t]
    l.ZSTD_getErrorCode.argtypes = [ctypes.c_size_t]
    l.ZSTD_versionNumber.restype = ctypes.c_uint
    return l


def verdict(got, content):
    """got: bytes or a negative error code"""
    if isinstance(got, int):
        return "rejected:%d" % -got
    if content is not None and got == content:
        return "equal"
    return "different:%d:%s" % (len(got), hashlib.sha256(got).hexdigest())


def libzstd_decode(l, blob, cap):
    buf = ctypes.create_string_buffer(max(cap, 1))
    n = l.ZSTD_decompress(buf, cap, blob, len(blob))
    return -l.ZSTD_getErrorCode(n) if l.ZSTD_isError(n) else buf.raw[:n]


def main():
    libs = {}
    for p in ["/usr/lib/x86_64-linux-gnu/libzstd.so.1"] + glob.glob("/usr/local/lib/python3*/dist-packages/pillow.libs/libzstd*"):
        l = load(p); libs[l.ZSTD_versionNumber()] = l
    assert len(libs) == 2, "two libzstd versions are needed"
    cases, files, agreed_tags = [], {}, set()
    for name, tags, build, valid in forge_cases.CASES:
        blob, content = build()
        assert (content is not None) == valid, name
        cap = forge_cases.capacity(len(content) if valid else None)
        v = {str(ver): verdict(libzstd_decode(l, blob, cap), content) for ver, l in sorted(libs.items())}
        vo = verdict(oracle_lib.decompress(blob, cap), content)
        every = list(v.values()) + [vo]
        agreed = all(x == "equal" for x in every) if valid else all(x.startswith("rejected") for x in every)
        if agreed:
            agreed_tags.update(tags)
        fn = "forge_" + name + ".zst"
        files[fn] = blob
        cases.append(dict(file=fn, name=name, tags=tags, valid=valid, csize=len(blob),
                          size=len(content) if valid else None, sha256=hashlib.sha256(content).hexdigest() if valid else None,
                          libzstd=v, oracle=vo, agreed=agreed))
        if not agreed:
            print("contested:", name, v, vo)
    missing = [t for t in forge_cases.TAGS if t not in agreed_tags]
    assert not missing, ("tags without an agreed case", missing)
    total = sum(len(b) for b in files.values())
    # 64 KiB per fixture; the two long frames may take 256 KiB; one skippable frame of 70 000 bytes cannot be smaller than it is
    limit = {"forge_long_frame_1m_plus_5.zst": 256 << 10, "forge_long_frame_3m.zst": 256 << 10, "forge_skip_long.zst": 72 << 10}
    big = [fn for fn, b in files.items() if len(b) >= limit.get(fn, 64 << 10)]
    assert total < (1 << 20) and not big, (total, big)
    for old in glob.glob(os.path.join(HERE, "forge_*.zst")):
        os.remove(old)
    for fn, blob in files.items():
        open(os.path.join(HERE, fn), "wb").write(blob)
    json.dump(dict(generator="tests/golden/make_golden_forge.py", tags=forge_cases.TAGS, cases=cases),
              open(os.path.join(HERE, "manifest_forge.json"), "w"), indent=1)
    print(len(cases), "fixtures,", total, "bytes,", sum(1 for c in cases if not c["agreed"]), "contested")


if __name__ == "__main__":
    main()
