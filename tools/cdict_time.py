"""Digested dictionaries (ZSTD_CDict / ZSTD_DDict) against ZSTD_*_loadDictionary, run on the GPU box.  Every figure is the best of 3 after a
warm-up of the same shape, the host clock stopped after the final synchronise, and every output is compared with the yardstick's.
  switch   : 2 000 ZSTD_compress2 calls on 300-byte JSON-like records (tests/golden/make_golden_train.py), alternating between two trained
             dictionaries (train_default_json.dict, trained_16k.dict), all four dictionary switches on: ZSTD_CCtx_loadDictionary before
             each call against ZSTD_CCtx_refCDict before each call; us per call (the switch and the call).
  contexts : creation to the first compressed record for 16 contexts, each with ZSTD_CCtx_loadDictionary, against 16 contexts that
             reference one CDict (its creation included); ms for all 16.
  decode   : [records] (default 65 536) text records of 4 KiB, level 3, trained_16k.dict, ZSTDMI_CCtx_setDictEntropy on, one
             ZSTDMI_decompressBatch: ZSTD_DCtx_loadDictionary against ZSTD_DCtx_refDDict; call ms, the seq_decode stage and the literal
             stage, and the blocks that copied a ready-made table.
python tools/cdict_time.py [records]"""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen
import make_golden_train as mgt
lib = z._ffi.load()
GOLDEN = os.path.join(ROOT, "tests", "golden")
records = int(sys.argv[1]) if len(sys.argv) > 1 else 65536


def golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def best_of(f):
    f()
    best = 1e9
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
    return best, r


def stage_times(d):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = lib.ZSTDMI_DCtx_getStageTimes(d, ms, names, 24)
    out = {}
    for i in range(k):
        out[names[i].decode()] = out.get(names[i].decode(), 0.0) + float(ms[i])
    return out


def all_switches(c):
    for call, v in ((lib.ZSTDMI_CCtx_setDictEntropy, 1), (lib.ZSTDMI_CCtx_setDictIndex, 1), (lib.ZSTDMI_CCtx_setDictIndexStrategy, 2), (lib.ZSTDMI_CCtx_setDictIndexChain, 1)):
        assert call(c, v) == 0


def switch_cost():
    dicts = [golden("train_default_json.dict"), golden("trained_16k.dict")]
    recs = [r[:300].ljust(300, b" ") for r in mgt.json_records(2000, 77)]
    room = ctypes.create_string_buffer(lib.ZSTD_compressBound(300))

    def run(ref):
        c = lib.ZSTD_createCCtx()
        all_switches(c)
        cds = [lib.ZSTD_createCDict(d, len(d), 3) for d in dicts] if ref else None
        assert not ref or all(cds)

        def calls():
            out = []
            for i, r in enumerate(recs):
                if ref:
                    assert lib.ZSTD_CCtx_refCDict(c, cds[i & 1]) == 0
                else:
                    assert lib.ZSTD_CCtx_loadDictionary(c, dicts[i & 1], len(dicts[i & 1])) == 0
                n = lib.ZSTD_compress2(c, room, len(room), r, len(r))
                assert not lib.ZSTD_isError(n), lib.ZSTD_getErrorName(n)
                out.append(room.raw[:n])
            return out
        t, out = best_of(calls)
        uploads = lib.ZSTDMI_debugDictUploads(c)
        lib.ZSTD_freeCCtx(c)
        for cd in cds or ():
            lib.ZSTD_freeCDict(cd)
        return t, out, uploads
    tl, wl, ul = run(False)
    tr, wr, ur = run(True)
    assert wl == wr, "refCDict must write the loaded dictionary's bytes"
    print(f"switch   : {len(recs)} calls of 300 B, two dictionaries alternating, all switches on: loadDictionary {tl / len(recs) * 1e6:8.1f} us/call "
          f"({ul} uploads), refCDict {tr / len(recs) * 1e6:8.1f} us/call ({ur} uploads)", flush=True)


def contexts():
    dic, rec = golden("train_default_json.dict"), mgt.json_records(2000, 77)[5][:300]
    room = ctypes.create_string_buffer(lib.ZSTD_compressBound(len(rec)))

    def run(ref):
        def go():
            cd = lib.ZSTD_createCDict(dic, len(dic), 3) if ref else None
            ctxs, out = [], []
            for _ in range(16):
                c = lib.ZSTD_createCCtx()
                all_switches(c)
                assert (lib.ZSTD_CCtx_refCDict(c, cd) if ref else lib.ZSTD_CCtx_loadDictionary(c, dic, len(dic))) == 0
                n = lib.ZSTD_compress2(c, room, len(room), rec, len(rec))
                assert not lib.ZSTD_isError(n), lib.ZSTD_getErrorName(n)
                out.append(room.raw[:n]); ctxs.append(c)
            return ctxs, cd, out
        best, outs = 1e9, None
        for k in range(4):          # (the first is the warm-up)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ctxs, cd, outs = go()
            torch.cuda.synchronize(); t = time.perf_counter() - t0
            if k:
                best = min(best, t)
            for c in ctxs:
                lib.ZSTD_freeCCtx(c)
            lib.ZSTD_freeCDict(cd)
        return best, outs
    tl, wl = run(False)
    tr, wr = run(True)
    assert wl == wr and len(set(wl)) == 1
    print(f"contexts : 16 contexts from creation to the first record: loadDictionary each {tl * 1e3:7.2f} ms, one shared CDict {tr * 1e3:7.2f} ms", flush=True)


def decode():
    dic = golden("trained_16k.dict")
    base = np.frombuffer(datagen.gen("text", 16 << 20, 3), dtype=np.uint8)
    n = records
    src = torch.from_numpy(np.resize(base, n * 4096).copy()).cuda()
    with z.Compressor(3) as c:
        c.dict_entropy = True
        c.LoadDictionary(dic)
        comp = z.compress_batch(c, [src[i * 4096:(i + 1) * 4096] for i in range(n)])
    sizes = (ctypes.c_size_t * n)(*[t.numel() for t in comp])
    srcs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in comp])
    out = torch.empty(n * 4096, dtype=torch.uint8, device="cuda")
    dsts = (ctypes.c_void_p * n)(*[out.data_ptr() + i * 4096 for i in range(n)])
    caps = (ctypes.c_size_t * n)(*([4096] * n))
    got = (ctypes.c_size_t * n)()
    dd = lib.ZSTD_createDDict(dic, len(dic))
    assert dd
    rows = {}
    for label in ("loadDictionary", "refDDict", "loadDictionary again", "refDDict again"):
        d = lib.ZSTD_createDCtx()
        assert (lib.ZSTD_DCtx_refDDict(d, dd) if label.startswith("ref") else lib.ZSTD_DCtx_loadDictionary(d, dic, len(dic))) == 0
        lib.ZSTDMI_DCtx_setProfiling(d, 1)

        def call():
            assert lib.ZSTDMI_decompressBatch(d, srcs, sizes, n, dsts, caps, got) == 0
        out.zero_()
        t, _ = best_of(call)
        assert all(g == 4096 for g in got) and bool(torch.equal(out, src)), label
        st = stage_times(d)
        lits = sum(v for k, v in st.items() if "literal" in k and k != "place_literals")
        rows[label] = (t * 1e3, st.get("seq_decode", 0.0), lits)
        print(f"decode   : {n} x 4 KiB text, level 3, trained_16k.dict, dictionary entropy on, {label:22s}: call {t * 1e3:7.3f} ms  seq_decode {st.get('seq_decode', 0.0):6.3f} ms  "
              f"literal stage {lits:6.3f} ms  ready-table blocks {lib.ZSTDMI_debugLastDictTableBlocks(d)}  uploads {lib.ZSTDMI_debugDictUploadsD(d)}", flush=True)
        print(f"           stages ms { {k: round(v, 3) for k, v in st.items()} }", flush=True)
        lib.ZSTD_freeDCtx(d)
    lib.ZSTD_freeDDict(dd)


switch_cost()
contexts()
decode()
