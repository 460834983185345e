"""Many dictionaries in one batch (ZSTDMI_compressBatchCDicts) against one ZSTD_CCtx_refCDict + ZSTDMI_compressBatch round per
dictionary, run on the GPU box: the mirror of tools/ddict_set_time.py.  Device-resident entries; every figure is the best of 3 after a
warm-up of the same shape, the host clock stopped after the final synchronise; every output is decoded (ZSTD_d_refMultipleDDicts) and
compared with the records; stage times through ZSTDMI_CCtx_getStageTimes.
  workload : [records] (default 65 536) text records of 4 KiB, and the 1000 JSON records (tests/golden/make_golden_train.py) tiled to
             the same count, at level 3 with ZSTDMI_CCtx_setDictEntropy, setDictIndex and setDictIndexStrategy(2) on, record i behind
             dictionary i mod K for K = 1, 4, 16, 64: trained_16k.dict / train_default_json.dict with bytes 4..7 rewritten, each a CDict
             of its own with its own device copy.
  (a) rounds : the entries grouped by dictionary, K rounds of ZSTD_CCtx_refCDict + ZSTDMI_compressBatch on one context; with
             --parent LIB by the library at LIB as well (the parent commit's build), alternating with this one's in the same session.
  (b) one call : this library, ONE ZSTDMI_compressBatchCDicts over all entries in their round-robin order.
At K = 1 every entry names one CDict, so (b) launches the single-dictionary kernels; its three runs are printed beside the best.
python tools/cdict_batch_time.py [records] [--parent LIB]"""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen
import make_golden_train as mgt
from zstdsharp_amd import _ffi
lib = _ffi.load()
GOLDEN = os.path.join(ROOT, "tests", "golden")
args = sys.argv[1:]
parent = None
if "--parent" in args:
    at = args.index("--parent")
    parent = ctypes.CDLL(os.path.abspath(args[at + 1]))
    for name, (res, argtypes) in _ffi.SIGNATURES.items():
        if hasattr(parent, name):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = res, argtypes
    del args[at:at + 2]
records = int(args[0]) if args else 65536
REC = 4096
STAGES = ("lz_fast", "lz_region", "huf_hist", "huf_tree", "huf_encode", "seq_encode")


def golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def runs_of(f, n=3):
    f()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts


def stage_times(L, c):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = L.ZSTDMI_CCtx_getStageTimes(c, ms, names, 24)
    out = {}
    for i in range(k):
        out[names[i].decode()] = out.get(names[i].decode(), 0.0) + float(ms[i])
    return out


def add(acc, st):
    for k, v in st.items():
        acc[k] = acc.get(k, 0.0) + v


def context(L):
    c = L.ZSTD_createCCtx()
    assert not z.errors.is_error(L.ZSTD_CCtx_setParameter(c, 100, 3))      # (ZSTD_c_compressionLevel; the call returns the level)
    assert L.ZSTDMI_CCtx_setDictEntropy(c, 1) == 0 and L.ZSTDMI_CCtx_setDictIndex(c, 1) == 0 and L.ZSTDMI_CCtx_setDictIndexStrategy(c, 2) == 0
    return c


def workload(kind):
    n = records
    if kind == "text":
        flat = np.resize(np.frombuffer(datagen.gen("text", 16 << 20, 3), dtype=np.uint8), n * REC)
    else:
        flat = np.resize(np.frombuffer(b"".join(mgt.json_records(1000, 77)), dtype=np.uint8), n * REC)      # (tiled, then cut into 4 KiB entries)
    return torch.from_numpy(flat.copy()).cuda()


def arrays(src, out, cap, idx):
    m = len(idx)
    return ((ctypes.c_void_p * m)(*[src.data_ptr() + i * REC for i in idx]), (ctypes.c_size_t * m)(*([REC] * m)), m,
            (ctypes.c_void_p * m)(*[out.data_ptr() + i * cap for i in idx]), (ctypes.c_size_t * m)(*([cap] * m)), (ctypes.c_size_t * m)())


def check(src, out, cap, sizes, dicts):
    """every entry decodes to its record behind the dictionary its header names"""
    n = len(sizes)
    with z.Decompressor() as d:
        d.SetParameter(z.ZSTD_d_refMultipleDDicts, 1)
        dds = [z.DDict(b) for b in dicts]
        for dd in dds:
            d.RefDDict(dd)
        back = z.decompress_batch(d, [out[i * cap:i * cap + sizes[i]] for i in range(n)], [REC] * n)
        ok = bool(torch.equal(torch.cat(back), src))
        d.RefDDict(None)
        for dd in dds:
            dd.Dispose()
    assert ok, "an entry does not decode to its record"


def rounds(L, src, out, cap, dicts):
    """(a): K rounds of refCDict + compressBatch, entries grouped by dictionary"""
    K, n = len(dicts), records
    cds = [L.ZSTD_createCDict(b, len(b), 3) for b in dicts]
    assert all(cds)
    c = context(L)
    groups = [arrays(src, out, cap, list(range(k, n, K))) for k in range(K)]
    acc = {}

    def call(stages=False):
        for k in range(K):
            assert L.ZSTD_CCtx_refCDict(c, cds[k]) == 0
            a = groups[k]
            assert L.ZSTDMI_compressBatch(c, a[0], a[1], a[2], a[3], a[4], a[5]) == 0
            if stages:
                add(acc, stage_times(L, c))
    ts = runs_of(call)                      # (timed with profiling off; the stage times come from one more pass with it on)
    sizes = [0] * n
    for k in range(K):
        for j, i in enumerate(range(k, n, K)):
            sizes[i] = groups[k][5][j]
    check(src, out, cap, sizes, dicts)
    L.ZSTDMI_CCtx_setProfiling(c, 1)
    call(True)
    L.ZSTD_CCtx_refCDict(c, None)
    L.ZSTD_freeCCtx(c)
    for cd in cds:
        L.ZSTD_freeCDict(cd)
    return ts, dict(acc), sum(sizes)


def one_call(src, out, cap, dicts):
    """(b): one compressBatchCDicts over all entries"""
    K, n = len(dicts), records
    cds = [lib.ZSTD_createCDict(b, len(b), 3) for b in dicts]
    assert all(cds)
    c = context(lib)
    a = arrays(src, out, cap, list(range(n)))
    handles = (ctypes.c_void_p * n)(*[cds[i % K] for i in range(n)])

    def call():
        assert lib.ZSTDMI_compressBatchCDicts(c, a[0], a[1], a[2], a[3], a[4], a[5], handles) == 0
    ts = runs_of(call)
    check(src, out, cap, list(a[5]), dicts)
    lib.ZSTDMI_CCtx_setProfiling(c, 1)
    call()
    st = stage_times(lib, c)
    passes, chunks = lib.ZSTDMI_debugLastBatchPasses(c), lib.ZSTDMI_debugLastBatchSetChunks(c)
    assert chunks == (n if K > 1 else 0) and lib.ZSTDMI_debugLastBatchAlone(c) == 0 and lib.ZSTDMI_debugDictUploads(c) == 0
    lib.ZSTD_freeCCtx(c)
    for cd in cds:
        lib.ZSTD_freeCDict(cd)
    return ts, st, sum(a[5]), passes, chunks


def row(label, ts, st):
    return (f"    {label:14s}: call {min(ts) * 1e3:8.3f} ms (runs {' '.join(f'{t * 1e3:.3f}' for t in ts)})  " +
            "  ".join(f"{k} {st.get(k, 0.0):.3f}" for k in STAGES if k in st) + " ms")


for kind, name in (("text", "trained_16k.dict"), ("json", "train_default_json.dict")):
    src = workload(kind)
    cap = (lib.ZSTD_compressBound(REC) + 63) & ~63
    out = torch.empty(records * cap, dtype=torch.uint8, device="cuda")
    base = golden(name)
    for K in (1, 4, 16, 64):
        dicts = [base[:4] + (0x51000000 + k).to_bytes(4, "little") + base[8:] for k in range(K)]
        print(f"{kind}: {records} x 4 KiB, level 3, entropy + index + strategy 2 on, {name} x {K} dictIDs", flush=True)
        results = []
        for rep in range(2 if parent is not None else 1):        # (parent and this library alternate)
            if parent is not None:
                ts, st, total = rounds(parent, src, out, cap, dicts)
                results.append(("parent rounds", ts, st, total))
            ts, st, total = rounds(lib, src, out, cap, dicts)
            results.append(("rounds", ts, st, total))
            ts, st, total, passes, chunks = one_call(src, out, cap, dicts)
            results.append(("one call", ts, st, total))
        assert len({r[3] for r in results}) == 1, "the three ways wrote different sizes"
        for label, ts, st, _ in results:
            print(row(label, ts, st), flush=True)
        a = min(min(r[1]) for r in results if r[0] == ("parent rounds" if parent is not None else "rounds"))
        b = min(min(r[1]) for r in results if r[0] == "one call")
        print(f"    (a)/(b) = {a / b:.2f}  ({results[-1][3]} compressed bytes; one call: {passes} passes, {chunks} chunks in set instances)", flush=True)
        print(f"    one call stages ms { {k: round(v, 3) for k, v in results[-1][2].items()} }", flush=True)
    del src, out
    torch.cuda.empty_cache()
