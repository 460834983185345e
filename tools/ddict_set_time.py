"""Many dictionaries behind one context (ZSTD_d_refMultipleDDicts) against one ZSTD_DCtx_refDDict + ZSTDMI_decompressBatch round per
dictionary, run on the GPU box.  Device-resident entries; every figure is the best of 3 after a warm-up of the same shape, the host clock
stopped after the final synchronise; every output is compared with the records; stage times through ZSTDMI_DCtx_getStageTimes.
  workload : [records] (default 65 536) text records of 4 KiB at level 3 with ZSTDMI_CCtx_setDictEntropy on, and the 1000 JSON records
             (tests/golden/make_golden_train.py) tiled to the same count, spread round-robin over K = 1, 4, 16, 64 dictionaries:
             trained_16k.dict / train_default_json.dict with bytes 4..7 rewritten, each a DDict of its own with its own device copy.
  (a) rounds : the entries grouped by dictionary, K rounds of ZSTD_DCtx_refDDict + ZSTDMI_decompressBatch on one context; with
             --parent LIB by the library at LIB as well (the parent commit's build), alternating with this one's in the same session.
  (b) set    : this library, the parameter on, ONE ZSTDMI_decompressBatch over all entries in their round-robin order.
At K = 1 the set holds one DDict, so (b) launches the single-dictionary kernels; its three runs' spread is printed beside the best.
python tools/ddict_set_time.py [records] [--parent LIB]"""
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


def stage_times(L, d):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = L.ZSTDMI_DCtx_getStageTimes(d, ms, names, 24)
    out = {}
    for i in range(k):
        out[names[i].decode()] = out.get(names[i].decode(), 0.0) + float(ms[i])
    return out


def pick(st):
    lits = sum(v for k, v in st.items() if "literal" in k and k != "place_literals")
    return st.get("seq_decode", 0.0), lits, st.get("exec_matches", 0.0)


def add(acc, st):
    for k, v in st.items():
        acc[k] = acc.get(k, 0.0) + v


def workload(kind, base_dict, K):
    """n records behind K copies of the dictionary, record i behind copy i % K -> (the records on the device, the compressed entries)"""
    n = records
    if kind == "text":
        flat = np.resize(np.frombuffer(datagen.gen("text", 16 << 20, 3), dtype=np.uint8), n * REC)
    else:
        flat = np.resize(np.frombuffer(b"".join(mgt.json_records(1000, 77)), dtype=np.uint8), n * REC)      # (tiled, then cut into 4 KiB entries)
    src = torch.from_numpy(flat.copy()).cuda()
    dicts = [base_dict[:4] + (0x51000000 + k).to_bytes(4, "little") + base_dict[8:] for k in range(K)]
    comp = [None] * n
    with z.Compressor(3) as c:
        c.dict_entropy = True
        for k in range(K):
            c.LoadDictionary(dicts[k])
            idx = list(range(k, n, K))
            for i, t in zip(idx, z.compress_batch(c, [src[i * REC:(i + 1) * REC] for i in idx])):
                comp[i] = t
    return src, comp, dicts


def arrays(comp, out, idx):
    m = len(idx)
    return ((ctypes.c_void_p * m)(*[comp[i].data_ptr() for i in idx]), (ctypes.c_size_t * m)(*[comp[i].numel() for i in idx]), m,
            (ctypes.c_void_p * m)(*[out.data_ptr() + i * REC for i in idx]), (ctypes.c_size_t * m)(*([REC] * m)), (ctypes.c_size_t * m)())


def rounds(L, comp, dicts, src, out):
    """(a): K rounds of refDDict + decompressBatch, entries grouped by dictionary"""
    K, n = len(dicts), len(comp)
    dds = [L.ZSTD_createDDict(d, len(d)) for d in dicts]
    assert all(dds)
    d = L.ZSTD_createDCtx()
    groups = [arrays(comp, out, list(range(k, n, K))) for k in range(K)]
    acc = {}

    def call(stages=False):
        for k in range(K):
            assert L.ZSTD_DCtx_refDDict(d, dds[k]) == 0
            a = groups[k]
            assert L.ZSTDMI_decompressBatch(d, a[0], a[1], a[2], a[3], a[4], a[5]) == 0
            if stages:
                add(acc, stage_times(L, d))
    out.zero_()
    ts = runs_of(call)                      # (timed with profiling off; the stage times come from one more pass with it on)
    assert all(g == REC for a in groups for g in a[5]) and bool(torch.equal(out, src)), "rounds"
    L.ZSTDMI_DCtx_setProfiling(d, 1)
    call(True)
    L.ZSTD_DCtx_refDDict(d, None)
    L.ZSTD_freeDCtx(d)
    for dd in dds:
        L.ZSTD_freeDDict(dd)
    return ts, dict(acc)


def one_call(comp, dicts, src, out):
    """(b): the set, one decompressBatch over all entries"""
    n = len(comp)
    dds = [lib.ZSTD_createDDict(d, len(d)) for d in dicts]
    assert all(dds)
    d = lib.ZSTD_createDCtx()
    assert lib.ZSTD_DCtx_setParameter(d, z.ZSTD_d_refMultipleDDicts, 1) == 0
    for dd in dds:
        assert lib.ZSTD_DCtx_refDDict(d, dd) == 0
    a = arrays(comp, out, list(range(n)))

    def call():
        assert lib.ZSTDMI_decompressBatch(d, a[0], a[1], a[2], a[3], a[4], a[5]) == 0
    out.zero_()
    ts = runs_of(call)
    assert all(g == REC for g in a[5]) and bool(torch.equal(out, src)), "set"
    lib.ZSTDMI_DCtx_setProfiling(d, 1)
    call()
    st = stage_times(lib, d)
    found = lib.ZSTDMI_debugLastSetFrames(d)
    assert found == (n if len(dicts) > 1 else 0) and lib.ZSTDMI_debugDictUploadsD(d) == 0
    lib.ZSTD_DCtx_refDDict(d, None)
    lib.ZSTD_freeDCtx(d)
    for dd in dds:
        lib.ZSTD_freeDDict(dd)
    return ts, st, found


def row(label, ts, st):
    s, l, e = pick(st)
    return (f"    {label:14s}: call {min(ts) * 1e3:8.3f} ms (runs {' '.join(f'{t * 1e3:.3f}' for t in ts)})  seq_decode {s:7.3f}  literal stage {l:7.3f}  "
            f"exec_matches {e:7.3f} ms")


for kind, name in (("text", "trained_16k.dict"), ("json", "train_default_json.dict")):
    for K in (1, 4, 16, 64):
        src, comp, dicts = workload(kind, golden(name), K)
        out = torch.empty(records * REC, dtype=torch.uint8, device="cuda")
        print(f"{kind}: {records} x 4 KiB, level 3, dictionary entropy on, {name} x {K} dictIDs, {sum(t.numel() for t in comp)} compressed bytes", flush=True)
        results = []
        for rep in range(2 if parent is not None else 1):        # (parent and this library alternate)
            if parent is not None:
                results.append(("parent rounds", ) + rounds(parent, comp, dicts, src, out))
            results.append(("rounds", ) + rounds(lib, comp, dicts, src, out))
            ts, st, found = one_call(comp, dicts, src, out)
            results.append(("set, one call", ts, st))
        for label, ts, st in results:
            print(row(label, ts, st), flush=True)
        a = min(min(ts) for label, ts, _ in results if label == ("parent rounds" if parent is not None else "rounds"))
        b = min(min(ts) for label, ts, _ in results if label == "set, one call")
        print(f"    (a)/(b) = {a / b:.2f}  (frames found in the set: {found})", flush=True)
        print(f"    set stages ms { {k: round(v, 3) for k, v in results[-1][2].items()} }", flush=True)
        del src, comp, out
        torch.cuda.empty_cache()
