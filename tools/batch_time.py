"""Batched calls against a loop of single calls (run on the GPU box): 256 MiB of device-resident entries of 4 KiB, 16 KiB and 64 KiB
(65 536, 16 384 and 4096 entries), text and Zipf bytes at levels 1 and 3, 4 KiB text records at level 3 with
tests/golden/trained_16k.dict, and entries of several blocks — 256 KiB (1024 entries) and 1 MiB (256 entries), the multi-block frames
with history of the default settings — at the same kinds and levels.  Per point, compress and decompress:
  (a) loop   : one ZSTDMI_compressDevice / ZSTDMI_decompressDevice call per entry (timed on the first 4096 entries, scaled to all)
  (b) batch  : one ZSTDMI_compressBatch / ZSTDMI_decompressBatch call
  (c) concat : one single call on the concatenation — a different product (the entries are not decodable on their own), the ceiling
  (d) the batch call's stage times (ZSTDMI_*_getStageTimes)
Best of 3 after a warm-up call of the same shape; the host clock stops after the call's final synchronise (every call ends with one).
The input is 16 MiB of generated data repeated (entries are independent, so the repeats are nobody's match).
python tools/batch_time.py [MiB] [--dict-entropy] [--dict-row] [--frames-rows] [--measure-only] [--dict-index-rows] [--dict-index]
                           [--level=N] [--dict-index-strategy=N] [--dict-index-chain] [--unsized-rows] [--batch-unsized] [--async]
  --async        : only the rows of ZSTDMI_compressBatchAsync: text entries of 4 KiB at levels 1 and 3, the descriptors as CUDA tensors.
                   One ZSTDMI_CCtx_prepareBatchAsync for a pass of 16 384 entries (the pass limit), then per measurement one async call
                   per 16 384 entries back to back on the context's stream: (a) until the last call has returned, (b) until a following
                   hipStreamSynchronize (torch.cuda.synchronize) has returned, and (c) the synchronous ZSTDMI_compressBatch of the same
                   entries in the same session, its final wait included.  The bytes of both are compared afterwards.
                   Then the decode rows (ZSTDMI_decompressBatchAsync) over those frames: one ZSTDMI_DCtx_prepareBatchAsync per row with
                   limits of 1x, 4x and 16x what the call holds, all entries in one async call per measurement, the same (a), (b), and
                   (c) ZSTDMI_decompressBatch in the same session; every entry's size and bytes are compared afterwards.
                   Then the rows of ZSTDMI_CCtx_prepareBatchAsyncLimits: text entries of 256 KiB at levels 1 and 3, the same (a), (b),
                   (c): all entries in one async call; 256 entries per call with a grid of exactly the chunk slots the entries fill;
                   and 256 per call with four times as many slots (a bound of 1 MiB), the price of surplus slots.
  --unsized-rows : only the rows of ZSTDMI_DCtx_setBatchUnsized, decompression alone: text and Zipf entries of 4 KiB at level 3,
                   (a) written with content sizes, one batch call; (b) written with ZSTD_c_contentSizeFlag = 0 and the window restated as
                   the 2^19 a streaming encoder declares (each frame's bound: 128 KiB), the switch off — every entry goes alone: timed on
                   the first 4096 entries and scaled as the loop column is —; (c) those with the switch on, one batch call; the stage
                   times of (a) and (c) and what (c) asked its work buffers for.  Every entry is compared afterwards.
  --batch-unsized : those rows with column (c) (without it the call is not made, so (a) and (b) also run on a library from before the switch)
  --dict-index-rows : only the rows of ZSTDMI_CCtx_setDictIndex, batch calls alone: 4 KiB text entries at level 1 with
                   tests/golden/train_default_text.dict, and the 1000 held-out JSON records of tests/golden/make_golden_train.py
                   tiled to the total with train_default_json.dict; the ratio, the batch call's ms and its stage times
  --dict-index   : those rows with the switch on (without it they also run on a library from before the switch existed)
  --level=N      : those rows at level N instead of 1 (3: the dual-hash finder)
  --dict-index-strategy=N : those rows with ZSTDMI_CCtx_setDictIndexStrategy(N) (2: the index also serves level 3; without the flag the
                   call is not made, so the rows also run on a library from before it existed)
  --dict-index-chain : those rows with ZSTDMI_CCtx_setDictIndexChain(1) (the index also serves the levels >= 5; without the flag the call
                   is not made, so the rows also run on a library from before it existed)
  --dict-entropy : the dictionary row with ZSTDMI_CCtx_setDictEntropy on (the dictionary's entropy tables in the compressor)
  --dict-row     : only the dictionary row
  --frames-rows  : only the 256 KiB and 1 MiB rows
  --measure-only : no assertion that every entry took the batched pass and that the batch beats the loop; the number of entries that
                   went alone is printed instead (for a library from before the multi-block rows were batched: the "before" column)"""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen
lib = z._ffi.load()
MiB = 1 << 20
FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
VALUED = {f.split("=", 1)[0]: int(f.split("=", 1)[1]) for f in FLAGS if "=" in f}
FLAGS = [f for f in FLAGS if "=" not in f]
assert all(f in ("--dict-entropy", "--dict-row", "--frames-rows", "--measure-only", "--dict-index-rows", "--dict-index", "--dict-index-chain", "--unsized-rows", "--batch-unsized", "--async") for f in FLAGS), FLAGS
assert all(f in ("--level", "--dict-index-strategy") for f in VALUED), VALUED
DICT_INDEX_ROWS, DICT_INDEX = "--dict-index-rows" in FLAGS, "--dict-index" in FLAGS
INDEX_LEVEL, INDEX_STRATEGY, INDEX_CHAIN = VALUED.get("--level", 1), VALUED.get("--dict-index-strategy"), "--dict-index-chain" in FLAGS
UNSIZED_ROWS, BATCH_UNSIZED = "--unsized-rows" in FLAGS, "--batch-unsized" in FLAGS
DICT_ENTROPY, DICT_ROW, FRAMES_ROWS, MEASURE_ONLY = "--dict-entropy" in FLAGS, "--dict-row" in FLAGS, "--frames-rows" in FLAGS, "--measure-only" in FLAGS
total = (int(ARGS[0]) if ARGS else 256) * MiB
SAMPLE = 4096
DICT = open(os.path.join(ROOT, "tests", "golden", "trained_16k.dict"), "rb").read()


def stage_times(get, ctx):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = get(ctx, ms, names, 24)
    return " ".join(f"{names[i].decode()} {float(ms[i]):.2f}" for i in range(k))


def best_of(f, reps=3):
    f()                                     # warm-up: same shape, workspaces allocated
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        best = min(best, time.perf_counter() - t0)
    return best


def ptrs(base, offs):
    return (ctypes.c_void_p * len(offs))(*[base + o for o in offs])


def sizes(vals):
    return (ctypes.c_size_t * len(vals))(*vals)


def ok(r):
    assert not lib.ZSTD_isError(r), lib.ZSTD_getErrorName(r)
    return r


def dict_index_rows():
    golden = os.path.join(ROOT, "tests", "golden")
    sys.path.insert(0, golden)
    import make_golden_train as mgt
    text = datagen.gen("text", 16 * MiB, 5) * (total // (16 * MiB))
    recs = mgt.json_records(2000, 77)[1000:]
    json_blob = b"".join(recs); json_sizes = [len(r) for r in recs]
    reps = total // len(json_blob)
    rows = [(f"text 4 KiB L{INDEX_LEVEL} train_default_text", "train_default_text.dict", text, [4096] * (total // 4096)),
            (f"json records L{INDEX_LEVEL} train_default_json", "train_default_json.dict", json_blob * reps, json_sizes * reps)]
    print(f"level {INDEX_LEVEL}; dictionary index {'on' if DICT_INDEX else 'off'}, up to strategy {INDEX_STRATEGY if INDEX_STRATEGY else '1 (not set)'}, chain finder {'on' if INDEX_CHAIN else 'off'}; "
          f"entropy tables {'on' if DICT_ENTROPY else 'off'}", flush=True)
    for name, dname, blob, szs in rows:
        dic = open(os.path.join(golden, dname), "rb").read()
        src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        n = len(szs)
        offs = np.concatenate(([0], np.cumsum(szs)[:-1])).tolist()
        caps = [lib.ZSTD_compressBound(x) for x in szs]
        coffs = np.concatenate(([0], np.cumsum(caps)[:-1])).tolist()
        dst = torch.empty(sum(caps) + 64, dtype=torch.uint8, device="cuda")
        out = torch.empty(len(blob), dtype=torch.uint8, device="cuda")
        c, d = lib.ZSTD_createCCtx(), lib.ZSTD_createDCtx()
        lib.ZSTD_CCtx_setParameter(c, 100, INDEX_LEVEL)
        if DICT_INDEX:
            ok(lib.ZSTDMI_CCtx_setDictIndex(c, 1))
        if INDEX_STRATEGY:
            ok(lib.ZSTDMI_CCtx_setDictIndexStrategy(c, INDEX_STRATEGY))
        if INDEX_CHAIN:
            ok(lib.ZSTDMI_CCtx_setDictIndexChain(c, 1))
        if DICT_ENTROPY:
            ok(lib.ZSTDMI_CCtx_setDictEntropy(c, 1))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ok(lib.ZSTD_CCtx_loadDictionary(c, dic, len(dic)))
        tiny = (ctypes.c_size_t * 1)()
        ok(lib.ZSTDMI_compressBatch(c, ptrs(src.data_ptr(), [0]), sizes([8]), 1, ptrs(dst.data_ptr(), [0]), sizes([caps[0]]), tiny))
        load_ms = (time.perf_counter() - t0) * 1e3       # the load, the dictionary's upload (and index) and one 8-byte entry
        ok(lib.ZSTD_DCtx_loadDictionary(d, dic, len(dic)))
        s_ptr, d_ptr, o_ptr = ptrs(src.data_ptr(), offs), ptrs(dst.data_ptr(), coffs), ptrs(out.data_ptr(), offs)
        s_sz, d_cap, got, back = sizes(szs), sizes(caps), (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
        lib.ZSTDMI_CCtx_setProfiling(c, 1)
        cb = best_of(lambda: ok(lib.ZSTDMI_compressBatch(c, s_ptr, s_sz, n, d_ptr, d_cap, got)))
        assert not any(lib.ZSTD_isError(g) for g in got) and lib.ZSTDMI_debugLastBatchAlone(c) == 0
        cst = stage_times(lib.ZSTDMI_CCtx_getStageTimes, c)
        ok(lib.ZSTDMI_decompressBatch(d, d_ptr, got, n, o_ptr, s_sz, back))
        assert list(back) == szs and bool(torch.equal(out, src))
        print(f"| {name:36s} | {n:7d} | ratio {sum(got) / len(blob):.4f} | batch {cb * 1e3:7.2f} ms | load + first call {load_ms:6.2f} ms |\n    compress stages ms: {cst}", flush=True)
        lib.ZSTD_freeCCtx(c); lib.ZSTD_freeDCtx(d)
        del src, dst, out
        torch.cuda.empty_cache()


def unsized_rows():
    size, level = 4096, 3
    n = total // size
    cap = lib.ZSTD_compressBound(size)
    offs = [i * size for i in range(n)]
    coffs = [i * cap for i in range(n)]
    print(f"{n} entries of 4 KiB at level {level}; ms per call of all entries (GB/s of content)", flush=True)
    for kind in ("text", "zipf"):
        src = torch.from_numpy(np.frombuffer(datagen.gen(kind, 16 * MiB, 5), dtype=np.uint8).copy()).cuda().repeat(total // (16 * MiB))
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        blobs = {}
        for flag in (1, 0):
            dst = torch.empty(n * cap + MiB, dtype=torch.uint8, device="cuda")
            c = lib.ZSTD_createCCtx()
            lib.ZSTD_CCtx_setParameter(c, 100, level); ok(lib.ZSTD_CCtx_setParameter(c, 200, flag))
            got = (ctypes.c_size_t * n)()
            ok(lib.ZSTDMI_compressBatch(c, ptrs(src.data_ptr(), offs), sizes([size] * n), n, ptrs(dst.data_ptr(), coffs), sizes([cap] * n), got))
            assert not any(lib.ZSTD_isError(g) for g in got)
            lib.ZSTD_freeCCtx(c)
            if not flag:            # byte 5 is the window descriptor of a frame without a content size: 2^19
                at = torch.tensor(coffs, dtype=torch.int64, device="cuda")
                assert bool((dst[at + 4] & 0xE0).eq(0).all()), "a frame carries a content size"
                dst[at + 5] = (19 - 10) << 3
                torch.cuda.synchronize()
            blobs[flag] = (dst, got, ptrs(dst.data_ptr(), coffs))
        s_sz, back, o_ptr = sizes([size] * n), (ctypes.c_size_t * n)(), ptrs(out.data_ptr(), offs)

        def run(d, flag, m=n):
            dst, got, d_ptr = blobs[flag]
            ok(lib.ZSTDMI_decompressBatch(d, d_ptr, got, m, o_ptr, s_sz, back))

        def checked(d, flag, m=n):
            out.zero_(); run(d, flag, m)
            assert all(back[i] == size for i in range(m)) and bool(torch.equal(out[:m * size], src[:m * size]))

        d = lib.ZSTD_createDCtx(); lib.ZSTDMI_DCtx_setProfiling(d, 1)
        ta = best_of(lambda: run(d, 1)); checked(d, 1)
        assert lib.ZSTDMI_debugLastBatchAloneD(d) == 0
        sta = stage_times(lib.ZSTDMI_DCtx_getStageTimes, d)
        lib.ZSTD_freeDCtx(d)
        d = lib.ZSTD_createDCtx()
        m = min(n, SAMPLE)
        tb = best_of(lambda: run(d, 0, m)) * n / m; checked(d, 0, m)
        assert lib.ZSTDMI_debugLastBatchAloneD(d) == m
        lib.ZSTD_freeDCtx(d)
        gbs = lambda t: total / t / 1e9
        line = f"| {kind} 4 KiB L{level} | {n:6d} | (a) sized {ta * 1e3:7.2f} ({gbs(ta):6.1f}) | (b) unsized, switch off {tb * 1e3:9.1f} ({gbs(tb):6.3f}) |"
        if BATCH_UNSIZED:
            d = lib.ZSTD_createDCtx(); lib.ZSTDMI_DCtx_setProfiling(d, 1)
            ok(lib.ZSTDMI_DCtx_setBatchUnsized(d, 1))
            tc = best_of(lambda: run(d, 0)); checked(d, 0)
            assert lib.ZSTDMI_debugLastBatchAloneD(d) == 0
            stc, ws = stage_times(lib.ZSTDMI_DCtx_getStageTimes, d), lib.ZSTDMI_debugLastBatchWorkspace(d)
            lib.ZSTD_freeDCtx(d)
            line += f" (c) unsized, switch on {tc * 1e3:7.2f} ({gbs(tc):6.1f}) | workspace {ws / MiB:.1f} MiB |\n    (c) stages ms: {stc}"
        print(line + f"\n    (a) stages ms: {sta}", flush=True)
        del src, out, blobs
        torch.cuda.empty_cache()


def async_rows():
    size, pass_entries = 4096, 16384
    n = total // size
    cap = lib.ZSTD_compressBound(size)
    src = torch.from_numpy(np.frombuffer(datagen.gen("text", 16 * MiB, 5), dtype=np.uint8).copy()).cuda().repeat(total // (16 * MiB))
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    print(f"{n} text entries of 4 KiB; ms for all entries (GB/s of content)", flush=True)
    for level in (1, 3):
        dst_a = torch.zeros(n * cap + MiB, dtype=torch.uint8, device="cuda")
        dst_s = torch.zeros(n * cap + MiB, dtype=torch.uint8, device="cuda")
        c, cs = lib.ZSTD_createCCtx(), lib.ZSTD_createCCtx()
        for x in (c, cs):
            lib.ZSTD_CCtx_setParameter(x, 100, level)
        ok(lib.ZSTDMI_CCtx_prepareBatchAsync(c, pass_entries, size))
        ok(lib.ZSTDMI_CCtx_setStream(c, torch.cuda.current_stream().cuda_stream or 1))      # (1: hipStreamLegacy, torch's default stream)
        srcs, dsts = src.data_ptr() + idx * size, dst_a.data_ptr() + idx * cap
        szs, caps = torch.full((n,), size, dtype=torch.int64, device="cuda"), torch.full((n,), cap, dtype=torch.int64, device="cuda")
        out = torch.empty(n, dtype=torch.int64, device="cuda")
        returned = [0.0]

        def enqueue():
            t0 = time.perf_counter()
            for at in range(0, n, pass_entries):
                m = min(pass_entries, n - at)
                ok(lib.ZSTDMI_compressBatchAsync(c, srcs.data_ptr() + 8 * at, szs.data_ptr() + 8 * at, m, dsts.data_ptr() + 8 * at, caps.data_ptr() + 8 * at, out.data_ptr() + 8 * at))
            returned[0] = time.perf_counter() - t0
            torch.cuda.synchronize()

        waits = lib.ZSTDMI_debugHostWaits(c)
        ret, done = 1e9, 1e9
        enqueue()
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            enqueue()
            done = min(done, time.perf_counter() - t0); ret = min(ret, returned[0])
        assert lib.ZSTDMI_debugHostWaits(c) == waits
        s_ptr, d_ptr = ptrs(src.data_ptr(), [i * size for i in range(n)]), ptrs(dst_s.data_ptr(), [i * cap for i in range(n)])
        s_sz, d_cap, got = sizes([size] * n), sizes([cap] * n), (ctypes.c_size_t * n)()
        sync = best_of(lambda: ok(lib.ZSTDMI_compressBatch(cs, s_ptr, s_sz, n, d_ptr, d_cap, got)))
        assert out.cpu().tolist() == list(got) and bool(torch.equal(dst_a, dst_s))
        gbs = lambda t: total / t / 1e9
        print(f"| text 4 KiB L{level} | {n:6d} | ratio {sum(got) / total:.3f} | (a) async calls returned {ret * 1e3:7.2f} | (b) ... and the stream drained {done * 1e3:7.2f} ({gbs(done):6.1f}) "
              f"| (c) synchronous batch {sync * 1e3:7.2f} ({gbs(sync):6.1f}) |", flush=True)
        lib.ZSTD_freeCCtx(c); lib.ZSTD_freeCCtx(cs)
        del dst_a
        async_decode_rows(level, n, size, cap, src, dst_s, got)
        del dst_s
        torch.cuda.empty_cache()


def async_decode_rows(level, n, size, cap, src, comp, got):
    """the decode rows of --async: the frames the synchronous compress batch has just written, all entries in ONE ZSTDMI_decompressBatchAsync
    call per measurement, under limits of 1x, 4x and 16x what the call holds (n frames, n blocks, the content; sequence records: the
    default maxContent / 3 + 64 of that content), against ZSTDMI_decompressBatch of the same build"""
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    out_a = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
    out_s = torch.zeros(n * size, dtype=torch.uint8, device="cuda")
    srcs, dsts = comp.data_ptr() + idx * cap, out_a.data_ptr() + idx * size
    szs = torch.tensor(list(got), dtype=torch.int64, device="cuda")
    caps = torch.full((n,), size, dtype=torch.int64, device="cuda")
    back = torch.empty(n, dtype=torch.int64, device="cuda")
    gbs = lambda t: n * size / t / 1e9
    ds = lib.ZSTD_createDCtx()
    c_ptr, o_ptr = ptrs(comp.data_ptr(), [i * cap for i in range(n)]), ptrs(out_s.data_ptr(), [i * size for i in range(n)])
    o_cap, back_s = sizes([size] * n), (ctypes.c_size_t * n)()
    sync = best_of(lambda: ok(lib.ZSTDMI_decompressBatch(ds, c_ptr, got, n, o_ptr, o_cap, back_s)))
    assert all(b == size for b in back_s) and bool(torch.equal(out_s, src[:n * size]))
    lib.ZSTD_freeDCtx(ds)
    for k in (1, 4, 16):
        d = lib.ZSTD_createDCtx()
        content = k * n * size
        lim = z._ffi.DBatchLimits(n, cap, content, k * n, k * n, content // 3 + 64)
        ok(lib.ZSTDMI_DCtx_prepareBatchAsync(d, ctypes.byref(lim)))
        ok(lib.ZSTDMI_DCtx_setStream(d, torch.cuda.current_stream().cuda_stream or 1))
        returned = [0.0]

        def enqueue():
            t0 = time.perf_counter()
            ok(lib.ZSTDMI_decompressBatchAsync(d, srcs.data_ptr(), szs.data_ptr(), n, dsts.data_ptr(), caps.data_ptr(), back.data_ptr()))
            returned[0] = time.perf_counter() - t0
            torch.cuda.synchronize()

        waits = lib.ZSTDMI_debugHostWaitsD(d)
        ret, done = 1e9, 1e9
        enqueue()
        for _ in range(3):
            out_a.zero_(); torch.cuda.synchronize(); t0 = time.perf_counter()
            enqueue()
            done = min(done, time.perf_counter() - t0); ret = min(ret, returned[0])
        assert lib.ZSTDMI_debugHostWaitsD(d) == waits
        assert bool((back == size).all()) and bool(torch.equal(out_a, src[:n * size]))
        print(f"| decode text 4 KiB L{level} | {n:6d} | limits {k:2d}x ({lib.ZSTDMI_batchAsyncWorkspaceD(ctypes.byref(lim)) / MiB:8.1f} MiB) | (a) async call returned {ret * 1e3:7.2f} "
              f"| (b) ... and the stream drained {done * 1e3:7.2f} ({gbs(done):6.1f}) | (c) synchronous batch {sync * 1e3:7.2f} ({gbs(sync):6.1f}) |", flush=True)
        lib.ZSTD_freeDCtx(d)
    del out_a, out_s


def async_frames_rows():
    """the rows of ZSTDMI_CCtx_prepareBatchAsyncLimits: text entries of 256 KiB, all in one async call, then 256 per call back to back.
    A call's grid is min(maxChunks, n * ceil(bound / chunkBytes)) chunk slots, so surplus slots come from a bound above the entries:
    the 1x rows prepare the entries' own size (every slot filled; bytes compared with the synchronous batch), the 4x row a bound of
    1 MiB (four slots launched per slot filled, which fits the pass limit at 256 entries per call; another tier, so only sizes and
    ratio are compared)."""
    size = 256 << 10
    n = total // size
    src = torch.from_numpy(np.frombuffer(datagen.gen("text", 16 * MiB, 5), dtype=np.uint8).copy()).cuda().repeat(total // (16 * MiB))
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    cap = lib.ZSTD_compressBound(size)
    print(f"{n} text entries of 256 KiB; ms for all entries (GB/s of content)", flush=True)
    for level in (1, 3):
        dst_s = torch.zeros(n * cap + MiB, dtype=torch.uint8, device="cuda")
        cs = lib.ZSTD_createCCtx()
        lib.ZSTD_CCtx_setParameter(cs, 100, level)
        s_ptr, d_ptr = ptrs(src.data_ptr(), [i * size for i in range(n)]), ptrs(dst_s.data_ptr(), [i * cap for i in range(n)])
        s_sz, d_cap, got = sizes([size] * n), sizes([cap] * n), (ctypes.c_size_t * n)()
        sync = best_of(lambda: ok(lib.ZSTDMI_compressBatch(cs, s_ptr, s_sz, n, d_ptr, d_cap, got)))
        assert lib.ZSTDMI_debugLastBatchAlone(cs) == 0
        lib.ZSTD_freeCCtx(cs)
        for per_call, k in ((n, 1), (256, 1), (256, 4)):
            dst_a = torch.zeros(n * cap + MiB, dtype=torch.uint8, device="cuda")
            c = lib.ZSTD_createCCtx()
            lib.ZSTD_CCtx_setParameter(c, 100, level)
            lim = z._ffi.CBatchLimits(per_call, size * k, 0)
            ok(lib.ZSTDMI_CCtx_prepareBatchAsyncLimits(c, ctypes.byref(lim)))
            cb, fb, mc = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
            ok(lib.ZSTDMI_CCtx_getBatchAsyncPlan(c, ctypes.byref(cb), ctypes.byref(fb), ctypes.byref(mc)))
            ok(lib.ZSTDMI_CCtx_setStream(c, torch.cuda.current_stream().cuda_stream or 1))
            srcs, dsts = src.data_ptr() + idx * size, dst_a.data_ptr() + idx * cap
            szs, caps = torch.full((n,), size, dtype=torch.int64, device="cuda"), torch.full((n,), cap, dtype=torch.int64, device="cuda")
            out = torch.empty(n, dtype=torch.int64, device="cuda")
            returned = [0.0]

            def enqueue():
                t0 = time.perf_counter()
                for at in range(0, n, per_call):
                    m = min(per_call, n - at)
                    ok(lib.ZSTDMI_compressBatchAsync(c, srcs.data_ptr() + 8 * at, szs.data_ptr() + 8 * at, m, dsts.data_ptr() + 8 * at, caps.data_ptr() + 8 * at, out.data_ptr() + 8 * at))
                returned[0] = time.perf_counter() - t0
                torch.cuda.synchronize()

            waits = lib.ZSTDMI_debugHostWaits(c)
            ret, done = 1e9, 1e9
            enqueue()
            for _ in range(3):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                enqueue()
                done = min(done, time.perf_counter() - t0); ret = min(ret, returned[0])
            assert lib.ZSTDMI_debugHostWaits(c) == waits
            sizes_a = out.cpu().tolist()
            assert all(0 < s <= cap for s in sizes_a)
            if k == 1:
                assert sizes_a == list(got) and bool(torch.equal(dst_a, dst_s))
            gbs = lambda t: total / t / 1e9
            filled = -(-size // cb.value)
            print(f"| text 256 KiB L{level} | {n:5d} | {per_call:4d} per call, bound {size * k // 1024:4d} KiB: {mc.value} slots of {cb.value} B per call, {per_call * filled} filled | ratio {sum(sizes_a) / total:.3f} "
                  f"| (a) async calls returned {ret * 1e3:7.2f} | (b) ... and the stream drained {done * 1e3:7.2f} ({gbs(done):6.1f}) | (c) synchronous batch {sync * 1e3:7.2f} ({gbs(sync):6.1f}), ratio {sum(got) / total:.3f} |", flush=True)
            lib.ZSTD_freeCCtx(c)
            del dst_a
            torch.cuda.empty_cache()
        del dst_s
        torch.cuda.empty_cache()


if "--async" in FLAGS:
    async_rows()
    async_frames_rows()
    sys.exit(0)
if DICT_INDEX_ROWS:
    dict_index_rows()
    sys.exit(0)
if UNSIZED_ROWS:
    unsized_rows()
    sys.exit(0)
data = {k: torch.from_numpy(np.frombuffer(datagen.gen(k, 16 * MiB, 5), dtype=np.uint8).copy()).cuda().repeat(total // (16 * MiB)) for k in ("text", "zipf")}
points = [(kind, size, level, None) for size in (4096, 16384, 65536) for kind in ("text", "zipf") for level in (1, 3)] + [("text", 4096, 3, DICT)]
frames_points = [(kind, size, level, None) for size in (256 << 10, 1 << 20) for kind in ("text", "zipf") for level in (1, 3)]
points = points[-1:] if DICT_ROW else frames_points if FRAMES_ROWS else points + frames_points
print(f"{total // MiB} MiB per point; ms per call of all entries (GB/s of content)", flush=True)
for kind, size, level, dic in points:
    src = data[kind]
    n = total // size
    cap = lib.ZSTD_compressBound(size)
    dst = torch.empty(n * cap + total // 64 + MiB, dtype=torch.uint8, device="cuda")
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    c, d = lib.ZSTD_createCCtx(), lib.ZSTD_createDCtx()
    lib.ZSTD_CCtx_setParameter(c, 100, level)
    if dic:
        ok(lib.ZSTD_CCtx_loadDictionary(c, dic, len(dic))); ok(lib.ZSTD_DCtx_loadDictionary(d, dic, len(dic)))
        if DICT_ENTROPY:
            ok(lib.ZSTDMI_CCtx_setDictEntropy(c, 1))
    s_ptr, d_ptr, o_ptr = ptrs(src.data_ptr(), [i * size for i in range(n)]), ptrs(dst.data_ptr(), [i * cap for i in range(n)]), ptrs(out.data_ptr(), [i * size for i in range(n)])
    s_sz, d_cap, got, back = sizes([size] * n), sizes([cap] * n), (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    # (b) batch
    lib.ZSTDMI_CCtx_setProfiling(c, 1); lib.ZSTDMI_DCtx_setProfiling(d, 1)
    cb = best_of(lambda: ok(lib.ZSTDMI_compressBatch(c, s_ptr, s_sz, n, d_ptr, d_cap, got)))
    alone = lib.ZSTDMI_debugLastBatchAlone(c)
    assert not any(lib.ZSTD_isError(g) for g in got) and (alone == 0 or MEASURE_ONLY)
    cst = stage_times(lib.ZSTDMI_CCtx_getStageTimes, c)
    db = best_of(lambda: ok(lib.ZSTDMI_decompressBatch(d, d_ptr, got, n, o_ptr, s_sz, back)))
    assert all(b == size for b in back) and lib.ZSTDMI_debugLastBatchAloneD(d) == 0 and bool(torch.equal(out, src))
    dst_t = stage_times(lib.ZSTDMI_DCtx_getStageTimes, d)
    lib.ZSTDMI_CCtx_setProfiling(c, 0); lib.ZSTDMI_DCtx_setProfiling(d, 0)
    comp_bytes = sum(got)
    # (a) the loop of single calls, on a sample
    m = min(n, SAMPLE)

    def loop_c():
        for i in range(m):
            lib.ZSTDMI_compressDevice(c, d_ptr[i], cap, s_ptr[i], size)

    def loop_d():
        for i in range(m):
            lib.ZSTDMI_decompressDevice(d, o_ptr[i], size, d_ptr[i], got[i])

    ca = best_of(loop_c, 3) * n / m
    da = best_of(loop_d, 3) * n / m
    # (c) one call on the concatenation (without the dictionary's small-input framing it is simply another stream)
    whole = [0]

    def concat_c():
        whole[0] = ok(lib.ZSTDMI_compressDevice(c, dst.data_ptr(), dst.numel(), src.data_ptr(), total))

    cc = best_of(concat_c)
    dc = best_of(lambda: ok(lib.ZSTDMI_decompressDevice(d, out.data_ptr(), total, dst.data_ptr(), whole[0])))
    gbs = lambda t: total / t / 1e9
    name = f"{kind} {size // 1024:2d} KiB L{level}{' dict' if dic else ''}{'+entropy' if dic and DICT_ENTROPY else ''}"
    print(f"| {name:22s} | {n:6d} | {comp_bytes / total:.3f} | {ca * 1e3:8.1f} ({gbs(ca):6.2f}) | {cb * 1e3:7.2f} ({gbs(cb):6.1f}) | {cc * 1e3:7.2f} ({gbs(cc):6.1f}) "
          f"| {da * 1e3:8.1f} ({gbs(da):6.2f}) | {db * 1e3:7.2f} ({gbs(db):6.1f}) | {dc * 1e3:7.2f} ({gbs(dc):6.1f}) |", flush=True)
    print(f"    compress stages ms: {cst}\n    decompress stages ms: {dst_t}", flush=True)
    if MEASURE_ONLY:
        print(f"    entries compressed alone: {alone} of {n}", flush=True)
    assert MEASURE_ONLY or (cb < ca and db < da), "the batch call must beat the loop of single calls"
    lib.ZSTD_freeCCtx(c); lib.ZSTD_freeDCtx(d)
    del dst, out
    torch.cuda.empty_cache()
