"""ZSTDMI_compressPack against what a caller has to do without it (run on the GPU box): 256 MiB of device-resident entries per row —
text entries of 4 KiB (65 536) and 64 KiB (4096) at levels 1 and 3, of 1 MiB (256) at level 3, and the 1000 held-out JSON records of
tests/golden/make_golden_train.py tiled to the total with train_default_json.dict at level 1, ZSTDMI_CCtx_setDictIndex on.  Per row:
  (a) pack   : one ZSTDMI_compressPack call into ZSTDMI_packBound bytes
  (b) batch+ : the same entries through ZSTDMI_compressBatch into ZSTD_compressBound-sized slots, PLUS what gives the same bytes today:
               one device-side concatenation of the pieces (a byte gather through an index made with torch from the sizes), and a
               table built on the host and uploaded behind them.  The table's rows are taken from (a)'s table: the walk over the
               pieces a caller needs to learn the frame sizes of entries of several frames is NOT charged.
  (c) the pack call's stage times (ZSTDMI_CCtx_getStageTimes) and the share of the new stages (pack_*) in their sum
  (d) read   : 4096 random records read back with one ZSTDMI_decompressRanges call
Best of 3 after a warm-up call of the same shape; the host clock stops after the final synchronise.  Every pack is compared with (b)'s
stream byte for byte and decoded back to the input.  The text is 16 MiB of generated data repeated (entries are independent).
python tools/pack_time.py [MiB] [--json-only] [--sorted] [--async]
  --json-only : the JSON row alone
  --sorted    : the JSON row with its records ordered by size, every record repeated in place instead of the list being tiled: a round
                then holds one class of resolved parameters, as a pass of the batch does (which sorts the whole call by class)
  --async     : ZSTDMI_compressPackAsync instead (README "Packs enqueued from the device"): text entries of 4 KiB in packs of 16 384 and
                of 256 KiB in packs of 1024, levels 1 and 3, every pack a stream of its own behind one prepare.  Per row, best of 3
                after a warm-up: (a) the time until the async calls have returned, (b) until the stream has drained, (c)
                ZSTDMI_compressPack of the same entries on a second context of the same build, all three repetitions shown.  The
                streams are compared byte for byte afterwards (every entry is in the bound's tier)."""
import ctypes, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, GOLDEN)
import numpy as np, torch
torch.zeros(1, device="cuda")
import zstdsharp_amd as z, datagen
import make_golden_train as mgt
lib = z._ffi.load()
MiB = 1 << 20
FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
assert all(f in ("--json-only", "--sorted", "--async") for f in FLAGS), FLAGS
total = (int(ARGS[0]) if ARGS else 256) * MiB


def stage_times(ctx):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = lib.ZSTDMI_CCtx_getStageTimes(ctx, ms, names, 24)
    return [(names[i].decode(), float(ms[i])) for i in range(k)]


def best_of(f, reps=3):
    f()                                     # warm-up: same shape, workspaces allocated
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def ok(r):
    assert not lib.ZSTD_isError(r), lib.ZSTD_getErrorName(r)
    return r


def arr(kind, vals):
    a = np.ascontiguousarray(vals, dtype=np.uint64)
    return (kind * len(a)).from_buffer_copy(a.tobytes())


def rows():
    text = datagen.gen("text", 16 * MiB, 5) * (total // (16 * MiB))
    for size, levels in () if "--json-only" in FLAGS else ((4096, (1, 3)), (65536, (1, 3)), (MiB, (3,))):
        for level in levels:
            yield f"text {size // 1024:4d} KiB L{level}", text, [size] * (total // size), level, None
    recs = mgt.json_records(2000, 77)[1000:]
    blob = b"".join(recs)
    reps = total // len(blob)
    if "--sorted" in FLAGS:
        recs = sorted(recs, key=len)
        yield "json sorted L1 dict+index", b"".join(r * reps for r in recs), [len(r) for r in recs for _ in range(reps)], 1, open(os.path.join(GOLDEN, "train_default_json.dict"), "rb").read()
        return
    yield "json records L1 dict+index", blob * reps, [len(r) for r in recs] * reps, 1, open(os.path.join(GOLDEN, "train_default_json.dict"), "rb").read()


def async_rows():
    text = datagen.gen("text", 16 * MiB, 5) * (total // (16 * MiB))
    src = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    print(f"{total // MiB} MiB per row; ms (GB/s of content); (c) = ZSTDMI_compressPack, the yardstick", flush=True)
    for size, per_pack in ((4096, 16384), (256 * 1024, 1024)):
        for level in (1, 3):
            n = total // size
            packs = [(i, min(per_pack, n - i)) for i in range(0, n, per_pack)]
            offs = np.arange(n, dtype=np.uint64) * np.uint64(size)
            ptrs_np, szs_np = offs + np.uint64(src.data_ptr()), np.full(n, size, dtype=np.uint64)
            d_ptrs, d_szs = torch.from_numpy(ptrs_np.astype(np.int64)).cuda(), torch.from_numpy(szs_np.astype(np.int64)).cuda()
            with z.Compressor(level) as c, z.Compressor(level) as ref:
                if size <= 65536:
                    c.PrepareBatchAsync(per_pack, size)
                else:
                    c.PrepareBatchAsyncLimits(per_pack, size)
                room = c.pack_async_bound(per_pack)
                dsts = [torch.empty(room, dtype=torch.uint8, device="cuda") for _ in packs]
                outs = [torch.empty(1, dtype=torch.int64, device="cuda") for _ in packs]
                want = [torch.empty(room, dtype=torch.uint8, device="cuda") for _ in packs]
                h_ptr, h_sz = arr(ctypes.c_void_p, ptrs_np), arr(ctypes.c_size_t, szs_np)
                step = ctypes.sizeof(ctypes.c_size_t)

                def run_async():
                    for (i, k), dst, out in zip(packs, dsts, outs):
                        z.batch.compress_pack_async(c, d_ptrs[i:i + k], d_szs[i:i + k], dst, out_size=out)

                run_async(); torch.cuda.synchronize()           # warm-up
                ta = tb = 1e9
                for _ in range(3):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    run_async()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    ta, tb = min(ta, t1 - t0), min(tb, time.perf_counter() - t0)
                got = [int(o.item()) for o in outs]
                assert all(g > 0 for g in got), got
                sync_size = [0] * len(packs)

                def run_sync():
                    for j, (i, k) in enumerate(packs):
                        sync_size[j] = ok(lib.ZSTDMI_compressPack(ref.cctx, want[j].data_ptr(), room, ctypes.cast(ctypes.addressof(h_ptr) + i * step, ctypes.POINTER(ctypes.c_void_p)),
                                                                 ctypes.cast(ctypes.addressof(h_sz) + i * step, ctypes.POINTER(ctypes.c_size_t)), k))

                run_sync()
                tc = []
                for _ in range(3):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    run_sync()
                    torch.cuda.synchronize()
                    tc.append(time.perf_counter() - t0)
                same = all(g == w and bool(torch.equal(d[:g], x[:w])) for g, w, d, x in zip(got, sync_size, dsts, want))
                gbs = lambda t: total / t / 1e9
                print(f"| text {size // 1024:4d} KiB L{level} | {n:6d} entries in {len(packs)} packs | ratio {sum(got) / total:.4f} | (a) returned {ta * 1e3:7.2f} | "
                      f"(b) drained {tb * 1e3:8.2f} ({gbs(tb):5.1f}) | (c) {min(tc) * 1e3:8.2f} ({gbs(min(tc)):5.1f}) of {' '.join(f'{t * 1e3:.2f}' for t in tc)} | "
                      f"bytes {'equal' if same else 'DIFFER'} |", flush=True)
                assert same, "the async pack's streams are not ZSTDMI_compressPack's"
            del dsts, want
            torch.cuda.empty_cache()


if "--async" in FLAGS:
    async_rows()
    sys.exit(0)
print(f"{total // MiB} MiB per row; ms per call (GB/s of content)", flush=True)
for name, blob, szs, level, dic in rows():
    content = len(blob)
    src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    n = len(szs)
    szs_np = np.asarray(szs, dtype=np.uint64)
    offs = np.concatenate(([0], np.cumsum(szs_np)[:-1])).astype(np.uint64)
    caps_np = np.asarray([lib.ZSTD_compressBound(int(x)) for x in np.unique(szs_np)], dtype=np.uint64)[np.searchsorted(np.unique(szs_np), szs_np)]
    coffs = np.concatenate(([0], np.cumsum(caps_np)[:-1])).astype(np.uint64)
    s_sz, s_ptr = arr(ctypes.c_size_t, szs_np), arr(ctypes.c_void_p, offs + np.uint64(src.data_ptr()))
    bound = ok(lib.ZSTDMI_packBound(s_sz, n))
    packed = torch.empty(bound, dtype=torch.uint8, device="cuda")
    slots = torch.empty(int(caps_np.sum()) + 64, dtype=torch.uint8, device="cuda")
    d_ptr, d_cap, got = arr(ctypes.c_void_p, coffs + np.uint64(slots.data_ptr())), arr(ctypes.c_size_t, caps_np), (ctypes.c_size_t * n)()
    c, d = lib.ZSTD_createCCtx(), lib.ZSTD_createDCtx()
    lib.ZSTD_CCtx_setParameter(c, 100, level)
    if dic:
        ok(lib.ZSTDMI_CCtx_setDictIndex(c, 1)); ok(lib.ZSTD_CCtx_loadDictionary(c, dic, len(dic))); ok(lib.ZSTD_DCtx_loadDictionary(d, dic, len(dic)))
    # (a) the pack
    size = [0]

    def pack():
        size[0] = ok(lib.ZSTDMI_compressPack(c, packed.data_ptr(), bound, s_ptr, s_sz, n))

    ta = best_of(pack)
    lib.ZSTDMI_CCtx_setProfiling(c, 1)      # (the stage times: a call of their own, after the timed ones)
    pack()
    st = stage_times(c)
    lib.ZSTDMI_CCtx_setProfiling(c, 0)
    alone, frames = lib.ZSTDMI_debugLastPackAlone(c), lib.ZSTDMI_debugLastPackFrames(c)
    table = packed[size[0] - (17 + 8 * frames):size[0]].cpu().numpy().tobytes()
    table_rows = np.frombuffer(table[8:-9], dtype=np.uint32).reshape(-1, 2)
    # (b) the batch, the concatenation, the table
    starts = torch.from_numpy(coffs.astype(np.int64)).cuda()
    whole = [None]

    def batch_plus():
        ok(lib.ZSTDMI_compressBatch(c, s_ptr, s_sz, n, d_ptr, d_cap, got))
        lens = torch.from_numpy(np.frombuffer(got, dtype=np.uint64).astype(np.int64)).cuda()
        ends = torch.cumsum(lens, 0)
        index = torch.repeat_interleave(starts - (ends - lens), lens) + torch.arange(int(ends[-1]), device="cuda")
        tab = np.empty(17 + 8 * len(table_rows), dtype=np.uint8)
        tab[:8] = np.frombuffer(np.array([0x184D2A5E, 9 + 8 * len(table_rows)], dtype=np.uint32).tobytes(), dtype=np.uint8)
        tab[8:-9] = np.frombuffer(table_rows.tobytes(), dtype=np.uint8)
        tab[-9:] = np.frombuffer(np.array([len(table_rows)], dtype=np.uint32).tobytes() + b"\0" + np.array([0x8F92EAB1], dtype=np.uint32).tobytes(), dtype=np.uint8)
        whole[0] = torch.cat([slots[index], torch.from_numpy(tab).cuda()])

    tb = best_of(batch_plus)
    tbatch = best_of(lambda: ok(lib.ZSTDMI_compressBatch(c, s_ptr, s_sz, n, d_ptr, d_cap, got)))
    assert whole[0].numel() == size[0] and bool(torch.equal(whole[0], packed[:size[0]])), "the pack is not the batch's pieces side by side"
    whole[0] = None
    out = torch.empty(content, dtype=torch.uint8, device="cuda")
    assert ok(lib.ZSTDMI_decompressDevice(d, out.data_ptr(), content, packed.data_ptr(), size[0])) == content and bool(torch.equal(out, src))
    # (d) 4096 random records
    pick = np.random.default_rng(1).choice(n, size=min(4096, n), replace=False)
    k = len(pick)
    r_off, r_len = arr(ctypes.c_ulonglong, offs[pick]), arr(ctypes.c_size_t, szs_np[pick])
    o_at = np.concatenate(([0], np.cumsum(szs_np[pick])[:-1])).astype(np.uint64)
    r_dst, r_got = arr(ctypes.c_void_p, o_at + np.uint64(out.data_ptr())), (ctypes.c_size_t * k)()
    tr = best_of(lambda: ok(lib.ZSTDMI_decompressRanges(d, packed.data_ptr(), size[0], r_off, r_len, k, r_dst, r_len, r_got)))
    assert list(r_got) == [int(x) for x in szs_np[pick]]
    for j in (0, k // 2, k - 1):
        a, b, m = int(o_at[j]), int(offs[pick[j]]), int(szs_np[pick[j]])
        assert bool(torch.equal(out[a:a + m], src[b:b + m]))
    gbs = lambda t: content / t / 1e9
    new = sum(ms for nm, ms in st if nm.startswith("pack_"))
    print(f"| {name:26s} | {n:7d} | ratio {size[0] / content:.4f} | frames {frames:7d} alone {alone} | pack {ta * 1e3:8.2f} ({gbs(ta):5.1f}) | "
          f"batch+concat+table {tb * 1e3:8.2f} ({gbs(tb):5.1f}), the batch call alone {tbatch * 1e3:8.2f} | {k} ranges {tr * 1e3:7.2f} |", flush=True)
    print(f"    pack stages ms: {' '.join(f'{nm} {ms:.2f}' for nm, ms in st)}\n    new stages (pack_*): {new:.2f} ms of {sum(ms for _, ms in st):.2f} ms on the device, "
          f"{100 * new / (ta * 1e3):.1f} % of the call", flush=True)
    lib.ZSTD_freeCCtx(c); lib.ZSTD_freeDCtx(d)
    del src, packed, slots, out, starts
    torch.cuda.empty_cache()
