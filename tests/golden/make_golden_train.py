"""Generates the dictionary-training fixtures (tests/golden/train_*.dict + manifest_train.json): what libzstd's fastCover trainer
returns for sample sets that the tests rebuild from a recipe (datagen kind, seed, record sizes).  Run ONCE in the authoring
container (needs the third-party libzstd 1.5.7 shared object bundled with Pillow there, as make_golden_dict.py); outputs are
committed, tests only read them.  libzstd stands in for the reference's U/Fastcover.cs, as it does for frames (T/ZstdTest.cs)."""
import ctypes, glob, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import datagen

sz, vp, ci, cu = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint


class ZDICT_params_t(ctypes.Structure):
    _fields_ = [("compressionLevel", ci), ("notificationLevel", cu), ("dictID", cu)]


class ZDICT_fastCover_params_t(ctypes.Structure):
    _fields_ = [("k", cu), ("d", cu), ("f", cu), ("steps", cu), ("nbThreads", cu), ("splitPoint", ctypes.c_double),
                ("accel", cu), ("shrinkDict", cu), ("shrinkDictMaxRegression", cu), ("zParams", ZDICT_params_t)]


def record_sizes(recipe):
    """sizes cycle through recipe['sizes'] until `count` records"""
    s = recipe["sizes"]
    return [s[i % len(s)] for i in range(recipe["count"])]


def json_records(count, seed):
    """structured records: JSON objects with shared field names and value templates (what dictionaries are made for)"""
    import numpy as np
    r = np.random.default_rng(seed)
    cities = ["Amsterdam", "Berlin", "Chicago", "Denver", "Edinburgh", "Florence", "Geneva", "Houston"]
    status = ["active", "suspended", "pending_review", "closed"]
    out = []
    for i in range(count):
        n = int(r.integers(1, 4))
        items = ",".join('{"sku":"SKU-%06d","qty":%d,"price":%d.%02d}' % (int(r.integers(0, 10 ** 6)), int(r.integers(1, 9)),
                                                                           int(r.integers(1, 500)), int(r.integers(0, 100))) for _ in range(n))
        out.append(('{"id":%d,"user":{"name":"user_%05d","email":"user_%05d@example.com","city":"%s"},"status":"%s",'
                    '"created_at":"2024-%02d-%02dT%02d:%02d:%02dZ","items":[%s],"tags":["customer","tier-%d"]}'
                    % (100000 + i, int(r.integers(0, 10 ** 5)), int(r.integers(0, 10 ** 5)), cities[int(r.integers(0, 8))],
                       status[int(r.integers(0, 4))], int(r.integers(1, 13)), int(r.integers(1, 29)), int(r.integers(0, 24)),
                       int(r.integers(0, 60)), int(r.integers(0, 60)), items, int(r.integers(1, 4)))).encode())
    return out


def samples(recipe):
    """-> list of records: consecutive slices of one datagen stream (a shared vocabulary: what dictionaries are for);
    kind 'same' = `count` copies of one datagen record; kind 'json' = structured records (json_records)"""
    if recipe["kind"] == "json":
        return json_records(recipe["count"], recipe["seed"])
    sizes = record_sizes(recipe)
    if recipe["kind"] == "same":
        one = datagen.gen("text", sizes[0], recipe["seed"])
        return [one] * len(sizes)
    data = datagen.gen(recipe["kind"], sum(sizes), recipe["seed"])
    out, pos = [], 0
    for n in sizes:
        out.append(data[pos:pos + n]); pos += n
    return out


# fixed-parameter cases: ZDICT_trainFromBuffer_fastCover
FIXED = [
    dict(name="d8_f20_a1_k50_4k", recipe=dict(kind="text", seed=11, sizes=[120, 260, 380, 90], count=400), cap=4096, k=50, d=8, f=20, accel=1),
    dict(name="d8_f20_a1_k1998_16k", recipe=dict(kind="text", seed=12, sizes=[300, 700, 150], count=300), cap=16384, k=1998, d=8, f=20, accel=1),
    dict(name="d6_f20_a1_k537_8k", recipe=dict(kind="text", seed=13, sizes=[200, 450], count=300), cap=8192, k=537, d=6, f=20, accel=1),
    dict(name="d8_f16_a1_k1024_8k", recipe=dict(kind="zipf", seed=14, sizes=[256, 512, 100], count=240), cap=8192, k=1024, d=8, f=16, accel=1),
    dict(name="d8_f20_a4_k537_8k", recipe=dict(kind="text", seed=15, sizes=[333, 222], count=300), cap=8192, k=537, d=8, f=20, accel=4),
    dict(name="d6_f18_a2_k50_2k", recipe=dict(kind="text", seed=16, sizes=[64, 96, 150], count=200), cap=2048, k=50, d=6, f=18, accel=2),
    # the content does not fill the capacity: no truncation on either side
    dict(name="d8_f20_a1_k1998_32k_small", recipe=dict(kind="text", seed=17, sizes=[100], count=20), cap=32768, k=1998, d=8, f=20, accel=1),
    dict(name="d8_f20_a1_k50_32k_small", recipe=dict(kind="text", seed=18, sizes=[90, 40], count=30), cap=32768, k=50, d=8, f=20, accel=1),
]
# ZDICT_trainFromBuffer at the default capacity (ratio and validity tests) and the degenerate inputs (error codes)
DEFAULT = [
    dict(name="default_text", recipe=dict(kind="text", seed=21, sizes=[180, 420, 260, 900, 140], count=1200), cap=112640),
    dict(name="default_zipf", recipe=dict(kind="zipf", seed=22, sizes=[300, 700, 500], count=900), cap=112640),
    dict(name="default_json", recipe=dict(kind="json", seed=26, sizes=[0], count=3000), cap=112640),
    dict(name="build_dictionary", recipe=dict(kind="same", seed=1234, sizes=[100], count=8), cap=1024),
    dict(name="too_few_samples", recipe=dict(kind="text", seed=23, sizes=[500], count=4), cap=4096),
    dict(name="total_under_8", recipe=dict(kind="text", seed=24, sizes=[1], count=6), cap=4096),
    dict(name="capacity_under_256", recipe=dict(kind="text", seed=25, sizes=[300], count=50), cap=200),
]


def load():
    path = glob.glob("/usr/local/lib/python3*/dist-packages/pillow.libs/libzstd*")[0]
    l = ctypes.CDLL(path)
    l.ZSTD_versionNumber.restype = cu
    l.ZDICT_trainFromBuffer.restype = sz; l.ZDICT_trainFromBuffer.argtypes = [vp, sz, vp, ctypes.POINTER(sz), cu]
    l.ZDICT_trainFromBuffer_fastCover.restype = sz
    l.ZDICT_trainFromBuffer_fastCover.argtypes = [vp, sz, vp, ctypes.POINTER(sz), cu, ZDICT_fastCover_params_t]
    l.ZDICT_isError.restype = cu; l.ZDICT_isError.argtypes = [sz]
    l.ZDICT_getDictHeaderSize.restype = sz; l.ZDICT_getDictHeaderSize.argtypes = [vp, sz]
    return l


def run(l, case, fixed):
    recs = samples(case["recipe"])
    flat = b"".join(recs)
    sizes = (sz * len(recs))(*[len(r) for r in recs])
    src = ctypes.create_string_buffer(flat, max(len(flat), 1))
    dst = ctypes.create_string_buffer(case["cap"])
    if fixed:
        p = ZDICT_fastCover_params_t(); p.k = case["k"]; p.d = case["d"]; p.f = case["f"]; p.accel = case["accel"]
        r = l.ZDICT_trainFromBuffer_fastCover(dst, case["cap"], src, sizes, len(recs), p)
    else:
        r = l.ZDICT_trainFromBuffer(dst, case["cap"], src, sizes, len(recs))
    entry = dict(case, fixed=fixed, libzstd=l.ZSTD_versionNumber())
    if l.ZDICT_isError(r):
        entry["error"] = (1 << 64) - r
        return entry
    d = dst.raw[:r]
    entry.update(size=r, header_size=l.ZDICT_getDictHeaderSize(dst, r), file=f"train_{case['name']}.dict")
    with open(os.path.join(HERE, entry["file"]), "wb") as fh:
        fh.write(d)
    return entry


def main():
    l = load()
    cases = [run(l, c, True) for c in FIXED] + [run(l, c, False) for c in DEFAULT]
    with open(os.path.join(HERE, "manifest_train.json"), "w") as fh:
        json.dump({"generator": "tests/golden/make_golden_train.py", "cases": cases}, fh, indent=1)
    for c in cases:
        print(c["name"], c.get("size"), c.get("header_size"), c.get("error"))


if __name__ == "__main__":
    main()
