"""GPU dictionary training (ZDICT_trainFromBuffer / the fastCover entry points, dict_train.hip).  The dictionary content for given
parameters must equal libzstd's byte for byte (tests/golden/manifest_train.json, made by make_golden_train.py); the whole
dictionary must load and round-trip in the GPU decoder and the oracle's; training must be deterministic across threads."""
import ctypes
import json
import os
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_golden_train as mgt          # noqa: E402
import oracle_lib                        # noqa: E402
import zstdsharp_amd as z                # noqa: E402
from zstdsharp_amd import _ffi           # noqa: E402

pytestmark = pytest.mark.gpu
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_train.json")))["cases"]


def _buffers(recs):
    flat = b"".join(recs)
    return ctypes.create_string_buffer(flat, max(len(flat), 1)), (ctypes.c_size_t * len(recs))(*[len(r) for r in recs])


def train_fixed(recs, cap, k, d, f=0, accel=0):
    lib = _ffi.load()
    src, sizes = _buffers(recs)
    p = _ffi.ZDICT_fastCover_params_t(); p.k = k; p.d = d; p.f = f; p.accel = accel
    dst = ctypes.create_string_buffer(cap)
    n = lib.ZDICT_trainFromBuffer_fastCover(dst, cap, src, sizes, len(recs), p)
    assert not lib.ZDICT_isError(n), lib.ZDICT_getErrorName(n)
    return dst.raw[:n]


def train_optimize(recs, cap):
    lib = _ffi.load()
    src, sizes = _buffers(recs)
    p = _ffi.ZDICT_fastCover_params_t(); p.d = 8; p.steps = 4; p.zParams.compressionLevel = 3
    dst = ctypes.create_string_buffer(cap)
    n = lib.ZDICT_optimizeTrainFromBuffer_fastCover(dst, cap, src, sizes, len(recs), ctypes.byref(p))
    assert not lib.ZDICT_isError(n), lib.ZDICT_getErrorName(n)
    return dst.raw[:n], p


def _ncount_size(b: bytes, pos: int, max_sv: int) -> int:
    """bytes of one FSE table description starting at b[pos] (FSE_readNCount, RFC 8878 4.1.1)"""
    bit = pos * 8
    def read(n):
        nonlocal bit
        v = (int.from_bytes(b[bit // 8:bit // 8 + 8].ljust(8, b"\0"), "little") >> (bit % 8)) & ((1 << n) - 1)
        return v
    acc = read(4) + 5; bit += 4
    remaining, sym, prev0 = (1 << acc) + 1, 0, False
    while remaining > 1 and sym <= max_sv:
        if prev0:
            while True:
                rep = read(2); bit += 2; sym += rep
                if rep != 3:
                    break
            prev0 = False
            continue
        nb = remaining.bit_length()                      # bits of the largest value still possible
        max_v = (1 << nb) - 1 - remaining
        low = read(nb - 1)
        if low < max_v:
            val = low; bit += nb - 1
        else:
            val = read(nb); bit += nb
            if val >= (1 << (nb - 1)):
                val -= max_v
        proba = val - 1
        remaining -= -proba if proba < 0 else proba
        prev0 = proba == 0
        sym += 1
    return (bit + 7) // 8 - pos


def header_size(d: bytes) -> int:
    """a formatted dictionary's header: magic, dictID, the Huffman table description, three FSE descriptions, repcodes"""
    hb = d[8]
    pos = 8 + (1 + hb if hb < 128 else 1 + (hb - 127 + 1) // 2)
    for max_sv in (31, 52, 35):
        pos += _ncount_size(d, pos, max_sv)
    return pos + 12


@pytest.mark.parametrize("case", [c for c in MANIFEST if c["fixed"]], ids=lambda c: c["name"])
def test_fixed_k_content_equals_libzstd(case):
    recs = mgt.samples(case["recipe"])
    ours = train_fixed(recs, case["cap"], case["k"], case["d"], case["f"], case["accel"])
    ref = open(os.path.join(GOLDEN, case["file"]), "rb").read()
    assert len(ref) == case["size"]
    ours_c, ref_c = ours[header_size(ours):], ref[case["header_size"]:]
    assert len(ours) <= case["cap"]
    if len(ours_c) == len(ref_c):
        assert ours_c == ref_c
    else:            # one side truncated its content at the end to fit its header: the shorter one is a prefix
        short, long_ = sorted([ours_c, ref_c], key=len)
        assert long_.startswith(short)
    if case["name"].endswith("_small"):          # the content does not fill the capacity: nothing truncated on either side
        assert ours_c == ref_c
    assert int.from_bytes(ours[:4], "little") == 0xEC30A437
    dict_id = int.from_bytes(ours[4:8], "little")
    assert 32768 <= dict_id < (1 << 31)
    if case["name"].endswith("_small"):          # the ID hashes the content before truncation: checkable where there is none
        assert dict_id == oracle_dict_id(ours_c) == int.from_bytes(ref[4:8], "little")


def oracle_dict_id(content: bytes) -> int:
    """ZDICT_finalizeDictionary's compliant ID: XXH64(content, 0) % ((1 << 31) - 32768) + 32768"""
    return _xxh64(content) % ((1 << 31) - 32768) + 32768


def _xxh64(data: bytes, seed: int = 0) -> int:
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M
    def rnd(acc, v):
        return (rotl((acc + v * P2) & M, 31) * P1) & M
    n, i = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        while i + 32 <= n:
            for j in range(4):
                v[j] = rnd(v[j], int.from_bytes(data[i + 8 * j:i + 8 * j + 8], "little"))
            i += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for j in range(4):
            h = ((h ^ rnd(0, v[j])) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while i + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[i:i + 8], "little")), 27) * P1 + P4) & M; i += 8
    if i + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * P1 & M), 23) * P2 + P3) & M; i += 4
    while i < n:
        h = (rotl(h ^ (data[i] * P5 & M), 11) * P1) & M; i += 1
    h ^= h >> 33; h = h * P2 & M; h ^= h >> 29; h = h * P3 & M; h ^= h >> 32
    return h


def _held_out(case, seed_shift=1000):
    r = dict(case["recipe"]); r["seed"] = r["seed"] + seed_shift; r["count"] = 200
    return mgt.samples(r)


def _total(recs, dict_bytes):
    with z.Compressor(3) as c:
        if dict_bytes:
            c.LoadDictionary(dict_bytes)
        return sum(len(c.Wrap(r)) for r in recs)


@pytest.mark.parametrize("name", ["default_text", "default_zipf"])
def test_default_training_valid_and_round_trips(name):
    case = next(c for c in MANIFEST if c["name"] == name)
    recs = mgt.samples(case["recipe"])
    dic = z.DictBuilder.train_from_buffer(recs)
    assert 256 <= len(dic) <= 112640
    assert int.from_bytes(dic[:4], "little") == 0xEC30A437
    held = _held_out(case)
    with z.Compressor(3) as c, z.Decompressor() as d:
        c.LoadDictionary(dic); d.LoadDictionary(dic)
        for r in held[:60]:
            comp = c.Wrap(r)
            assert d.Unwrap(comp) == r
            assert oracle_lib.decompress(comp, len(r), dic) == r
    # the content is the fixed-k content of the k the optimizer reports
    best, p = train_optimize(recs, 112640)
    assert best == dic
    assert p.d == 8 and p.k in (50, 537, 1024, 1511, 1998)
    fixed = train_fixed(recs[:int(len(recs) * 0.75)], 112640, p.k, 8)
    # (fixed-k training uses every sample it is given; the optimizer trained on the first 75 %)
    assert dic[header_size(dic):] == fixed[header_size(fixed):]


@pytest.mark.parametrize("name", ["default_json", "default_text", "default_zipf"])
def test_ratio_against_libzstd_dictionary(name):
    case = next(c for c in MANIFEST if c["name"] == name)
    recs = mgt.samples(case["recipe"])
    ours = z.DictBuilder.train_from_buffer(recs)
    ref = open(os.path.join(GOLDEN, case["file"]), "rb").read()
    held = _held_out(case)
    t_ours, t_ref, t_none = _total(held, ours), _total(held, ref), _total(held, None)
    print(f"{name}: ours {t_ours} libzstd-dict {t_ref} none {t_none} -> {t_ours / t_ref:.4f}, {t_ours / t_none:.4f}")
    assert t_ours <= 1.03 * t_ref
    if name == "default_json":       # structured records: a dictionary must clearly pay off
        assert t_ours < 0.6 * t_none
    else:                            # these datagen records gain little from any dictionary, libzstd's included
        assert t_ours <= 1.03 * t_none


def test_build_dictionary_case():
    case = next(c for c in MANIFEST if c["name"] == "build_dictionary")
    recs = mgt.samples(case["recipe"])
    dic = z.DictBuilder.train_from_buffer(recs, 1024)
    assert 0 < len(dic) <= 1024
    with z.Compressor(3) as c, z.Decompressor() as d:
        c.LoadDictionary(dic); d.LoadDictionary(dic)
        assert d.Unwrap(c.Wrap(recs[0])) == recs[0]


def test_parallel_training_is_deterministic():
    case = next(c for c in MANIFEST if c["name"] == "default_text")
    recs = mgt.samples(dict(case["recipe"], count=300))
    out, errs = [], []

    def work():
        try:
            for _ in range(2):
                out.append(z.DictBuilder.train_from_buffer(recs, 16384))
        except Exception as e:           # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work) for _ in range(8)]
    [t.start() for t in th]; [t.join() for t in th]
    assert not errs
    assert len(out) == 16 and all(o == out[0] for o in out)


def test_train_dictionary_parallel_sample_set():
    # T/ZstdNetTests.cs:587-605: bytes (i * i) & 0xFF, 100 samples of 200 - i bytes from offset i
    buf = bytes((i * i) & 0xFF for i in range(100000))
    recs = [buf[i:i + 200 - i] for i in range(100)]
    first = z.DictBuilder.train_from_buffer(recs)
    assert 0 < len(first) <= 112640
    out = []
    th = [threading.Thread(target=lambda: out.append(z.DictBuilder.train_from_buffer(recs))) for _ in range(8)]
    [t.start() for t in th]; [t.join() for t in th]
    assert len(out) == 8 and all(o == first for o in out)


def test_mirror_round_trip_and_dst_size_too_small():
    case = next(c for c in MANIFEST if c["name"] == "default_text")
    recs = mgt.samples(dict(case["recipe"], count=400))
    dic = z.DictBuilder.TrainFromBuffer(recs, 8192)
    data = b"".join(_held_out(case)[:5])
    with z.Compressor(3) as c, z.Decompressor() as d:
        c.LoadDictionary(dic); d.LoadDictionary(dic)
        assert d.Unwrap(c.Wrap(data)) == data
    with pytest.raises(z.ZstdException) as e:
        z.DictBuilder.train_from_buffer(recs, 255)
    assert e.value.Code == z.ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall


def test_batch_hook_matches_compress2_per_sample():
    """ZSTDMI_debugCompressSamples: one batch, each sample sized as ZSTD_compress2 of it alone (1 B to 150 KiB: several dictionary
    prefix classes, multi-chunk samples), with a formatted dictionary and with a raw-content one"""
    import numpy as np
    lib = _ffi.load()
    r = np.random.default_rng(5)
    base = b"".join(mgt.json_records(400, 9))
    lens = [1, 7, 8, 100, 1000, 4000, 20000, 30000, 40000, 65536, 100000, 150000] + [int(x) for x in r.integers(1, 70000, 24)]
    recs = [base[(o := int(r.integers(0, len(base) - n))):o + n] if n < len(base) else (base * 3)[:n] for n in lens]
    for dic in (open(os.path.join(GOLDEN, "train_default_json.dict"), "rb").read(), base[-50000:]):
        with z.Compressor(3) as c:
            c.LoadDictionary(dic)
            alone = [len(c.Wrap(x)) for x in recs]
            src, sizes = _buffers(recs)
            out = (ctypes.c_size_t * len(recs))()
            assert lib.ZSTDMI_debugCompressSamples(c.cctx, src, sizes, len(recs), out) == 0
            assert list(out) == alone
