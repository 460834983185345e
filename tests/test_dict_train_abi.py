"""Dictionary training ABI (ZDICT_trainFromBuffer and the fastCover entry points, include/zstd_mi355x.h), without a GPU: the
symbols are exported and agree with the header and _ffi.py, and the argument checks answer in the reference's order with the
error codes libzstd recorded (tests/golden/manifest_train.json) before any device is touched."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_train as mgt          # noqa: E402  (recipes only; libzstd is not loaded)
import zstdsharp_amd as z                # noqa: E402
from zstdsharp_amd import _ffi           # noqa: E402

NAMES = ["ZDICT_trainFromBuffer", "ZDICT_trainFromBuffer_fastCover", "ZDICT_optimizeTrainFromBuffer_fastCover",
         "ZDICT_finalizeDictionary"]
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest_train.json")))["cases"]


def test_symbols_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    for n in NAMES:
        assert re.search(rf"\bT {n}$", out, re.M), n
        assert re.search(rf"\b{n}\(", header), n
        assert n in _ffi.SIGNATURES, n
    for s in ["ZDICT_params_t", "ZDICT_cover_params_t", "ZDICT_fastCover_params_t"]:
        assert s in header


def test_param_struct_layouts():
    # U/ZDICT_fastCover_params_t.cs etc.: uint fields, a double, the nested ZDICT_params_t
    assert ctypes.sizeof(_ffi.ZDICT_params_t) == 12
    assert _ffi.ZDICT_fastCover_params_t.splitPoint.offset == 24
    assert _ffi.ZDICT_fastCover_params_t.zParams.offset == 44
    assert ctypes.sizeof(_ffi.ZDICT_fastCover_params_t) == 56
    assert _ffi.ZDICT_cover_params_t.splitPoint.offset == 16
    assert ctypes.sizeof(_ffi.ZDICT_cover_params_t) == 48


def _call_default(recs, cap):
    lib = _ffi.load()
    flat = b"".join(recs)
    sizes = (ctypes.c_size_t * max(len(recs), 1))(*[len(r) for r in recs])
    dst = ctypes.create_string_buffer(max(cap, 1))
    return lib.ZDICT_trainFromBuffer(dst, cap, ctypes.create_string_buffer(flat, max(len(flat), 1)), sizes, len(recs))


def _call_fixed(recs, cap, **kw):
    lib = _ffi.load()
    p = _ffi.ZDICT_fastCover_params_t()
    for k, v in kw.items():
        setattr(p, k, v)
    flat = b"".join(recs)
    sizes = (ctypes.c_size_t * max(len(recs), 1))(*[len(r) for r in recs])
    dst = ctypes.create_string_buffer(max(cap, 1))
    return lib.ZDICT_trainFromBuffer_fastCover(dst, cap, ctypes.create_string_buffer(flat, max(len(flat), 1)), sizes, len(recs), p)


def _code(v):
    return (1 << 64) - v


@pytest.mark.parametrize("case", [c for c in MANIFEST if "error" in c], ids=lambda c: c["name"])
def test_degenerate_inputs_match_libzstd(case):
    assert _code(_call_default(mgt.samples(case["recipe"]), case["cap"])) == case["error"]


def test_fixed_parameter_checks():
    recs = mgt.samples(dict(kind="text", seed=3, sizes=[200], count=20))
    oob, unsup, src = 42, 40, 72
    assert _code(_call_fixed(recs, 4096, k=200, d=7)) == oob          # FASTCOVER_checkParameters: d in {6, 8}
    assert _code(_call_fixed(recs, 4096, k=0, d=8)) == oob
    assert _code(_call_fixed(recs, 4096, k=5000, d=8)) == oob         # k <= capacity
    assert _code(_call_fixed(recs, 4096, k=6, d=8)) == oob            # d <= k
    assert _code(_call_fixed(recs, 4096, k=200, d=8, accel=11)) == oob
    assert _code(_call_fixed(recs, 4096, k=200, d=8, f=32)) == oob
    assert _code(_call_fixed([], 4096, k=200, d=8)) == src            # no samples
    assert _code(_call_fixed(recs, 255, k=200, d=8)) == 70            # capacity under 256
    assert _code(_call_fixed(recs, 4096, k=200, d=8, f=25)) == unsup  # the 2^f frequency copies: f <= 24
    assert _code(_call_fixed(recs, 4096, k=200, d=8, shrinkDict=1)) == unsup
    assert _code(_call_fixed(recs[:4], 4096, k=200, d=8)) == src      # fewer than 5 training samples


def test_optimize_parameter_checks():
    lib = _ffi.load()
    recs = mgt.samples(dict(kind="text", seed=4, sizes=[200], count=20))
    flat = b"".join(recs)
    sizes = (ctypes.c_size_t * len(recs))(*[len(r) for r in recs])
    src = ctypes.create_string_buffer(flat, len(flat))
    dst = ctypes.create_string_buffer(4096)

    def run(n=len(recs), cap=4096, **kw):
        p = _ffi.ZDICT_fastCover_params_t()
        for k, v in kw.items():
            setattr(p, k, v)
        return _code(lib.ZDICT_optimizeTrainFromBuffer_fastCover(dst, cap, src, sizes, n, ctypes.byref(p)))

    assert run(splitPoint=1.5) == 42
    assert run(accel=11) == 42
    assert run(k=4, d=8) == 42                                         # kMinK < kMaxD
    assert run(n=0) == 72
    assert run(cap=100) == 70
    assert run(n=6) == 72                                              # 6 * 0.75 = 4 training samples


def test_dict_builder_mirror_raises_like_ensure_zdict_success():
    with pytest.raises(z.ZstdException) as e:
        z.DictBuilder.train_from_buffer([b"x" * 300] * 20, 100)
    assert e.value.Code == z.ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall
    with pytest.raises(z.ZstdException) as e:
        z.DictBuilder.TrainFromBuffer([b"abc"] * 3)
    assert e.value.Code == z.ZSTD_ErrorCode.ZSTD_error_srcSize_wrong
