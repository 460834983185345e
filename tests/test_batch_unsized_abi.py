"""CPU tests of ZSTDMI_DCtx_setBatchUnsized and ZSTDMI_debugLastBatchWorkspace (include/zstd_mi355x.h "frames without a content size
in the shared pass"): the symbols exist, are typed and declared, the setter's answers, NULL handling, an empty batch — none of which
touches a device —, the Python property, and the per-entry placement rule (zmi_batch_rescan.h, what batch_rescan_kernel runs) built with
a stand-alone main under AddressSanitizer and UBSan.  No kernel is launched here."""
import ctypes
import os
import subprocess

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from host_cc import host_compiler
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_typed_and_declared():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    for name in ("ZSTDMI_DCtx_setBatchUnsized", "ZSTDMI_debugLastBatchWorkspace"):
        assert hasattr(raw, name), name + " is not exported"
    assert _ffi.SIGNATURES["ZSTDMI_DCtx_setBatchUnsized"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_uint])
    assert _ffi.SIGNATURES["ZSTDMI_debugLastBatchWorkspace"] == (ctypes.c_longlong, [ctypes.c_void_p])
    assert _ffi.load().ZSTDMI_debugLastBatchWorkspace.restype is ctypes.c_longlong
    flat = " ".join(header.split())
    assert "size_t ZSTDMI_DCtx_setBatchUnsized(ZSTD_DCtx* dctx, unsigned mode);" in flat
    assert "long long ZSTDMI_debugLastBatchWorkspace(const ZSTD_DCtx* dctx);" in flat
    assert "(unless ZSTDMI_DCtx_setBatchUnsized)" in flat, "the batch comment does not name the switch"


def test_setter_answers():
    lib = _ffi.load()
    r = lib.ZSTDMI_DCtx_setBatchUnsized(None, 1)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    r = lib.ZSTDMI_DCtx_setBatchUnsized(None, 0)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    d = lib.ZSTD_createDCtx()
    try:
        for wrong in (2, 3, 0xFFFFFFFF):
            r = lib.ZSTDMI_DCtx_setBatchUnsized(d, wrong)
            assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound, wrong
        for mode in (0, 1, 1, 0):
            assert lib.ZSTDMI_DCtx_setBatchUnsized(d, mode) == 0, mode
        r = lib.ZSTDMI_DCtx_setOverlap(d, 3)        # (the setter it is modelled on answers alike)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound
    finally:
        lib.ZSTD_freeDCtx(d)


def test_workspace_without_a_context_and_before_any_call():
    lib = _ffi.load()
    assert lib.ZSTDMI_debugLastBatchWorkspace(None) == -1
    d = lib.ZSTD_createDCtx()
    try:
        assert lib.ZSTDMI_debugLastBatchWorkspace(d) == 0
    finally:
        lib.ZSTD_freeDCtx(d)


def test_empty_batch_with_the_switch_on():
    lib = _ffi.load()
    d = lib.ZSTD_createDCtx()
    try:
        assert lib.ZSTDMI_DCtx_setBatchUnsized(d, 1) == 0
        assert lib.ZSTDMI_decompressBatch(d, None, None, 0, None, None, None) == 0
        assert lib.ZSTDMI_debugLastBatchAloneD(d) == 0 and lib.ZSTDMI_debugLastBatchWorkspace(d) == 0
    finally:
        lib.ZSTD_freeDCtx(d)


def test_python_property_round_trips():
    with z.Decompressor() as d:
        assert d.batch_unsized is False
        d.batch_unsized = True
        assert d.batch_unsized is True
        d.batch_unsized = 0
        assert d.batch_unsized is False
        assert z.decompress_batch(d, [], []) == []


def test_placement_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "batch_rescan"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "batch_rescan_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    for n in (0, 1, 63, 64, 65, 5000):
        assert f"n={n} at capacity: {n} frames" in out.stdout, out.stdout
    for line in ("n=5000 sum 2^64-1: 5000 frames", "n=65 sum 2^64: 65 frames", "n=64 sum far beyond: 64 frames", "lane rules ok"):
        assert line in out.stdout, out.stdout
    assert " bad=1" not in out.stdout and out.stdout.rstrip().endswith("done bad=0")
