"""CPU tests of ZSTD_d_refMultipleDDicts (include/zstd_mi355x.h "many dictionaries, one context"): the parameter and the diagnostic exist
and are typed, the parameter's round trip and bounds, NULL handling — none of which touches a device —, and the DDict set itself
(zmi_dictset.h: insert, replace, the sorted image, the lookup the walk kernels run) built with a stand-alone main under AddressSanitizer
and UBSan.  No kernel is launched here."""
import ctypes
import os
import subprocess

import pytest

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from host_cc import host_compiler
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM = 1003


def test_symbol_is_exported_typed_and_declared():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    assert hasattr(raw, "ZSTDMI_debugLastSetFrames"), "ZSTDMI_debugLastSetFrames is not exported"
    assert _ffi.SIGNATURES["ZSTDMI_debugLastSetFrames"] == (ctypes.c_longlong, [ctypes.c_void_p])
    assert _ffi.load().ZSTDMI_debugLastSetFrames.restype is ctypes.c_longlong
    assert "ZSTDMI_debugLastSetFrames(const ZSTD_DCtx* dctx);" in header
    assert "ZSTD_d_refMultipleDDicts = 1003" in header and "ZSTD_rmd_refSingleDDict = 0" in header and "ZSTD_rmd_refMultipleDDicts = 1" in header
    assert z.ZSTD_d_refMultipleDDicts == PARAM and z.ZSTD_rmd_refSingleDDict == 0 and z.ZSTD_rmd_refMultipleDDicts == 1
    assert z.ZSTD_d_windowLogMax == 100


def test_header_and_readme_state_what_is_open():
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "Many dictionaries, one context (`ZSTD_d_refMultipleDDicts`)" in readme
    for text in (header, readme):
        flat = " ".join(text.split())
        assert "constructors, ZSTD_d_refMultipleDDicts and" not in flat and "constructors, `ZSTD_d_refMultipleDDicts`" not in flat
        assert "ZSTDMI_compressBatch" in flat and "segmented streams" in flat and "several device workers" in flat
    assert "DDict of the last ZSTD_DCtx_refDDict" in " ".join(header.split()), "the header does not state the difference from the reference"


def test_parameter_round_trip_and_bounds():
    lib = _ffi.load()
    d = lib.ZSTD_createDCtx()
    try:
        v = ctypes.c_int(-7)
        assert lib.ZSTD_DCtx_getParameter(d, PARAM, ctypes.byref(v)) == 0 and v.value == 0, "the default is ZSTD_rmd_refSingleDDict"
        assert lib.ZSTD_DCtx_setParameter(d, PARAM, 1) == 0
        assert lib.ZSTD_DCtx_getParameter(d, PARAM, ctypes.byref(v)) == 0 and v.value == 1
        for wrong in (2, -1, 1003):
            r = lib.ZSTD_DCtx_setParameter(d, PARAM, wrong)
            assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound, wrong
        assert lib.ZSTD_DCtx_getParameter(d, PARAM, ctypes.byref(v)) == 0 and v.value == 1, "a refused value leaves the parameter as it was (sticky)"
        assert lib.ZSTD_DCtx_setParameter(d, 100, 20) == 0          # (another parameter does not disturb it)
        assert lib.ZSTD_DCtx_getParameter(d, PARAM, ctypes.byref(v)) == 0 and v.value == 1
        assert lib.ZSTD_DCtx_setParameter(d, PARAM, 0) == 0
        assert lib.ZSTD_DCtx_getParameter(d, PARAM, ctypes.byref(v)) == 0 and v.value == 0
        r = lib.ZSTD_DCtx_setParameter(d, 1002, 1)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_parameter_unsupported, "the neighbouring experimental parameter stays unsupported"
    finally:
        lib.ZSTD_freeDCtx(d)


def test_null_handling():
    lib = _ffi.load()
    assert lib.ZSTDMI_debugLastSetFrames(None) == -1
    r = lib.ZSTD_DCtx_setParameter(None, PARAM, 1)
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    v = ctypes.c_int(0)
    r = lib.ZSTD_DCtx_getParameter(None, PARAM, ctypes.byref(v))
    assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    d = lib.ZSTD_createDCtx()
    try:
        r = lib.ZSTD_DCtx_getParameter(d, PARAM, None)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
        assert lib.ZSTDMI_debugLastSetFrames(d) == 0, "a context that has decoded nothing"
        assert lib.ZSTD_DCtx_setParameter(d, PARAM, 1) == 0
        assert lib.ZSTD_DCtx_refDDict(d, None) == 0, "refDDict(NULL) with the parameter on clears the current DDict and is no error"
        assert lib.ZSTD_DCtx_refDDict(d, None) == 0
        assert lib.ZSTDMI_debugLastSetFrames(d) == 0
        r = lib.ZSTD_DCtx_refDDict(None, None)
        assert is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_GENERIC
    finally:
        lib.ZSTD_freeDCtx(d)


def test_python_decompressor_names_the_parameter():
    with z.Decompressor() as d:
        assert d.GetParameter(z.ZSTD_d_refMultipleDDicts) == 0
        d.SetParameter(z.ZSTD_d_refMultipleDDicts, z.ZSTD_rmd_refMultipleDDicts)
        assert d.GetParameter(z.ZSTD_d_refMultipleDDicts) == 1
        d.RefDDict(None)
        assert d._ddict is None and d._ddict_set == {}
        with pytest.raises(z.ZstdException) as ei:
            d.SetParameter(z.ZSTD_d_refMultipleDDicts, 2)
        assert ei.value.code == ZSTD_ErrorCode.ZSTD_error_parameter_outOfBound


def test_set_and_lookup_under_sanitizers(tmp_path):
    exe = tmp_path / "dictset"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "dictset_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for line in ("empty: 0 entries bad=0", "one: 1 entries bad=0", "two (first and last id): 2 entries bad=0",
                 "three (adjacent across the sign bit): 3 entries bad=0", "4096: 4096 entries bad=0", "one more refused ok"):
        assert line in out.stdout, out.stdout
    assert out.stdout.rstrip().endswith("done bad=0")
