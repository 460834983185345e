"""CPU tests of the gather read's C ABI (include/zstd_mi355x.h "Gather reads"): the symbols exist and are typed, the cases that never
reach a kernel answer as the header says — with or without a GPU in the machine —, and the host's run packing (zmi_pack_runs.h) is
built with a stand-alone main under AddressSanitizer and UBSan and run over an empty list, one run that is the stream's whole front,
and 1000 seeded runs.  No kernel is launched here."""
import ctypes
import os
import subprocess

import pytest

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from host_cc import host_compiler
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC = ZSTD_ErrorCode.ZSTD_error_GENERIC


def _arrays(n):
    return ((ctypes.c_ulonglong * n)(), (ctypes.c_size_t * n)(), (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)())


def test_symbols_are_exported_and_typed():
    lib = _ffi.load()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("ZSTDMI_decompressRanges", "ZSTDMI_debugLastRangesFrames", "ZSTDMI_debugLastRangesAlone", "ZSTDMI_debugLastRangesStaged"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    res, args = _ffi.SIGNATURES["ZSTDMI_decompressRanges"]
    p = ctypes.POINTER
    assert res is ctypes.c_size_t
    assert args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, p(ctypes.c_ulonglong), p(ctypes.c_size_t), ctypes.c_size_t,
                    p(ctypes.c_void_p), p(ctypes.c_size_t), p(ctypes.c_size_t)]
    assert lib.ZSTDMI_debugLastRangesFrames.restype is ctypes.c_int and lib.ZSTDMI_debugLastRangesAlone.restype is ctypes.c_int
    assert lib.ZSTDMI_debugLastRangesStaged.restype is ctypes.c_longlong
    for name in ("ZSTDMI_debugLastRangesFrames", "ZSTDMI_debugLastRangesAlone", "ZSTDMI_debugLastRangesStaged"):
        assert _ffi.SIGNATURES[name][1] == [ctypes.c_void_p]
    assert callable(getattr(z.Decompressor, "unwrap_ranges"))
    # the header declares what the binding types
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    assert "size_t ZSTDMI_decompressRanges(ZSTD_DCtx* dctx, const void* src, size_t srcSize," in header
    assert "const unsigned long long* offsets, const size_t* lengths, size_t n," in header
    assert "int ZSTDMI_debugLastRangesFrames(const ZSTD_DCtx* dctx);" in header and "int ZSTDMI_debugLastRangesAlone(const ZSTD_DCtx* dctx);" in header
    assert "long long ZSTDMI_debugLastRangesStaged(const ZSTD_DCtx* dctx);" in header


def test_no_ranges_is_no_work():
    lib = _ffi.load()
    d = z.Decompressor()
    offs, lens, dsts, caps, got = _arrays(1)
    blob = bytes(32)                    # (not a seekable stream: with n == 0 nobody looks)
    assert lib.ZSTDMI_decompressRanges(d.dctx, blob, len(blob), offs, lens, 0, dsts, caps, got) == 0
    assert lib.ZSTDMI_decompressRanges(d.dctx, None, 0, None, None, 0, None, None, None) == 0
    assert lib.ZSTDMI_debugLastRangesFrames(d.dctx) == 0 and lib.ZSTDMI_debugLastRangesAlone(d.dctx) == 0
    assert lib.ZSTDMI_debugLastRangesStaged(d.dctx) == 0
    d.Dispose()


def test_null_context_and_null_arrays():
    lib = _ffi.load()
    offs, lens, dsts, caps, got = _arrays(1)
    blob = bytes(32)
    for n in (0, 1):
        r = lib.ZSTDMI_decompressRanges(None, blob, len(blob), offs, lens, n, dsts, caps, got)
        assert is_error(r) and get_error_code(r) == GENERIC
    assert lib.ZSTDMI_debugLastRangesFrames(None) == -1 and lib.ZSTDMI_debugLastRangesAlone(None) == -1
    assert lib.ZSTDMI_debugLastRangesStaged(None) == -1
    d = z.Decompressor()
    full = [offs, lens, dsts, caps, got]
    for hole in range(5):
        a = [None if k == hole else v for k, v in enumerate(full)]
        r = lib.ZSTDMI_decompressRanges(d.dctx, blob, len(blob), a[0], a[1], 1, a[2], a[3], a[4])
        assert is_error(r) and get_error_code(r) == GENERIC, hole
    d.Dispose()


def test_run_packing_under_sanitizers(tmp_path):
    exe = tmp_path / "pack_runs"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "pack_runs_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "empty list: 0 bytes" in out.stdout and "whole front: 100000 bytes ok" in out.stdout and "1000 seeded runs:" in out.stdout
    assert "refused: reversed, beyond the source, beyond the destination ok" in out.stdout and out.stdout.rstrip().endswith("done bad=0")
