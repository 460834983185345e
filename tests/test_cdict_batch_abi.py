"""CPU tests of ZSTDMI_compressBatchCDicts (include/zstd_mi355x.h "a CDict per entry"): the entry point and its two diagnostics are
exported, typed and declared; NULL and n == 0 handling; no CPU fallback; the header and the README no longer call the feature missing;
and the slot assignment (zmi_cdictset.h: dedupe, NULL entries, the bound of 65536 distinct CDicts, a pass's image) built with a
stand-alone main under AddressSanitizer and UBSan.  No kernel is launched here."""
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
    return (ctypes.c_void_p * max(n, 1))(), (ctypes.c_size_t * max(n, 1))()


@pytest.fixture()
def cctx():
    lib = _ffi.load()
    c = lib.ZSTD_createCCtx()
    yield lib, c
    lib.ZSTD_freeCCtx(c)


def test_symbols_are_exported_typed_and_declared():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    header = " ".join(open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read().split())
    v, s, ll = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong
    pv, ps = ctypes.POINTER(v), ctypes.POINTER(s)
    for name in ("ZSTDMI_compressBatchCDicts", "ZSTDMI_debugLastBatchPasses", "ZSTDMI_debugLastBatchSetChunks"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    assert _ffi.SIGNATURES["ZSTDMI_compressBatchCDicts"] == (s, [v, pv, ps, s, pv, ps, ps, pv])
    assert _ffi.SIGNATURES["ZSTDMI_debugLastBatchPasses"] == (ll, [v]) and _ffi.SIGNATURES["ZSTDMI_debugLastBatchSetChunks"] == (ll, [v])
    assert _ffi.load().ZSTDMI_debugLastBatchPasses.restype is ll
    assert ("size_t ZSTDMI_compressBatchCDicts(ZSTD_CCtx* cctx, const void* const* srcs, const size_t* srcSizes, size_t n, "
            "void* const* dsts, const size_t* dstCapacities, size_t* dstSizes, const ZSTD_CDict* const* cdicts);") in header
    assert "long long ZSTDMI_debugLastBatchPasses(const ZSTD_CCtx* cctx);" in header
    assert "long long ZSTDMI_debugLastBatchSetChunks(const ZSTD_CCtx* cctx);" in header
    assert "cdicts" in z.compress_batch.__code__.co_varnames and "compress_batch" in z.__all__


def test_header_and_readme_no_longer_call_it_missing():
    header = " ".join(open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read().split())
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "Many dictionaries, one batch" in readme
    for flat in (header, readme):
        assert "per-entry dictionaries in ZSTDMI_compressBatch" not in flat and "per-entry dictionaries in `ZSTDMI_compressBatch`" not in flat
        assert "per-entry CDicts in `ZSTDMI_compressBatch`" not in flat and "still makes one round per" not in flat
        assert "ZSTDMI_compressBatchCDicts" in flat


def test_empty_batch_returns_zero_and_touches_nothing(cctx):
    lib, c = cctx
    srcs, sizes = _arrays(0)
    dsts, caps = _arrays(0)
    got = (ctypes.c_size_t * 1)(777)
    assert lib.ZSTDMI_compressBatchCDicts(c, srcs, sizes, 0, dsts, caps, got, (ctypes.c_void_p * 1)()) == 0
    assert lib.ZSTDMI_compressBatchCDicts(c, None, None, 0, None, None, None, None) == 0       # (n == 0: the arrays are not looked at)
    assert got[0] == 777
    assert lib.ZSTDMI_debugLastBatchAlone(c) == 0 and lib.ZSTDMI_debugLastBatchPasses(c) == 0 and lib.ZSTDMI_debugLastBatchSetChunks(c) == 0


def test_null_context_and_null_arrays(cctx):
    lib, c = cctx
    assert lib.ZSTDMI_debugLastBatchPasses(None) == -1 and lib.ZSTDMI_debugLastBatchSetChunks(None) == -1
    srcs, sizes = _arrays(2)
    dsts, caps = _arrays(2)
    got = (ctypes.c_size_t * 2)()
    cds = (ctypes.c_void_p * 2)()
    r = lib.ZSTDMI_compressBatchCDicts(None, srcs, sizes, 2, dsts, caps, got, cds)
    assert is_error(r) and get_error_code(r) == GENERIC
    for missing in range(6):            # (cdicts included: the plain batch is the call for "no array")
        args = [srcs, sizes, dsts, caps, got, cds]
        args[missing] = None
        r = lib.ZSTDMI_compressBatchCDicts(c, args[0], args[1], 2, args[2], args[3], args[4], args[5])
        assert is_error(r) and get_error_code(r) == GENERIC, missing


def test_fails_loudly_without_gpu_as_the_plain_batch_does(cctx):
    """No CPU fallback: without a gfx950 device both batch calls fail as a whole with init_missing and touch nothing."""
    lib, c = cctx
    if lib.ZSTDMI_deviceCount() > 0:
        pytest.skip("a GPU is visible here")
    src = ctypes.create_string_buffer(b"some bytes to compress, twice: some bytes to compress", 53)
    dst = ctypes.create_string_buffer(b"\xA5" * 128, 128)
    srcs, sizes = _arrays(1)
    dsts, caps = _arrays(1)
    srcs[0], sizes[0], dsts[0], caps[0] = ctypes.addressof(src), 53, ctypes.addressof(dst), 128
    got = (ctypes.c_size_t * 1)(12345)
    plain = lib.ZSTDMI_compressBatch(c, srcs, sizes, 1, dsts, caps, got)
    r = lib.ZSTDMI_compressBatchCDicts(c, srcs, sizes, 1, dsts, caps, got, (ctypes.c_void_p * 1)())
    assert r == plain and is_error(r) and get_error_code(r) == ZSTD_ErrorCode.ZSTD_error_init_missing
    assert got[0] == 12345 and dst.raw == b"\xA5" * 128


def test_slot_assignment_under_sanitizers(tmp_path):
    exe = tmp_path / "cdictset"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "cdictset_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for line in ("empty: 0 slots bad=0", "dedupe: 4 slots bad=0", "one for all: 1 slots bad=0", "65536: 65537 slots bad=0", "one more refused ok bad=0", "image: bad=0"):
        assert line in out.stdout, out.stdout
    assert out.stdout.rstrip().endswith("done bad=0")
