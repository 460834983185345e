"""CPU tests of the segmented stream decoder's C ABI (include/zstd_mi355x.h "Segmented stream decoding"): the symbols exist and are
typed, a NULL context answers as the header says, the setter is sticky and touches no device — it works with or without a GPU in the
machine —, the default is off, and the host scan that finds the blocks defining a frame's tables (zmi_stream_scan.h) is built with a
stand-alone main under AddressSanitizer and UBSan and compared with a second implementation over every fixture and over every
truncation of three of them.  No kernel is launched here."""
import ctypes
import glob
import os
import subprocess

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error
from zstdsharp_amd.streams import DecompressionStream
from test_ranges_abi import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC = ZSTD_ErrorCode.ZSTD_error_GENERIC
NAMES = ("ZSTDMI_DCtx_setStreamSegment", "ZSTDMI_debugStreamPeakInput", "ZSTDMI_debugStreamSegments")


def test_symbols_are_exported_and_typed():
    lib = _ffi.load()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
    assert _ffi.SIGNATURES["ZSTDMI_DCtx_setStreamSegment"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_size_t])
    assert lib.ZSTDMI_debugStreamPeakInput.restype is ctypes.c_longlong and lib.ZSTDMI_debugStreamSegments.restype is ctypes.c_int
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    assert "size_t ZSTDMI_DCtx_setStreamSegment(ZSTD_DCtx* dctx, size_t bytes);" in header
    assert "long long ZSTDMI_debugStreamPeakInput(const ZSTD_DCtx* dctx);" in header
    assert "int ZSTDMI_debugStreamSegments(const ZSTD_DCtx* dctx);" in header


def test_null_context():
    lib = _ffi.load()
    for v in (0, 1, 1 << 20):
        r = lib.ZSTDMI_DCtx_setStreamSegment(None, v)
        assert is_error(r) and get_error_code(r) == GENERIC
    assert lib.ZSTDMI_debugStreamPeakInput(None) == -1
    assert lib.ZSTDMI_debugStreamSegments(None) == -1


def test_default_is_off_and_the_setter_is_sticky_without_a_device():
    """(this test passes on a machine without a GPU: had the setter touched a device it would have failed there)"""
    lib = _ffi.load()
    d = z.Decompressor()
    assert d.stream_segment == 0
    assert lib.ZSTDMI_debugStreamPeakInput(d.dctx) == 0 and lib.ZSTDMI_debugStreamSegments(d.dctx) == 0
    for v in (1, 65536, (1 << 40) + 3, 0, 262144):
        assert lib.ZSTDMI_DCtx_setStreamSegment(d.dctx, v) == 0
        d.stream_segment = v
        assert d.stream_segment == v
    assert lib.ZSTDMI_debugStreamPeakInput(d.dctx) == 0 and lib.ZSTDMI_debugStreamSegments(d.dctx) == 0
    d.Dispose()
    import io
    d = z.Decompressor()
    with DecompressionStream(io.BytesIO(b""), decompressor=d):
        assert d.stream_segment == 0                   # segment=None leaves the decompressor as it is
    with DecompressionStream(io.BytesIO(b""), decompressor=d, segment=4096) as ds:
        assert d.stream_segment == 4096
        assert ds.Read(16) == b""                       # (an empty stream: nothing reaches a device)
    d.Dispose()


def test_host_scan_under_sanitizers(tmp_path):
    exe = tmp_path / "stream_scan"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "stream_scan_harness.cpp")])
    gold = os.path.join(ROOT, "tests", "golden")
    cut = [os.path.join(gold, f) for f in ("mixed_150000_l19.zst", "text_5000_x2_multiframe.zst", "zipf_40000_l5_chk.zst")]
    whole = sorted(f for f in glob.glob(os.path.join(gold, "*.zst")) if f not in cut)
    assert len(whole) >= 30
    out = subprocess.run([str(exe)] + whole + ["--cut"] + cut, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert f"files {len(whole) + 3} cut 3 " in out.stdout and out.stdout.rstrip().endswith("done bad=0")
    # (the fixtures do hold what the scan is for: blocks that define tables)
    definers = int(out.stdout.rsplit("definers ", 1)[1].split()[0])
    assert definers > 1000
