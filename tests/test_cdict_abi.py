"""CPU tests of the digested-dictionary C ABI (include/zstd_mi355x.h "digested dictionaries"): the symbols exist and are typed, the cases
that never reach a kernel answer as the header says — with or without a GPU in the machine —, the two host-only dictID readers agree with
the dictionaries and frames under tests/golden, and their parser (zmi_dictid.h) is built with a stand-alone main under AddressSanitizer
and UBSan and run over every frame header descriptor at every truncation.  No kernel is launched here."""
import ctypes
import os
import struct
import subprocess

import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from host_cc import host_compiler
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GENERIC = ZSTD_ErrorCode.ZSTD_error_GENERIC

NEW = {
    "ZSTD_createCDict": "ZSTD_CDict* ZSTD_createCDict(const void* dict, size_t dictSize, int compressionLevel);",
    "ZSTDMI_createCDictOnDevice": "ZSTD_CDict* ZSTDMI_createCDictOnDevice(const void* dict, size_t dictSize, int compressionLevel, int device);",
    "ZSTD_freeCDict": "ZSTD_freeCDict(ZSTD_CDict* cdict);",
    "ZSTD_sizeof_CDict": "ZSTD_sizeof_CDict(const ZSTD_CDict* cdict);",
    "ZSTD_getDictID_fromCDict": "ZSTD_getDictID_fromCDict(const ZSTD_CDict* cdict);",
    "ZSTD_CCtx_refCDict": "ZSTD_CCtx_refCDict(ZSTD_CCtx* cctx, const ZSTD_CDict* cdict);",
    "ZSTD_compress_usingCDict": "ZSTD_compress_usingCDict(ZSTD_CCtx* cctx, void* dst, size_t dstCapacity, const void* src, size_t srcSize, const ZSTD_CDict* cdict);",
    "ZSTD_createDDict": "ZSTD_DDict* ZSTD_createDDict(const void* dict, size_t dictSize);",
    "ZSTDMI_createDDictOnDevice": "ZSTD_DDict* ZSTDMI_createDDictOnDevice(const void* dict, size_t dictSize, int device);",
    "ZSTD_freeDDict": "ZSTD_freeDDict(ZSTD_DDict* ddict);",
    "ZSTD_sizeof_DDict": "ZSTD_sizeof_DDict(const ZSTD_DDict* ddict);",
    "ZSTD_getDictID_fromDDict": "ZSTD_getDictID_fromDDict(const ZSTD_DDict* ddict);",
    "ZSTD_DCtx_refDDict": "ZSTD_DCtx_refDDict(ZSTD_DCtx* dctx, const ZSTD_DDict* ddict);",
    "ZSTD_decompress_usingDDict": "ZSTD_decompress_usingDDict(ZSTD_DCtx* dctx, void* dst, size_t dstCapacity, const void* src, size_t srcSize, const ZSTD_DDict* ddict);",
    "ZSTD_getDictID_fromDict": "ZSTD_getDictID_fromDict(const void* dict, size_t dictSize);",
    "ZSTD_getDictID_fromFrame": "ZSTD_getDictID_fromFrame(const void* src, size_t srcSize);",
    "ZSTDMI_debugDictUploads": "ZSTDMI_debugDictUploads(const ZSTD_CCtx* cctx);",
    "ZSTDMI_debugDictUploadsD": "ZSTDMI_debugDictUploadsD(const ZSTD_DCtx* dctx);",
    "ZSTDMI_debugLastDictTableBlocks": "ZSTDMI_debugLastDictTableBlocks(const ZSTD_DCtx* dctx);",
}


def golden_bytes(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def test_symbols_are_exported_and_typed():
    lib = _ffi.load()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "zstd_mi355x.h")).read()
    for name, decl in NEW.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _ffi.SIGNATURES, f"{name} has no ctypes signature"
        assert decl in header, f"{name} is not declared as the reference declares it"
    v, s, i, u, ll = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint, ctypes.c_longlong
    assert _ffi.SIGNATURES["ZSTD_createCDict"] == (v, [v, s, i]) and _ffi.SIGNATURES["ZSTDMI_createCDictOnDevice"] == (v, [v, s, i, i])
    assert _ffi.SIGNATURES["ZSTD_createDDict"] == (v, [v, s]) and _ffi.SIGNATURES["ZSTDMI_createDDictOnDevice"] == (v, [v, s, i])
    for name in ("ZSTD_freeCDict", "ZSTD_sizeof_CDict", "ZSTD_freeDDict", "ZSTD_sizeof_DDict"):
        assert _ffi.SIGNATURES[name] == (s, [v])
    for name in ("ZSTD_getDictID_fromCDict", "ZSTD_getDictID_fromDDict"):
        assert _ffi.SIGNATURES[name] == (u, [v])
    assert _ffi.SIGNATURES["ZSTD_CCtx_refCDict"] == (s, [v, v]) and _ffi.SIGNATURES["ZSTD_DCtx_refDDict"] == (s, [v, v])
    assert _ffi.SIGNATURES["ZSTD_compress_usingCDict"] == (s, [v, v, s, v, s, v]) and _ffi.SIGNATURES["ZSTD_decompress_usingDDict"] == (s, [v, v, s, v, s, v])
    assert _ffi.SIGNATURES["ZSTD_getDictID_fromDict"] == (u, [v, s]) and _ffi.SIGNATURES["ZSTD_getDictID_fromFrame"] == (u, [v, s])
    for name in ("ZSTDMI_debugDictUploads", "ZSTDMI_debugDictUploadsD", "ZSTDMI_debugLastDictTableBlocks"):
        assert _ffi.SIGNATURES[name] == (ll, [v])
    assert lib.ZSTDMI_debugDictUploads.restype is ll
    for what in ("_byReference", "_advanced", "ZSTD_d_refMultipleDDicts", "ZSTD_estimateCDictSize"):
        assert what in header, f"the header does not say that {what} is not provided"
    for cls, members in ((z.CDict, ("Dispose", "dict_id", "sizeof", "__enter__")), (z.DDict, ("Dispose", "dict_id", "sizeof", "__enter__")),
                         (z.Compressor, ("RefCDict", "WrapUsingCDict")), (z.Decompressor, ("RefDDict", "UnwrapUsingDDict"))):
        for m in members:
            assert hasattr(cls, m), (cls.__name__, m)


def test_null_handling():
    lib = _ffi.load()
    assert lib.ZSTD_freeCDict(None) == 0 and lib.ZSTD_freeDDict(None) == 0
    assert lib.ZSTD_sizeof_CDict(None) == 0 and lib.ZSTD_sizeof_DDict(None) == 0
    assert lib.ZSTD_getDictID_fromCDict(None) == 0 and lib.ZSTD_getDictID_fromDDict(None) == 0
    for r in (lib.ZSTD_CCtx_refCDict(None, None), lib.ZSTD_DCtx_refDDict(None, None)):
        assert is_error(r) and get_error_code(r) == GENERIC
    assert lib.ZSTDMI_debugDictUploads(None) == -1 and lib.ZSTDMI_debugDictUploadsD(None) == -1 and lib.ZSTDMI_debugLastDictTableBlocks(None) == -1
    with z.Compressor() as c, z.Decompressor() as d:
        assert lib.ZSTD_CCtx_refCDict(c.cctx, None) == 0 and lib.ZSTD_DCtx_refDDict(d.dctx, None) == 0
        c.RefCDict(None)
        d.RefDDict(None)
        assert lib.ZSTDMI_debugDictUploads(c.cctx) == 0 and lib.ZSTDMI_debugDictUploadsD(d.dctx) == 0
        assert lib.ZSTDMI_debugLastDictTableBlocks(d.dctx) == 0
        out = ctypes.create_string_buffer(64)
        for r in (lib.ZSTD_compress_usingCDict(c.cctx, out, 64, b"abc", 3, None), lib.ZSTD_compress_usingCDict(None, out, 64, b"abc", 3, None),
                  lib.ZSTD_decompress_usingDDict(d.dctx, out, 64, b"abc", 3, None), lib.ZSTD_decompress_usingDDict(None, out, 64, b"abc", 3, None)):
            assert is_error(r) and get_error_code(r) == GENERIC


def test_dict_id_from_dict():
    lib = _ffi.load()
    for name in ("train_default_json.dict", "trained_16k.dict"):
        dic = golden_bytes(name)
        want = struct.unpack_from("<I", dic, 4)[0]
        assert want != 0
        assert lib.ZSTD_getDictID_fromDict(dic, len(dic)) == want and z.get_dict_id_from_dict(dic) == want
        assert lib.ZSTD_getDictID_fromDict(dic, 8) == want and lib.ZSTD_getDictID_fromDict(dic, 7) == 0
    raw = golden_bytes("rawcontent_6000.dict")
    assert lib.ZSTD_getDictID_fromDict(raw, len(raw)) == 0 and z.get_dict_id_from_dict(raw) == 0
    assert lib.ZSTD_getDictID_fromDict(b"7 bytes", 7) == 0
    assert lib.ZSTD_getDictID_fromDict(None, 0) == 0 and z.get_dict_id_from_dict(None) == 0


def test_dict_id_from_frame():
    lib = _ffi.load()
    want = struct.unpack_from("<I", golden_bytes("trained_16k.dict"), 4)[0]
    names = sorted(os.listdir(GOLDEN))
    fmt, raw = [n for n in names if n.startswith("dict_fmt_") and n.endswith(".zst")], [n for n in names if n.startswith("dict_raw_") and n.endswith(".zst")]
    assert len(fmt) >= 7 and len(raw) >= 4
    for n in fmt:
        blob = golden_bytes(n)
        assert lib.ZSTD_getDictID_fromFrame(blob, len(blob)) == want and z.get_dict_id_from_frame(blob) == want, n
    for n in raw:
        blob = golden_bytes(n)
        assert lib.ZSTD_getDictID_fromFrame(blob, len(blob)) == 0, n
    skippable = struct.pack("<II", 0x184D2A53, 4) + b"\x01\x02\x03\x04"
    blob = golden_bytes(fmt[0])
    assert lib.ZSTD_getDictID_fromFrame(skippable, len(skippable)) == 0
    assert lib.ZSTD_getDictID_fromFrame(blob, 3) == 0 and lib.ZSTD_getDictID_fromFrame(None, 0) == 0
    assert lib.ZSTD_getDictID_fromFrame(b"\x29" + blob[1:], len(blob)) == 0      # a wrong magic


def test_no_device_no_digest():
    lib = _ffi.load()
    if lib.ZSTDMI_deviceCount() != 0:
        return      # (with a device the constructors are the GPU suite's: tests/test_gpu_cdict.py, tests/test_gpu_ddict.py)
    dic = golden_bytes("trained_16k.dict")
    assert not lib.ZSTD_createCDict(dic, len(dic), 3) and not lib.ZSTD_createDDict(dic, len(dic))
    assert not lib.ZSTDMI_createCDictOnDevice(dic, len(dic), 3, 0) and not lib.ZSTDMI_createDDictOnDevice(dic, len(dic), 0)
    for make in (lambda: z.CDict(dic), lambda: z.DDict(dic)):
        try:
            make()
        except ValueError:
            continue
        raise AssertionError("a digest without a device")


def test_dict_id_parsers_under_sanitizers(tmp_path):
    exe = tmp_path / "dictid"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "dictid_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "frame headers: 128 descriptors bad=0" in out.stdout and "refused: reserved bit, skippable, wrong magic ok" in out.stdout
    assert "dictionaries: formatted, raw, short ok" in out.stdout and out.stdout.rstrip().endswith("done bad=0")
