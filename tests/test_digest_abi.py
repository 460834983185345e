"""CPU tests of the C ABI of piece digests (include/zstd_mi355x.h "Piece digests"): the symbols exist, are typed and declared;
ZSTDMI_digestSize; every answer ZSTDMI_digestPieces gives before it looks for a device, in the header's order of precedence; and the
serial model both kernels are written from (zmi_digest.h through ZSTDMI_debugDigestModel) against the oracle's XXH64, hashlib's SHA-256
and the published vectors.  No kernel is launched."""
import ctypes
import hashlib
import os

import pytest

import datagen
import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zstd_mi355x.h")
E = ZSTD_ErrorCode
s, v, u, ps = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint, ctypes.POINTER(ctypes.c_size_t)
SYMBOLS = {
    "ZSTDMI_digestSize": (s, [u]),
    "ZSTDMI_digestPieces": (s, [v, v, s, ps, s, u, v, s]),
    "ZSTDMI_contentCutsDigests": (s, [v, v, s, u, u, ps, s, ps, v, s]),
    "ZSTDMI_debugDigestModel": (s, [u, v, s, v]),
}
XXH64, SHA256 = 1, 2
SIZE_MAX = (1 << 64) - 1


def sizes_of(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


def code(r):
    return get_error_code(r) if is_error(r) else None


@pytest.fixture
def cctx():
    lib = _ffi.load()
    c = lib.ZSTD_createCCtx()
    yield c
    lib.ZSTD_freeCCtx(c)


def model(kind, data):
    lib = _ffi.load()
    out = ctypes.create_string_buffer(b"\xA5" * 40, 40)
    assert lib.ZSTDMI_debugDigestModel(kind, data if data else None, len(data), out) == 0
    n = lib.ZSTDMI_digestSize(kind)
    assert out.raw[n:] == b"\xA5" * (40 - n)
    return out.raw[:n]


def want(kind, data, oracle):
    if kind == SHA256:
        return hashlib.sha256(data).digest()
    return int(oracle.lib().zso_xxh64(data, len(data), 0)).to_bytes(8, "little")


# ---- symbols ----
def test_symbols_are_exported_typed_and_declared():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name, sig in SYMBOLS.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert _ffi.SIGNATURES[name] == sig, name
    text = " ".join(open(HEADER).read().split())
    for line in ["enum { ZSTDMI_digest_xxh64 = 1, ZSTDMI_digest_sha256 = 2 };",
                 "size_t ZSTDMI_digestSize(unsigned kind);",
                 "size_t ZSTDMI_digestPieces(ZSTD_CCtx* cctx, const void* src, size_t srcSize, const size_t* pieceSizes, size_t nPieces, unsigned kind, "
                 "void* digests, size_t digestsCapacity);",
                 "size_t ZSTDMI_contentCutsDigests(ZSTD_CCtx* cctx, const void* src, size_t srcSize, unsigned avgLog, unsigned kind, "
                 "size_t* pieceSizes, size_t capacity, size_t* nPieces, void* digests, size_t digestsCapacity);",
                 "size_t ZSTDMI_debugDigestModel(unsigned kind, const void* src, size_t srcSize, void* digest);"]:
        assert line in text, line
    assert callable(z.piece_digests) and callable(z.content_cuts_digests)


def test_digest_size():
    lib = _ffi.load()
    assert lib.ZSTDMI_digestSize(XXH64) == 8 and lib.ZSTDMI_digestSize(SHA256) == 32
    for kind in (0, 3, 4, 32, 0xFFFFFFFF):
        assert lib.ZSTDMI_digestSize(kind) == 0


# ---- the answers given before a device is looked for, each against the conditions that rank behind it ----
def test_answers_in_their_order_of_precedence(cctx):
    lib = _ffi.load()
    data = b"0123456789" * 10
    sizes = sizes_of([10, 20, 30])
    out = ctypes.create_string_buffer(b"\xA5" * 128, 128)
    call = lib.ZSTDMI_digestPieces
    # a NULL context, whatever else is wrong
    assert code(call(None, data, 100, sizes, 3, SHA256, out, 128)) == E.ZSTD_error_GENERIC
    assert code(call(None, None, 5, None, 3, 9, None, 0)) == E.ZSTD_error_GENERIC
    assert code(call(None, None, 0, None, 0, XXH64, None, 0)) == E.ZSTD_error_GENERIC
    # NULL arrays with pieces: in front of a bad kind, a short capacity, a wrong sum and a NULL source
    assert code(call(cctx, data, 100, None, 3, SHA256, out, 128)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, data, 100, sizes, 3, SHA256, None, 128)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, None, 5, None, 3, 9, out, 0)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, None, 5, sizes, 3, 9, None, 0)) == E.ZSTD_error_GENERIC
    # a kind that is none: in front of no pieces, a short capacity, a wrong sum and a NULL source
    for kind in (0, 3, 0xFFFFFFFF):
        assert code(call(cctx, data, 100, sizes, 3, kind, out, 128)) == E.ZSTD_error_parameter_outOfBound
        assert code(call(cctx, None, 0, None, 0, kind, None, 0)) == E.ZSTD_error_parameter_outOfBound
        assert code(call(cctx, None, 5, sizes, 3, kind, out, 0)) == E.ZSTD_error_parameter_outOfBound
    # no pieces: 0 with every pointer NULL, and in front of a NULL source with a size
    for kind in (XXH64, SHA256):
        assert call(cctx, None, 0, None, 0, kind, None, 0) == 0
        assert call(cctx, None, 5, None, 0, kind, None, 0) == 0
        assert call(cctx, data, 100, sizes, 0, kind, out, 0) == 0
    # a capacity one byte short: in front of a wrong sum and a NULL source; nothing is written
    for kind, need in ((XXH64, 24), (SHA256, 96)):
        assert code(call(cctx, data, 100, sizes, 3, kind, out, need - 1)) == E.ZSTD_error_dstSize_tooSmall
        assert code(call(cctx, data, 59, sizes, 3, kind, out, need - 1)) == E.ZSTD_error_dstSize_tooSmall
        assert code(call(cctx, None, 100, sizes, 3, kind, out, 0)) == E.ZSTD_error_dstSize_tooSmall
    assert code(call(cctx, data, 100, sizes, SIZE_MAX // 8, SHA256, out, SIZE_MAX)) == E.ZSTD_error_dstSize_tooSmall    # (the product overflows)
    # a sum one above srcSize, and one that overflows size_t: in front of a NULL source
    for kind, need in ((XXH64, 24), (SHA256, 96)):
        assert code(call(cctx, data, 59, sizes, 3, kind, out, need)) == E.ZSTD_error_srcSize_wrong
        assert code(call(cctx, None, 59, sizes, 3, kind, out, need)) == E.ZSTD_error_srcSize_wrong
        assert code(call(cctx, data, SIZE_MAX, sizes_of([SIZE_MAX, 1, 0]), 3, kind, out, need)) == E.ZSTD_error_srcSize_wrong
        assert code(call(cctx, data, 100, sizes_of([SIZE_MAX - 5, 3, 3]), 3, kind, out, need)) == E.ZSTD_error_srcSize_wrong
        # a NULL source with a size (the sum fits)
        assert code(call(cctx, None, 60, sizes, 3, kind, out, need)) == E.ZSTD_error_srcSize_wrong
        assert code(call(cctx, None, 1, sizes_of([0, 0, 0]), 3, kind, out, need)) == E.ZSTD_error_srcSize_wrong
    assert out.raw == b"\xA5" * 128
    # behind them a device is looked for: without one the call fails loudly and writes nothing
    r = call(cctx, data, 60, sizes, 3, SHA256, out, 96)
    if lib.ZSTDMI_deviceCount() > 0:
        assert r == 0
    else:
        assert code(r) == E.ZSTD_error_init_missing and out.raw == b"\xA5" * 128


def test_fused_call_answers_before_a_device(cctx):
    lib = _ffi.load()
    sizes, got = sizes_of([0] * 4), ctypes.c_size_t(77)
    out = ctypes.create_string_buffer(128)
    call = lib.ZSTDMI_contentCutsDigests
    assert code(call(None, None, 0, 12, SHA256, sizes, 4, ctypes.byref(got), out, 128)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, None, 0, 12, SHA256, sizes, 4, None, out, 128)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, None, 0, 12, SHA256, None, 4, ctypes.byref(got), out, 128)) == E.ZSTD_error_GENERIC
    assert code(call(cctx, None, 0, 12, SHA256, sizes, 4, ctypes.byref(got), None, 128)) == E.ZSTD_error_GENERIC
    for avg_log in (0, 11, 17):     # avgLog first, then the kind
        assert code(call(cctx, None, 0, avg_log, 9, sizes, 4, ctypes.byref(got), out, 128)) == E.ZSTD_error_parameter_outOfBound
    for kind in (0, 3):             # the kind in front of a source of 2^32 bytes
        assert code(call(cctx, None, 1 << 32, 12, kind, sizes, 4, ctypes.byref(got), out, 128)) == E.ZSTD_error_parameter_outOfBound
    assert code(call(cctx, None, 1 << 32, 12, XXH64, sizes, 4, ctypes.byref(got), out, 128)) == E.ZSTD_error_parameter_unsupported
    assert got.value == 0
    if lib.ZSTDMI_deviceCount() == 0:
        assert code(call(cctx, b"abc", 3, 12, XXH64, sizes, 4, ctypes.byref(got), out, 128)) == E.ZSTD_error_init_missing


def test_python_wrappers_refuse_a_bad_kind():
    with z.Compressor(1) as c:
        with pytest.raises(ValueError):
            z.piece_digests(c, b"abc", [3], kind="md5")
        with pytest.raises(z.ZstdException) as e:
            z.piece_digests(c, b"abc", [3], kind=7)
        assert e.value.code == E.ZSTD_error_parameter_outOfBound
        assert z.piece_digests(c, b"abc", [], kind="sha256") == []


# ---- the model ----
def test_model_answers():
    lib = _ffi.load()
    out = ctypes.create_string_buffer(32)
    for kind in (0, 3):
        assert code(lib.ZSTDMI_debugDigestModel(kind, b"abc", 3, out)) == E.ZSTD_error_parameter_outOfBound
    assert code(lib.ZSTDMI_debugDigestModel(XXH64, b"abc", 3, None)) == E.ZSTD_error_GENERIC
    assert code(lib.ZSTDMI_debugDigestModel(XXH64, None, 3, out)) == E.ZSTD_error_GENERIC


@pytest.mark.parametrize("kind", [XXH64, SHA256], ids=["xxh64", "sha256"])
def test_model_equals_the_oracle_and_hashlib(oracle, kind):
    base = datagen.gen("rand", 65537, 11)
    for n in list(range(301)) + [65535, 65536, 65537]:
        assert model(kind, base[:n]) == want(kind, base[:n], oracle), n
    # the same bytes from an odd address
    shifted = b"\x00" + base[:300]
    buf = ctypes.create_string_buffer(shifted, len(shifted))
    out = ctypes.create_string_buffer(32)
    assert _ffi.load().ZSTDMI_debugDigestModel(kind, ctypes.addressof(buf) + 1, 300, out) == 0
    assert out.raw[:_ffi.load().ZSTDMI_digestSize(kind)] == want(kind, base[:300], oracle)


def test_published_vectors():
    # XXH64, seed 0 (the vectors of tests/test_oracle.py)
    for text, value in ((b"", 0xEF46DB3751D8E999), (b"a", 0xD24EC4F1A98C6E5B), (b"abc", 0x44BC2CF5AD770999)):
        assert model(XXH64, text) == value.to_bytes(8, "little")
    # SHA-256 (FIPS 180-4 examples)
    for text, digest in ((b"", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"),
                         (b"abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"),
                         (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1")):
        assert model(SHA256, text) == bytes.fromhex(digest)
