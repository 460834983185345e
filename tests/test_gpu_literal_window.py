"""GPU tests (run with -m gpu on an MI355X): the serial literal decoders (modes 1 and 3, and whatever mode 0 picks) after the
change of their inner loop (decode_lit.hip, huf_decode_stream_fs): groups of 64 symbols that stay clear of the stream's
start run in a steady form, which goes on looking up from the registers of the step before while the window is re-based, the
rest in the general form.  One-block frames are forged on the CPU (tests/zstd_forge.py) with Huffman table logs 1, 5, 10 and 11 and
literal counts 300 .. 65 536, each once without sequences (decoded in place, transposed stores) and once with (literal scratch);
the symbols are drawn evenly over the alphabet, so that at logs 10 and 11 most codes are of the longest lengths — the case the
window's width is proved for.  The oracle decodes every frame first.  Every input is built once per module and only read."""
import random

import numpy as np
import pytest

import forge_cases as C
import zstd_forge as F
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error
from test_gpu_literal_lookahead import literal_streams, reframe

pytestmark = pytest.mark.gpu

LOGS = (1, 5, 10, 11)
COUNTS = (300, 1023, 4096, 5000, 65536)


def forged(log, n, with_seqs, seed):
    w = C.skewed_weights(log, 40 if log >= 10 else 12, seed) if log > 1 else [1, 1]
    assert F.huf_table_log(w) == log
    r = random.Random(seed * 1000 + n)
    syms = [s for s, x in enumerate(w) if x]
    data = bytes(r.choices(syms, k=n))
    seqs = [(n // 3, 4 + 3, 9), (n // 3, 1, 5)] if with_seqs else []
    frame, content = C.frame([C.cblock({"k": "huf", "data": data, "w": w, "enc": "direct" if log != 10 else "fse", "streams": 4}, seqs)])
    assert content is not None
    return frame, content


@pytest.fixture(scope="module")
def frames(oracle):
    out = []
    for log in LOGS:
        for n in COUNTS:
            for with_seqs in (False, True):
                f, content = forged(log, n, with_seqs, 3 + log)
                assert oracle.decompress(f, len(content)) == content, (log, n, with_seqs)
                out.append((f, content))
    return b"".join(f for f, _ in out), b"".join(c for _, c in out), len(out)


def test_frames_are_what_they_are_meant_to_be(frames, oracle):
    """CPU side: 40 frames; the largest literal sections have four streams of 16 384 symbols, long enough for hundreds of steady
    groups, the smallest (75 symbols a stream at log 1: 10 bytes) go to the plain bit reader"""
    blob, want, count = frames
    assert count == len(LOGS) * len(COUNTS) * 2 == 40
    f, content = forged(11, 65536, False, 3 + 11)
    sizes = literal_streams(f)[3]
    assert min(sizes) > 16384 * 7 // 8 and len(content) == 65536                # more than 7 bits a symbol on average: long codes dominate
    f, _ = forged(1, 300, False, 3 + 1)
    assert max(literal_streams(f)[3]) < 16


def decode(gpu_lib, blob, total, mode):
    import torch
    src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, mode) == 0
        r = gpu_lib.ZSTDMI_decompressDevice(d.dctx, out.data_ptr(), total, src.data_ptr(), len(blob))
        assert not is_error(r) and r == total, (r, get_error_code(r))
    return out.cpu().numpy()


@pytest.mark.parametrize("mode", [0, 1, 3], ids=["default", "serial", "compact"])
def test_forged_frames_bit_exact(gpu_lib, frames, mode):
    blob, want, _ = frames
    got = decode(gpu_lib, blob, len(want), mode)
    assert got[:len(want)].tobytes() == want and not got[len(want):].any()


@pytest.mark.parametrize("mode", [1, 3], ids=["serial", "compact"])
def test_two_calls_give_the_same_bytes(gpu_lib, frames, mode):
    blob, want, _ = frames
    a = decode(gpu_lib, blob, len(want), mode)
    b = decode(gpu_lib, blob, len(want), mode)
    assert np.array_equal(a, b)


@pytest.fixture(scope="module")
def damaged(oracle):
    import datagen
    src = datagen.zipf_bytes(1 << 20, 5)
    out = {}
    for n in (2000, 65536):
        data = src[:n].tobytes()
        frame = oracle.compress(data, 1, 0, 0)
        assert reframe(frame) == frame and oracle.decompress(frame, n) == data
        at, lh, tree, sizes = literal_streams(frame)
        section = lh + tree + 6 + sum(sizes)
        out[n] = {"jump_table_exceeds_section": reframe(frame, patch=(lh + tree, b"\xff\xff")),
                  "stream_cut_by_one_byte": reframe(frame, cut=1),
                  "last_byte_zero": reframe(frame, patch=(section - 1, b"\0"))}
        for name, f in out[n].items():
            assert f != frame and isinstance(oracle.decompress(f, n), int), (n, name)
    return out


@pytest.mark.parametrize("mode", [1, 3], ids=["serial", "compact"])
@pytest.mark.parametrize("case", ["jump_table_exceeds_section", "last_byte_zero", "stream_cut_by_one_byte"])
def test_damaged_sections_are_corruption(gpu_lib, damaged, case, mode):
    assert ZSTD_ErrorCode.ZSTD_error_corruption_detected == 20
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, mode) == 0
        for n in (2000, 65536):
            with pytest.raises(ZstdException) as e:
                d.Unwrap(damaged[n][case], bytearray(n))
            assert int(e.value.Code) == 20, (case, n, mode, int(e.value.Code))
