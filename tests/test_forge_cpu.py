"""Forged frames on the CPU: the committed fixtures (tests/golden/forge_*.zst) against the oracle decoder and against the forge
that explains them (tests/zstd_forge.py + tests/forge_cases.py).  No GPU, no libzstd: the verdicts of libzstd were recorded by
tests/golden/make_golden_forge.py.  tests/test_gpu_forge.py is the GPU side."""
import ctypes
import hashlib

import pytest

import forge_cases
import zstd_forge as F


@pytest.fixture(scope="module")
def manifest():
    return forge_cases.load_manifest()


def _result(got):
    return ("reject",) if isinstance(got, int) else ("bytes", len(got), hashlib.sha256(got).hexdigest())


def test_oracle_matches_its_recorded_verdict(oracle, manifest):
    for c in manifest["cases"]:
        got = oracle.decompress(c["blob"], c["cap"])
        v = c["oracle"]
        if v.startswith("rejected"):
            assert got == -int(v.split(":")[1]), c["name"]
        elif v == "equal":
            assert _result(got) == ("bytes", c["size"], c["sha256"]), c["name"]
        else:
            assert _result(got) == ("bytes", int(v.split(":")[1]), v.split(":")[2]), c["name"]
        if c["agreed"]:
            assert _result(got) == c["expect"], c["name"]


def test_forge_regenerates_every_fixture(manifest):
    """the committed files are exactly what the case descriptions say, and their content what the forge's executor makes of them"""
    by_name = {c["name"]: c for c in manifest["cases"]}
    assert list(by_name) == [c[0] for c in forge_cases.CASES]
    for name, tags, build, valid in forge_cases.CASES:
        blob, content = build()
        c = by_name[name]
        assert blob == c["blob"] and tags == c["tags"] and valid == c["valid"], name
        if valid:
            assert (len(content), hashlib.sha256(content).hexdigest()) == (c["size"], c["sha256"]), name
        else:
            assert content is None and c["sha256"] is None


def test_every_tag_has_an_agreed_case(manifest):
    assert manifest["tags"] == forge_cases.TAGS
    for tag in forge_cases.TAGS:
        assert any(c["agreed"] and tag in c["tags"] for c in manifest["cases"]), tag
    # "agreed" is what the generator's rule says, not a flag set by hand
    for c in manifest["cases"]:
        every = list(c["libzstd"].values()) + [c["oracle"]]
        assert len(c["libzstd"]) == 2
        assert c["agreed"] == (all(v == "equal" for v in every) if c["valid"] else all(v.startswith("rejected") for v in every)), c["name"]
    sizes = {c["file"]: c["csize"] for c in manifest["cases"]}
    assert sum(sizes.values()) < (1 << 20)


def _first_compressed_block(blob):
    """(offset of the block's content, its size) of the first compressed block of a one-frame blob — by the frame's own header fields"""
    fhd = blob[4]
    at = 5 + (0 if fhd & 0x20 else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if fhd & 0x20 else 0), 2, 4, 8)[fhd >> 6]
    while True:
        h = int.from_bytes(blob[at:at + 3], "little")
        btype, size = (h >> 1) & 3, h >> 3
        if btype == 2:
            return at + 3, size
        at += 3 + (1 if btype == 1 else size)


def test_cases_reach_the_paths_they_are_named_for(oracle, manifest):
    """What the summary claims is read back from the fixtures' own bytes: the Huffman table log through the oracle's
    HUF_readStats, the weight form from the header byte, the nbSeq form from the sequences header."""
    by_name = {c["name"]: c for c in manifest["cases"]}
    lib = oracle.lib()

    def huf_stats(name):
        blob = by_name[name]["blob"]
        at, size = _first_compressed_block(blob)
        lh = int.from_bytes(blob[at:at + 5], "little")
        assert lh & 3 == 2, name
        lhsize = (3, 3, 4, 5)[(lh >> 2) & 3]
        weights = ctypes.create_string_buffer(256)
        nsym, log = ctypes.c_uint32(0), ctypes.c_uint32(0)
        ranks = (ctypes.c_uint32 * 16)()
        src = blob[at + lhsize:at + size]
        r = lib.zso_huf_readStats(weights, ctypes.byref(nsym), ctypes.byref(log), ranks, src, len(src))
        assert not oracle.is_error(r), name
        return log.value, nsym.value, src[0]
    for n, s in ((300, 1), (1023, 1), (300, 4), (5000, 4)):
        assert huf_stats(f"huf_log12_{n}_s{s}")[0] == 12         # decode_lit.hip: tl12, huf_decode_stream<true>
        assert huf_stats(f"huf_log11_{n}_s{s}")[0] == 11         # the compact table's `pairs` form (tableLog > 10)
        assert huf_stats(f"huf_log10_{n}_s{s}")[0] == 10
        assert huf_stats(f"huf_log1_{n}_s{s}")[:2] == (1, 2)
    # direct weights (header byte >= 128): 1, 2, 3 and 128 stored weights
    assert [huf_stats(n)[2] for n in ("huf_direct_2sym_odd", "huf_direct_2sym_even", "huf_direct_3sym_odd", "huf_direct_128")] == [128, 129, 130, 255]
    assert huf_stats("huf_direct_128")[:2] == (8, 129)
    log, nsym, head = huf_stats("huf_fse_255")
    assert head < 128 and nsym == 256 and log == 9
    # the nbSeq forms: RLE literals (2-byte header below 4096 literals, 3-byte from there), then the count
    for name, n, form in (("nbseq_127", 127, 1), ("nbseq_128", 128, 2), ("nbseq_255", 255, 2), ("nbseq_127_in_2_bytes", 127, 2),
                          ("nbseq_32511", 0x7EFF, 2), ("nbseq_32512", 0x7F00, 3), ("nbseq_32513", 0x7F01, 3), ("nbseq_32768", 32768, 3)):
        blob = by_name[name]["blob"]
        at, size = _first_compressed_block(blob)
        assert blob[at] & 3 == 1
        p = at + (2 if n < 4096 else 3) + 1
        b0 = blob[p]
        if form == 1:
            assert b0 == n
        elif form == 2:
            assert 128 <= b0 < 255 and ((b0 - 128) << 8) + blob[p + 1] == n
        else:
            assert b0 == 255 and int.from_bytes(blob[p + 1:p + 3], "little") + 0x7F00 == n      # block_parse_kernel's 0xFF form
    # all three tables RLE and no extra bits: the whole bitstream is the end mark
    for n in (1, 64, 200):
        blob = by_name[f"seq_zero_bits_{n}"]["blob"]
        at, size = _first_compressed_block(blob)
        assert blob[at + size - 1] == 1 and blob[at + size - 5] == 0x54         # modes byte: RLE, RLE, RLE


def test_executor_on_the_formats_own_repeat_offset_rules():
    """the executor is the reference of the forged tests; its repeat-offset rules, case by case (RFC 8878 3.1.1.5)"""
    rep = [10, 20, 30]
    assert F.rep_step(rep, 5, 1) == (10, [10, 20, 30])
    assert F.rep_step(rep, 5, 2) == (20, [20, 10, 30])
    assert F.rep_step(rep, 5, 3) == (30, [30, 10, 20])
    assert F.rep_step(rep, 0, 1) == (20, [20, 10, 30])
    assert F.rep_step(rep, 0, 2) == (30, [30, 10, 20])
    assert F.rep_step(rep, 0, 3) == (9, [9, 10, 20])
    assert F.rep_step(rep, 0, 43) == (40, [40, 10, 20]) and F.rep_step(rep, 7, 4) == (1, [1, 10, 20])
    with pytest.raises(F.ForgeInvalid):
        F.rep_step([1, 4, 8], 0, 3)
    # "abc", then literal X and 5 bytes from 3 back (b c X b c), then no literals and offset_value 1: the SECOND repeat offset (the
    # frame's start value 1), 2 bytes; the last literal; an RLE block
    assert F.execute([{"t": "raw", "data": b"abc"}, {"t": "c", "lit": {"k": "raw", "data": b"XY"}, "seqs": [(1, 3 + 3, 5), (0, 1, 2)]},
                      {"t": "rle", "byte": 0x2E, "size": 3}]) == b"abcX" + b"bcXbc" + b"cc" + b"Y" + b"..."


def test_random_frames_decode_under_the_oracle(oracle):
    """200 seeded frames of 1 to 4 blocks: modes, table logs, Huffman weights and repeat offsets drawn at random"""
    for seed in range(200):
        blob, content = forge_cases.random_frame(1000 + seed)
        assert len(content) <= 8192
        assert oracle.decompress(blob, len(content)) == content, seed


def test_host_frame_walk_agrees_with_the_oracle(oracle, manifest):
    """ZSTD_decompressBound / ZSTD_findFrameCompressedSize of the product never touch a kernel: on every forged fixture, and on
    every truncation of the small ones, they answer what the oracle answers.  (A skippable frame's header of 5 to 7 bytes was
    prefix_unknown instead of srcSize_wrong: ZSTD_decompressStream, fed in small pieces, gave up on such a stream.)"""
    from zstdsharp_amd import _ffi
    from zstdsharp_amd.errors import get_error_code, is_error
    lib, o = _ffi.load(), oracle.lib()
    o.zso_decompressBound.restype = ctypes.c_uint64
    for c in manifest["cases"]:
        blob = c["blob"]
        cuts = range(len(blob) + 1) if len(blob) <= 200 else [len(blob)]
        for n in cuts:
            part = blob[:n]
            assert lib.ZSTD_decompressBound(part, n) == o.zso_decompressBound(part, n), (c["name"], n)
            got, want = lib.ZSTD_findFrameCompressedSize(part, n), o.zso_findFrameCompressedSize(part, n)
            if oracle.is_error(want):
                assert is_error(got) and int(get_error_code(got)) == oracle.err_code(want), (c["name"], n)
            else:
                assert got == want, (c["name"], n)
