"""GPU tests of ZSTDMI_DCtx_setBatchUnsized (include/zstd_mi355x.h "frames without a content size in the shared pass"): with the switch
on, an entry of ZSTDMI_decompressBatch that holds a frame without a content size takes the shared pass, and its size (or error code)
and bytes are exactly what ZSTDMI_decompressDevice gives for that entry alone on a second context with the same settings.  The
unsized frames are libzstd's (tests/golden/manifest_dict.json, known by their SHA-256), this compressor's with ZSTD_c_contentSizeFlag = 0
(checked against the original bytes) and forged ones (tests/zstd_forge.py).

Layout of every batch: all destinations are carved from one tensor filled with 0xA5, start at odd offsets and have at least 64 guard
bytes between them; everything outside the bytes an entry reports as written — for a failed entry: outside its capacity — must still
be 0xA5 afterwards.  (Nothing here is meant to fault: the decoder bounds every read and write itself.)"""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest

import datagen
import forge_cases
import zstd_forge as forge
import zstdsharp_amd as z
from zstdsharp_amd.errors import ZSTD_ErrorCode, ZstdException, get_error_code, is_error

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 200, 201
TOO_SMALL, CORRUPT, WRONG_DICT = -70, -20, -32
SET_DICTS = ("train_default_json.dict", "train_default_text.dict", "trained_16k.dict")


@functools.lru_cache(maxsize=None)
def data_of(kind, n, seed):
    return datagen.gen(kind, n, seed)


@functools.lru_cache(maxsize=None)
def dic(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def header_of(blob):
    """-> (unsized, window size or None, header bytes) of the frame a blob starts with"""
    assert blob[:4] == b"\x28\xb5\x2f\xfd"
    fhd = blob[4]
    single, fcs = (fhd >> 5) & 1, fhd >> 6
    window = None if single else (8 + (blob[5] & 7)) << (7 + (blob[5] >> 3))
    return (fcs == 0 and not single), window, 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0) if fcs == 0 else 1 << fcs)


def widen(blob, window_log=19):
    """a frame of this compressor's without a content size, its window descriptor restated as the 2^19 a streaming encoder declares
    (the compressor itself declares the smallest power of two that holds the frame): the frame's bound becomes blocks x 128 KiB"""
    unsized, window, _ = header_of(blob)
    assert unsized and window <= 1 << window_log
    return blob[:5] + bytes([(window_log - 10) << 3]) + blob[6:]


_compressors = {}


def unsized_frames(data, level=3, checksum=0, dictionary=None, single_frame=False):
    """data through this compressor with ZSTD_c_contentSizeFlag = 0 (contexts are kept for the run)"""
    key = (level, checksum, dictionary, single_frame)
    if key not in _compressors:
        c = z.Compressor(level)
        c.SetParameter(ZSTD_c_contentSizeFlag, 0)
        c.SetParameter(ZSTD_c_checksumFlag, checksum)
        if dictionary is not None:
            c.LoadDictionary(dic(dictionary))
        if single_frame:
            c.single_frame = True
        _compressors[key] = c
    blob = _compressors[key].Wrap(data)
    assert header_of(blob)[0], "the compressor wrote a content size"
    return blob


@functools.lru_cache(maxsize=None)
def fixtures():
    """the five libzstd streams without a content size -> ((blob, size, sha256), ...)"""
    import json
    man = json.load(open(os.path.join(GOLDEN, "manifest_dict.json")))
    out = tuple((open(os.path.join(GOLDEN, c["file"]), "rb").read(), c["n"], c["sha256"]) for c in man["cases"] if c.get("unsized"))
    assert len(out) == 5 and all(header_of(b)[0] for b, _, _ in out)
    return out


class Batch:
    """Sources in one tensor (shuffled order), destinations in another (0xA5, odd starts, guards of 64 bytes or more)."""

    def __init__(self, lib, blobs, caps, seed=1):
        import torch
        self.lib, self.blobs, self.n, self.caps = lib, blobs, len(blobs), list(caps)
        order = np.random.default_rng(seed).permutation(self.n)
        self.src_at = [0] * self.n
        at, parts = 3, [bytes(3)]
        for i in order:
            self.src_at[i] = at
            parts.append(blobs[i]); parts.append(bytes(5))
            at += len(blobs[i]) + 5
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).cuda()
        self.dst_at, at = [], 1
        for cap in self.caps:
            self.dst_at.append(at)
            at = (at + cap + 64) | 1
        self.dst = torch.full((at + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.got = (ctypes.c_size_t * max(self.n, 1))()
        torch.cuda.synchronize()

    def run(self, dctx):
        srcs = (ctypes.c_void_p * self.n)(*[self.src.data_ptr() + a for a in self.src_at])
        sizes = (ctypes.c_size_t * self.n)(*[len(b) for b in self.blobs])
        dsts = (ctypes.c_void_p * self.n)(*[self.dst.data_ptr() + a for a in self.dst_at])
        caps = (ctypes.c_size_t * self.n)(*self.caps)
        r = self.lib.ZSTDMI_decompressBatch(dctx, srcs, sizes, self.n, dsts, caps, self.got)
        self.host = self.dst.cpu().numpy()
        return r

    def result(self, i):
        """-> the entry's bytes, or its error code as a negative number"""
        g = self.got[i]
        if is_error(g):
            return -get_error_code(g)
        return self.host[self.dst_at[i]:self.dst_at[i] + g].tobytes()

    def assert_guards_untouched(self):
        rest = self.host.copy()
        for i in range(self.n):
            if is_error(self.got[i]):      # (a failed entry's destination holds nothing of use; beyond its capacity nothing may change)
                rest[self.dst_at[i]:self.dst_at[i] + self.caps[i]] = 0xA5
            else:
                assert self.got[i] <= self.caps[i], i
                rest[self.dst_at[i]:self.dst_at[i] + self.got[i]] = 0xA5
        bad = np.flatnonzero(rest != 0xA5)
        assert bad.size == 0, f"bytes outside the reported results were written, first at {bad[:4]}"


def single_decodes(lib, dctx, blobs, caps):
    """every blob through ZSTDMI_decompressDevice alone -> bytes, or the error code as a negative number"""
    import torch
    out = []
    room = torch.empty(max(caps) + 64, dtype=torch.uint8, device="cuda")
    for blob, cap in zip(blobs, caps):
        src = torch.from_numpy(np.frombuffer(blob or b"\0", dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        r = lib.ZSTDMI_decompressDevice(dctx, room.data_ptr(), cap, src.data_ptr(), len(blob))
        out.append(-get_error_code(r) if is_error(r) else room[:r].cpu().numpy().tobytes())
    return out


def context(lib, switch=1, overlap=0, lit=0, waves=0, long_frames=0, dictionary=None, ddict=None, ddict_set=None):
    d = z.Decompressor()
    assert lib.ZSTDMI_DCtx_setOverlap(d.dctx, overlap) == 0 and lib.ZSTDMI_DCtx_setLiteralDecoder(d.dctx, lit) == 0
    assert lib.ZSTDMI_DCtx_setExecWaves(d.dctx, waves) == 0 and lib.ZSTDMI_DCtx_setLongFrames(d.dctx, long_frames) == 0
    if dictionary is not None:
        d.LoadDictionary(dic(dictionary))
    if ddict_set is not None:
        d.SetParameter(z.ZSTD_d_refMultipleDDicts, 1)
        for dd in ddict_set:
            d.RefDDict(dd)
    if ddict is not None:
        d.RefDDict(ddict)
    assert lib.ZSTDMI_DCtx_setBatchUnsized(d.dctx, switch) == 0
    return d


def compare(lib, blobs, caps, seed, alone=0, expect=None, **settings):
    """one batch with the switch on against the single calls of a second context with the same settings -> (the batch, the single results)"""
    ref = context(lib, **settings)
    want = single_decodes(lib, ref.dctx, blobs, caps)
    d = context(lib, **settings)
    b = Batch(lib, blobs, caps, seed=seed)
    assert b.run(d.dctx) == 0
    for i in range(len(blobs)):
        got = b.result(i)
        assert got == want[i], (i, len(blobs[i]), caps[i], got if isinstance(got, int) else len(got), want[i] if isinstance(want[i], int) else len(want[i]))
        if expect is not None and expect[i] is not None:
            assert got == expect[i], (i, "differs from the known content or the expected code", got if isinstance(got, int) else len(got))
    b.assert_guards_untouched()
    assert lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == alone
    ref.Dispose(); d.Dispose()
    return b, want


@functools.lru_cache(maxsize=None)
def identity_entries():
    """-> (blobs, contents (None: known by SHA-256 only), sha256s, number of entries that hold an unsized frame)"""
    text, zipf, mixed = data_of("text", 200000, 41), data_of("zipf", 200000, 42), data_of("mixed", 200000, 43)
    import oracle_lib
    blobs, contents, shas, unsized = [], [], [], 0
    for blob, n, sha in fixtures():
        blobs.append(blob); contents.append(None); shas.append((n, sha)); unsized += 1
    sizes = [1, 2, 7, 63, 100, 255, 300, 1000, 1024, 2049, 4096, 5000, 9999, 16384, 16385, 20000, 25000, 29999, 30000, 12289]
    for i in range(40):
        n = sizes[i % 20] + (i // 20)
        pool = (text, zipf, mixed)[i % 3]
        data = pool[4000 * i:4000 * i + n]
        blob = unsized_frames(data, level=(1, 3, 5)[i % 3], checksum=1 if i % 4 == 1 else 0)
        blobs.append(widen(blob) if i % 2 else blob); contents.append(data); shas.append(None); unsized += 1
        if i % 5 == 0:          # a sized neighbour
            sized = oracle_lib.compress(pool[1000 * i:1000 * i + 3000 + i], 1, i % 2, 0)
            assert isinstance(sized, bytes) and not header_of(sized)[0]
            blobs.append(sized); contents.append(pool[1000 * i:1000 * i + 3000 + i]); shas.append(None)
    return tuple(blobs), tuple(contents), tuple(shas), unsized


def identity_caps(contents, shas):
    sizes = [len(c) if c is not None else s[0] for c, s in zip(contents, shas)]
    return [n if i % 2 == 0 else n + 1000 for i, n in enumerate(sizes)]


def check_known_contents(b, contents, shas):
    for i, (c, s) in enumerate(zip(contents, shas)):
        got = b.result(i)
        assert not isinstance(got, int), (i, got)
        if c is not None:
            assert got == c, (i, "differs from the original bytes")
        else:
            assert len(got) == s[0] and hashlib.sha256(got).hexdigest() == s[1], (i, "differs from the fixture's content")


@pytest.mark.parametrize("lit", [0, 1, 2, 3])
@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_identity(gpu_lib, overlap, lit):
    blobs, contents, shas, _ = identity_entries()
    caps = identity_caps(contents, shas)
    b, _ = compare(gpu_lib, list(blobs), caps, seed=3 + overlap, overlap=overlap, lit=lit)
    check_known_contents(b, contents, shas)


@pytest.mark.parametrize("waves,long_frames", [(1, 0), (16, 0), (0, 1), (0, 2)])
def test_identity_under_exec_settings(gpu_lib, waves, long_frames):
    blobs, contents, shas, _ = identity_entries()
    caps = identity_caps(contents, shas)
    b, _ = compare(gpu_lib, list(blobs), caps, seed=9, waves=waves, long_frames=long_frames)
    check_known_contents(b, contents, shas)


def test_the_switch(gpu_lib):
    """off: the same answers, the unsized entries alone; on, then off again: as never on; above 4 MiB compressed: alone either way"""
    blobs, contents, shas, unsized = identity_entries()
    caps = identity_caps(contents, shas)
    for d in (context(gpu_lib, switch=0), context(gpu_lib, switch=1)):
        assert gpu_lib.ZSTDMI_DCtx_setBatchUnsized(d.dctx, 0) == 0
        b = Batch(gpu_lib, list(blobs), caps, seed=5)
        assert b.run(d.dctx) == 0
        check_known_contents(b, contents, shas)
        b.assert_guards_untouched()
        assert gpu_lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == unsized
        d.Dispose()
    big = data_of("rand", (4 << 20) + 70000, 7)
    blob = unsized_frames(big, level=1)
    assert len(blob) > 4 << 20
    small = [unsized_frames(data_of("text", 3000, 60 + k)) for k in range(3)]
    compare(gpu_lib, [small[0], blob, small[1], small[2]], [3000, len(big), 3000, 3000], seed=6, alone=1,
            expect=[data_of("text", 3000, 60), big, data_of("text", 3000, 61), data_of("text", 3000, 62)])


def raw_frame(data):
    """one forged frame without a content size: the bytes stored raw"""
    blob, content = forge.frame([{"t": "raw", "data": data}], single=False, window=(7 << 3))
    assert content == data and header_of(blob)[0]
    return blob


@functools.lru_cache(maxsize=None)
def zipf_symbols(n, seed):
    """n bytes over 16 symbols with a skewed distribution whose Huffman weights are exact powers of two"""
    rng = np.random.default_rng(seed)
    p = np.array([1 / 2, 1 / 4, 1 / 8, 1 / 16] + [1 / 64] * 4, dtype=np.float64)
    return bytes(rng.choice(8, size=n, p=p / p.sum()).astype(np.uint8))


def huf_frame(data, sized):
    """one forged frame of one compressed block without sequences: Huffman-coded literals only, over the symbols 0 .. 7 with the
    weights 6 5 4 3 1 1 1 1 (32 + 16 + 8 + 4 + 4 x 1 = 64: a complete code)"""
    w = [6, 5, 4, 3, 1, 1, 1, 1]
    blk = {"t": "c", "lit": {"k": "huf", "data": data, "w": w, "streams": 4}, "seqs": []}
    if sized:
        blob, content = forge.frame([blk])
    else:
        blob, content = forge.frame([blk], single=False, window=(7 << 3))
    assert content == data and header_of(blob)[0] == (not sized)
    return blob


def sized_raw_frame(data):
    blob, content = forge.frame([{"t": "raw", "data": data}])
    assert content == data and not header_of(blob)[0]
    return blob


SKIP = forge.skippable(3, b"between two frames")


@functools.lru_cache(maxsize=None)
def several_frame_entries():
    """-> ((blob, content), ...): the orders [unsized, sized], [sized, unsized], [unsized, unsized, sized] with a skippable frame
    between two of the frames; the frame behind the unsized one is sequence-free (stored raw, or Huffman literals only): the block
    the early literal decoder would write in place.  And one entry of 70 unsized frames of 100 bytes."""
    rnd = data_of("rand", 4000, 3)
    text = data_of("text", 40000, 4)
    zs = zipf_symbols(3000, 5)
    u1 = unsized_frames(text[:7000], level=1); u2 = widen(unsized_frames(text[7000:9500], level=3)); u3 = unsized_frames(zs + text[:100], level=1)
    out = []
    for tail, tail_content in ((sized_raw_frame(rnd[:1500]), rnd[:1500]), (huf_frame(zs, True), zs)):
        out.append((u1 + SKIP + tail, text[:7000] + tail_content))
        out.append((u2 + tail, text[7000:9500] + tail_content))
        out.append((tail + SKIP + u1, tail_content + text[:7000]))
        out.append((tail + u2, tail_content + text[7000:9500]))
        out.append((u1 + u2 + SKIP + tail, text[:7000] + text[7000:9500] + tail_content))
        out.append((u3 + SKIP + u2 + tail, zs + text[:100] + text[7000:9500] + tail_content))
    # unsized forged frames behind unsized ones: raw and Huffman-only, without a content size themselves
    out.append((u2 + raw_frame(rnd[:999]) + huf_frame(zs[:2000], False), text[7000:9500] + rnd[:999] + zs[:2000]))
    out.append((huf_frame(zs[:1200], False) + SKIP + huf_frame(zs[100:1500], True), zs[:1200] + zs[100:1500]))
    seventy = b"".join(unsized_frames(text[100 * k:100 * k + 100], level=1) for k in range(70))
    out.append((seventy, text[:7000]))
    out.append((seventy + b"\x00", None))            # one trailing byte: srcSize_wrong
    return tuple(out)


@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_several_frames_per_entry(gpu_lib, overlap):
    entries = several_frame_entries()
    blobs = [b for b, _ in entries]
    expect = [c if c is not None else -72 for _, c in entries]
    caps = [(len(c) if c is not None else 7000) + (i % 2) * 37 for i, (_, c) in enumerate(entries)]
    compare(gpu_lib, blobs, caps, seed=11, expect=expect, overlap=overlap)


def test_capacities(gpu_lib):
    """exact - 1, 0, below the entry's Huffman-coded literals, between the regenerated size and the bound — among good neighbours"""
    text = data_of("text", 40000, 8)
    zipf = data_of("zipf", 30000, 9)
    one = widen(unsized_frames(zipf[:20000], level=1))              # one frame, mostly Huffman-coded literals; its bound is 128 KiB
    entries = several_frame_entries()
    three, three_content = entries[4]
    huf3, huf3_content = entries[11]
    good = unsized_frames(text[:5000])
    blobs, caps, expect = [], [], []
    for blob, content in ((one, zipf[:20000]), (three, three_content), (huf3, huf3_content)):
        n = len(content)
        for cap in (n - 1, 0, 1000, n // 2, n, n + 1, n + 70000):
            blobs += [good, blob]; caps += [5000, cap]; expect += [text[:5000], content if cap >= n else TOO_SMALL]
    blobs.append(good); caps.append(5000); expect.append(text[:5000])
    assert header_of(one)[1] >= 1 << 17 and 20000 + 70000 < 1 << 17          # (between the size and the bound)
    for overlap in (0, 2):
        compare(gpu_lib, blobs, caps, seed=12, expect=expect, overlap=overlap)


def frame_header_size(blob):
    return header_of(blob)[2]


def test_errors_among_good_entries(gpu_lib):
    """the eight kinds of damage of test_gpu_batch.py::test_damage_among_good_entries on unsized entries, the forged frames that
    regenerate more than their bound, and a damaged block in an entry whose capacity is too small as well: every damaged entry
    answers with the single call's code, every good one is restored exactly"""
    rng = np.random.default_rng(31)
    pool = {k: data_of(k, 1 << 18, 77) for k in ("text", "zipf", "mixed")}
    entries = []
    for i in range(44):
        n = int(rng.integers(2000, 30000)); at = int(rng.integers(0, (1 << 18) - n))
        entries.append(pool[("text", "zipf", "mixed")[i % 3]][at:at + n])
    blobs = [unsized_frames(e, level=(1, 3)[i % 2], checksum=1 if i % 4 == 3 else 0) for i, e in enumerate(entries)]
    blobs = [widen(b) if i % 3 == 0 else b for i, b in enumerate(blobs)]
    caps = [len(e) for e in entries]
    expect = list(entries)
    blobs[2] = blobs[2][:-1]                                         # cut by one byte
    blobs[5] = blobs[5][:5]                                          # cut inside the header
    blobs[8] = b"\x00\x01\x02\x03" + blobs[8][4:]                    # magic overwritten
    assert blobs[11][4] & 4                                          # (a checksummed frame)
    flip = bytearray(blobs[11]); flip[len(flip) // 2] ^= 0x10; blobs[11] = bytes(flip)      # a byte flipped in its middle
    flip = bytearray(blobs[14]); flip[frame_header_size(blobs[14])] ^= 0x06; blobs[14] = bytes(flip)     # the first block header: another block type
    blobs[17] = blobs[17] + b"\x00"                                   # one trailing byte
    caps[20] -= 1                                                    # capacity = content - 1
    blobs[23] = unsized_frames(entries[23], dictionary="trained_16k.dict")      # names a dictID, none loaded
    expect[23] = WRONG_DICT; expect[20] = TOO_SMALL; expect[17] = -72; expect[8] = -10
    for i in (2, 5, 11, 14):
        expect[i] = None            # (the single call names the code)
    above = [c for c in forge_cases.load_manifest()["cases"] if c["name"].startswith("neg_unsized_")]
    assert len(above) == 4
    for k, c in enumerate(above):                                   # frames that regenerate more than their bound
        blobs[26 + 3 * k] = c["blob"]; caps[26 + 3 * k] = c["cap"]; expect[26 + 3 * k] = CORRUPT
    # a damaged block AND a capacity that is too small: the block's error wins, as in the single call
    flip = bytearray(blobs[38]); flip[frame_header_size(blobs[38])] ^= 0x06; blobs[38] = bytes(flip); caps[38] -= 100; expect[38] = None
    blobs[41] = blobs[41][:-1]; caps[41] = 10; expect[41] = None
    # (the same with an error that only the block stages find: the literals section restated as treeless, with no table in front of it)
    at = frame_header_size(blobs[40])
    assert (blobs[40][at] >> 1) & 3 == 2 and blobs[40][at + 3] & 3 == 2, "entry 40 does not begin with Huffman-coded literals"
    flip = bytearray(blobs[40]); flip[at + 3] |= 3; blobs[40] = bytes(flip); caps[40] -= 100; expect[40] = None
    b, want = compare(gpu_lib, blobs, caps, seed=15, expect=expect)
    damaged = (2, 5, 8, 11, 14, 17, 20, 23, 26, 29, 32, 35, 38, 40, 41)
    for i in range(44):
        assert isinstance(want[i], int) == (i in damaged), (i, want[i] if isinstance(want[i], int) else len(want[i]))
    assert want[38] != TOO_SMALL and want[40] != TOO_SMALL and want[41] != TOO_SMALL


def test_dictionaries(gpu_lib):
    text = data_of("text", 120000, 500)
    records = [text[2500 * i:2500 * i + (300, 777, 1500, 4096, 2049, 3333)[i % 6]] for i in range(30)]
    blobs = [unsized_frames(r, level=(1, 3)[i % 2], dictionary="trained_16k.dict") for i, r in enumerate(records)]
    blobs = [widen(b) if i % 2 else b for i, b in enumerate(blobs)]
    assert all(z.get_dict_id_from_frame(b) == z.get_dict_id_from_dict(dic("trained_16k.dict")) for b in blobs)
    caps = [len(r) + (i % 3) * 500 for i, r in enumerate(records)]
    compare(gpu_lib, blobs, caps, seed=21, expect=records, dictionary="trained_16k.dict")
    dd = z.DDict(dic("trained_16k.dict"))
    compare(gpu_lib, blobs, caps, seed=22, expect=records, ddict=dd)
    dd.Dispose()


def test_ddict_set(gpu_lib):
    """record i behind dictionary i mod 3 of a set (ZSTD_d_refMultipleDDicts); a dictID that is not in the set fails alone"""
    text = data_of("text", 120000, 501)
    records = [text[2500 * i:2500 * i + (300, 777, 1500, 4096, 2049, 3333)[i % 6]] for i in range(30)]
    blobs = [unsized_frames(r, level=(1, 3)[(i // 3) % 2], dictionary=SET_DICTS[i % 3]) for i, r in enumerate(records)]
    blobs = [widen(b) if i % 2 else b for i, b in enumerate(blobs)]
    expect = list(records)
    blobs[13] = unsized_frames(records[13], dictionary="train_default_zipf.dict"); expect[13] = WRONG_DICT
    # a forged frame of five blocks without a dictID (the current DDict's): more blocks than frames, so block_link's set instance runs too
    five, five_content = next(c[2] for c in forge_cases.CASES if c[0] == "huf_treeless_gap_s4")()
    blobs.append(five); expect.append(five_content)
    caps = [len(r) for r in records] + [len(five_content)]
    dds = [z.DDict(dic(name)) for name in SET_DICTS]
    ref = context(gpu_lib, ddict_set=dds)
    want = single_decodes(gpu_lib, ref.dctx, blobs, caps)
    d = context(gpu_lib, ddict_set=dds)
    b = Batch(gpu_lib, blobs, caps, seed=23)
    assert b.run(d.dctx) == 0
    for i in range(31):
        assert b.result(i) == want[i] == expect[i], i
    b.assert_guards_untouched()
    assert gpu_lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == 0
    assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 29           # (every record but the one whose dictionary is not in the set)
    ref.Dispose(); d.Dispose()
    for dd in dds:
        dd.Dispose()


@pytest.mark.parametrize("long_frames", [2, 1])
def test_long_frame(gpu_lib, long_frames):
    text = data_of("text", 2 << 20, 71)
    long_blob = unsized_frames(text, level=3, single_frame=True)
    assert forge_cases.all_sized(long_blob) is False
    small = [data_of("zipf", 500 + 97 * k, 80 + k) for k in range(20)]
    blobs = [unsized_frames(s, level=1) for s in small]
    blobs.insert(7, long_blob)
    contents = list(small); contents.insert(7, text)
    compare(gpu_lib, blobs, [len(c) for c in contents], seed=31, expect=contents, long_frames=long_frames)


def test_ranges(gpu_lib):
    """a pack written without content sizes, read by unwrap_ranges: the same bytes with the switch off and on, and with it on the
    entries are in the shared pass's lists"""
    rng = np.random.default_rng(17)
    pool = data_of("mixed", 1 << 20, 88)
    sizes = [100, 200000, 333, 4096, 65536, 65537, 1000, 150000] + [int(rng.integers(100, 40000)) for _ in range(32)]
    entries = [pool[(7919 * i) % 500000:(7919 * i) % 500000 + n] for i, n in enumerate(sizes)]
    with z.Compressor(3) as c:
        c.SetParameter(ZSTD_c_contentSizeFlag, 0)
        pack = z.compress_pack(c, entries)
    whole = b"".join(entries)
    starts = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    plans = {
        "whole entries": [(starts[i], sizes[i]) for i in (0, 1, 5, 17, 39)],
        "cutting frames": [(starts[1] + 5, 100000), (starts[5] - 3, 70), (starts[7] + 140000, 20000), (starts[30] + 1, 10), (3, 50)],
        "the whole stream": [(0, len(whole))],
    }
    for name, ranges in plans.items():
        got = {}
        for switch in (0, 1):
            with z.Decompressor() as d:
                d.batch_unsized = bool(switch)
                got[switch] = [bytes(x) for x in d.unwrap_ranges(pack, ranges)]
                # ZSTDMI_debugLastRangesAlone counts RANGES handed to the single-range path, with the switch off too (an entry decoded
                # alone "does not make its ranges go alone": tests/test_gpu_ranges.py pins that), so it cannot tell the two paths apart.
                # The workspace can: with the switch off every entry here is left to the single-call path and the shared pass asks for
                # no lists at all; with it on the entries are in its lists.
                assert gpu_lib.ZSTDMI_debugLastRangesAlone(d.dctx) == 0, (name, switch)
                ws = gpu_lib.ZSTDMI_debugLastBatchWorkspace(d.dctx)
                assert (ws > 0) if switch else (ws == 0), (name, switch, ws)
                if name == "cutting frames":
                    o, l = ranges[0]
                    assert bytes(d.unwrap_range(pack, o, l)) == whole[o:o + l], (name, switch)
        assert got[0] == got[1] == [whole[o:o + l] for o, l in ranges], name


def test_workspace(gpu_lib):
    """4096 records of 200 to 300 bytes whose frames declare a window of 2^19, capacities exact: the literal scratch is sized by the
    capacities, not by the frames' bounds of 128 KiB each (a condition: below n x 8 KiB where the bounds come to n x 128 KiB)"""
    text = data_of("text", 1 << 20, 99)
    n = 4096
    records = [text[251 * i:251 * i + 200 + (i * 37) % 101] for i in range(n)]
    with z.Compressor(3) as c:
        c.SetParameter(ZSTD_c_contentSizeFlag, 0)
        blobs = [widen(b) for b in z.compress_batch(c, records)]
    for b in blobs:
        unsized, window, _ = header_of(b)
        assert unsized and window >= 1 << 17
    d = context(gpu_lib)
    b = Batch(gpu_lib, blobs, [len(r) for r in records], seed=41)
    assert b.run(d.dctx) == 0
    for i in range(n):
        assert b.result(i) == records[i], i
    b.assert_guards_untouched()
    assert gpu_lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == 0
    ws = gpu_lib.ZSTDMI_debugLastBatchWorkspace(d.dctx)
    print(f"workspace asked for {n} entries: {ws} bytes ({ws / n:.0f} per entry)")
    assert 0 < ws < 32 << 20, ws
    d.Dispose()


def test_python(gpu_lib):
    import torch
    items = [data_of("text", 3000, 1), data_of("zipf", 20000, 2), data_of("mixed", 9000, 3), b"x"]
    blobs = [unsized_frames(e) for e in items]
    with z.Decompressor() as d:
        d.batch_unsized = True
        assert z.decompress_batch(d, blobs, [len(e) for e in items]) == items
        assert gpu_lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == 0
        tensors = [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() for b in blobs]
        back = z.decompress_batch(d, tensors, [len(e) + 7 for e in items])
        assert [t.cpu().numpy().tobytes() for t in back] == items
        assert gpu_lib.ZSTDMI_debugLastBatchAloneD(d.dctx) == 0
        with pytest.raises(ZstdException) as err:
            z.decompress_batch(d, blobs, [len(items[0]), len(items[1]) - 1, len(items[2]), 1])
        assert "item 1" in str(err.value) and err.value.Code == ZSTD_ErrorCode.ZSTD_error_dstSize_tooSmall
