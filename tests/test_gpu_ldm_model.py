"""The exact GPU check of the long-distance stage (zstdsharp_amd/csrc/ldm.hip): every case of tests/ldm_cases.py through the kernels
and through the serial model tests/ldm_model.py, compared for equality in this order (the first difference is reported with its
index, what the kernels gave and what the model wants):

  1. the splits ZSTDMI_debugLdmPass returns against the model's: their count, then their positions
  2. (mStart, mLen, mOff) per split against the model's
  3. F = the finder's sequences per block (a call with ZSTDMI_debugLdmSkipMerge on), M = the merged ones (a call with it off), both
     replayed into (start, length, distance) triples and the block's bytes: M must equal ldm_model.merge(F, L), the bytes the source
  4. both streams decode under the oracle's decoder and the GPU's
  5. the whole table again in reverse order on the same context repeats the first run: the workspace is reused

One context serves every case, so what an earlier case left in the workspace is what a later one runs over."""
import ctypes

import pytest

import ldm_cases
import ldm_model as lm
import oracle_lib
import zstdsharp_amd as z
from zstdsharp_amd import _ffi
from zstdsharp_amd.compressor import (ZSTD_c_enableLongDistanceMatching, ZSTD_c_ldmBucketSizeLog, ZSTD_c_ldmHashLog, ZSTD_c_ldmHashRateLog,
                                      ZSTD_c_ldmMinMatch, ZSTD_ps_enable)

pytestmark = pytest.mark.gpu

ZSTD_c_windowLog = 101
CASES = ldm_cases.cases()
_expected, _first_run = {}, {}


def expected(c):
    """the model's answer for a case, computed once"""
    if c["name"] not in _expected:
        lay, p, buf = ldm_cases.framing(c)
        S, M, _ = lm.stage(buf, lay, p)
        _expected[c["name"]] = (lay, p, buf, S, M)
    return _expected[c["name"]]


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    with z.Compressor(1) as c:
        yield c


def configure(lib, c, case):
    c.Level = case["level"]
    c.SetParameter(ZSTD_c_enableLongDistanceMatching, ZSTD_ps_enable)
    c.SetParameter(ZSTD_c_windowLog, case["wlog"])
    for k, v in ((ZSTD_c_ldmMinMatch, "mm"), (ZSTD_c_ldmHashLog, "hlog"), (ZSTD_c_ldmBucketSizeLog, "blog"), (ZSTD_c_ldmHashRateLog, "hrl")):
        c.SetParameter(k, case[v])
    assert lib.ZSTDMI_CCtx_setHistory(c.cctx, -1 if case["history"] is None else case["history"], 0) == 0
    assert lib.ZSTDMI_CCtx_setPassChunks(c.cctx, case["pass_chunks"] or 16384) == 0
    c.single_frame = case["sliding"]
    c.sliding_ldm = case["sliding"]


def compress(lib, c, case, skip_merge):
    assert lib.ZSTDMI_debugLdmSkipMerge(c.cctx, 1 if skip_merge else 0) == 0
    try:
        if case["prefix"]:
            c.RefPrefix(case["prefix"])
        return c.Wrap(case["data"])
    finally:
        assert lib.ZSTDMI_debugLdmSkipMerge(c.cctx, 0) == 0


def ldm_pass(lib, c):
    n, base, vlo = ctypes.c_size_t(), ctypes.c_uint(), ctypes.c_uint()
    assert lib.ZSTDMI_debugLdmPass(c.cctx, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(base), ctypes.byref(vlo)) == 0
    k = n.value
    cols = [(ctypes.c_uint * max(k, 1))() for _ in range(4)]
    assert lib.ZSTDMI_debugLdmPass(c.cctx, cols[0], cols[1], cols[2], cols[3], k, ctypes.byref(n), ctypes.byref(base), ctypes.byref(vlo)) == 0
    assert n.value == k
    pos, ms, ml, mo = (list(col[:k]) for col in cols)
    return pos, list(zip(ms, ml, mo)), base.value, vlo.value


def chunk(lib, c, idx):
    seqs = (_ffi.ZSTDMI_Seq * 16384)()
    lits = ctypes.create_string_buffer(65536)
    ns, ls = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.ZSTDMI_debugGetChunk(c.cctx, idx, seqs, 16384, ctypes.byref(ns), lits, 65536, ctypes.byref(ls)) == 0
    return [(seqs[i].offBase, seqs[i].litLength, seqs[i].mlBase) for i in range(ns.value)], lits.raw[:ls.value]


def replay(seqs, lits, prior, n, rep):
    """a block's store as the decoder executes it (seq_encode leaves the repcodes resolved in it) -> [(start, length, distance)],
    the block's bytes"""
    out, rep, lp, base, tri = bytearray(prior), list(rep), 0, len(prior), []
    for ob, ll, mlb in seqs:
        out += lits[lp:lp + ll]; lp += ll
        if ob > 3:
            off = ob - 3; rep = [off, rep[0], rep[1]]
        else:
            idx = ob - 1 + (1 if ll == 0 else 0)
            if idx == 0:
                off = rep[0]
            else:
                off = rep[0] - 1 if idx == 3 else rep[idx]
                rep = [off, rep[0], rep[1]] if idx != 1 else [off, rep[0], rep[2]]
        assert 1 <= off <= len(out), "an offset of %d at %d" % (off, len(out) - base)
        tri.append((len(out) - base, mlb + 3, off))
        if off >= mlb + 3:
            out += out[len(out) - off:len(out) - off + mlb + 3]
        else:
            for _ in range(mlb + 3):
                out.append(out[-off])
    out += lits[lp:]
    assert len(out) == base + n, "the block replays to %d bytes, not %d" % (len(out) - base, n)
    return tri, bytes(out[base:])


def blocks_of(lay):
    return [(b, min(b + lay.chunk, lay.n)) for b in range(lay.base, lay.n, lay.chunk)]


def stores(lib, c, case, lay, buf):
    """[(triples, literal bytes)] of the last pass's blocks"""
    out = []
    for i, (bS, bE) in enumerate(blocks_of(lay)):
        seqs, lits = chunk(lib, c, i)
        first = bS == lay.base if (lay.base or not lay.span) else bS % lay.span == 0
        if case["sliding"] and len(case["data"]) > lay.n - lay.base:
            first = False                     # (the frame began passes ago)
        tri, got = replay(seqs, lits, buf[lay.vlo:bS], bE - bS, (1, 4, 8) if first else (0, 0, 0))
        assert got == buf[bS:bE], "block %d does not replay to its source" % i
        out.append((tri, len(lits)))
    return out


def first_difference(what, got, want):
    if got == want:
        return
    assert len(got) == len(want), "%s: %d, the model has %d" % (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: index %d: got %r, want %r" % (what, i, g, w)


def decode_both(case, comp):
    data, pre = case["data"], case["prefix"]
    assert oracle_lib.decompress(comp, len(data), dict_bytes=pre) == data, "the oracle's decoder must restore the input"
    with z.Decompressor() as d:
        if pre:
            d.RefPrefix(pre)
        assert d.Unwrap(comp, maxDecompressedSize=len(data)) == data, "the GPU decoder must restore the input"


def run_case(lib, c, case, decode=True):
    """-> what the run gave (compared between the two table orders), the merge labels its blocks reached"""
    lay, p, buf, S, M = expected(case)
    configure(lib, c, case)
    comp_f = compress(lib, c, case, skip_merge=True)
    pos, got, base, vlo = ldm_pass(lib, c)
    assert (base, vlo) == (lay.base, lay.vlo)
    if "want_splits" in case:
        assert len(S[0]) == case["want_splits"]
    first_difference("splits", pos, S[0])
    first_difference("matches", got, M)
    F = stores(lib, c, case, lay, buf)
    comp_m = compress(lib, c, case, skip_merge=False)
    pos2, got2, _, _ = ldm_pass(lib, c)
    assert (pos2, got2) == (pos, got), "the same call with the merge on gives other splits or matches"
    merged = stores(lib, c, case, lay, buf)
    labels = {}
    for i, (bS, bE) in enumerate(blocks_of(lay)):
        L = [(s - bS, n, o) for (s, n, o) in M if n and bS <= s < bE]
        want, lits, lab = lm.merge(F[i][0], L, bE - bS)
        first_difference("block %d: merged sequences" % i, merged[i][0], want)
        assert merged[i][1] == lits, "block %d: %d literal bytes, the model has %d" % (i, merged[i][1], lits)
        for k, v in lab.items():
            labels[k] = labels.get(k, 0) + v
    if decode:
        decode_both(case, comp_f)
        decode_both(case, comp_m)
    return (pos, got, merged, comp_f, comp_m), labels


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_stage_equals_the_model(gpu_lib, ctx, case):
    result, labels = run_case(gpu_lib, ctx, case)
    _first_run[case["name"]] = result
    print(case["name"], "merge labels:", sorted(labels))
    if case["merge"]:
        missing = [k for k in ldm_cases.MERGE_REACHED[case["name"]] if k not in labels]
        assert not missing, "the finder's parse no longer reaches %s" % missing


def test_reverse_order_on_the_same_context_repeats_the_first_run(gpu_lib, ctx):
    for case in CASES:
        if case["name"] not in _first_run:
            _first_run[case["name"]] = run_case(gpu_lib, ctx, case, decode=False)[0]
    for case in reversed(CASES):
        again = run_case(gpu_lib, ctx, case, decode=False)[0]
        assert again == _first_run[case["name"]], case["name"]
