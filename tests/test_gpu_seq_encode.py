"""GPU tests for the sequence encoder (seq_encode_kernel): crafted seqStores (tests/seq_cases.py, whose own claims
tests/test_seq_cases_cpu.py proves) through the entropy hooks at levels 1, 3, 5 and 9, against the oracle's restatement of
ZSTD_entropyCompressSeqStore at strategies 1, 2, 3 and 3.  The contract is byte identity; for raw offsets the resolved codes are
compared with the serial rule first, because a missed repcode is still a valid encoding and the bytes alone would only say "differs".
"""
import ctypes
import struct
import time

import pytest

import seq_cases as sc
import zstdsharp_amd as z
from zstdsharp_amd import _ffi

pytestmark = pytest.mark.gpu

CAP = sc.SRC + 1024


@pytest.fixture(scope="module")
def level_ctxs(gpu_lib):
    ctxs = [(z.Compressor(level), strategy) for level, strategy in sc.LEVELS]
    yield ctxs
    for c, _ in ctxs: c.Dispose()


@pytest.fixture(scope="module")
def buffers():
    return ctypes.create_string_buffer(CAP), (_ffi.ZSTDMI_Seq * 16384)(), ctypes.create_string_buffer(64)


def _seq_array(seqs):
    flat = [v for s in seqs for v in s]
    return (_ffi.ZSTDMI_Seq * max(len(seqs), 1)).from_buffer_copy(struct.pack(f"<{'IHH' * len(seqs)}", *flat) if seqs else bytes(8))


def _report(lines, failures):
    print("\n".join(lines))
    assert not failures, f"{len(failures)} mismatches, the first: {failures[:8]}"


def test_entropy_cases_are_byte_identical_to_oracle(gpu_lib, level_ctxs, oracle, buffers):
    out = buffers[0]
    cases = sc.entropy_cases()
    assert len(cases) > 150
    t0, lines, failures, wants = time.perf_counter(), [], [], {}
    for name, seqs, lits, src, _ in cases:
        arr = _seq_array(seqs)
        for (c, strategy), (level, _) in zip(level_ctxs, sc.LEVELS):
            if (name, strategy) not in wants:
                wants[name, strategy] = oracle.entropy_block(seqs, lits, src, strategy)
            want = wants[name, strategy]
            assert not isinstance(want, int), (name, want)
            r = gpu_lib.ZSTDMI_debugEntropyBlock(c.cctx, out, CAP, arr, len(seqs), lits, len(lits), src)
            assert r < (1 << 63), (name, level, r)
            lines.append(f"{name} L{level}: nbSeq {len(seqs)} oracle {len(want)} B, gpu {r} B")
            if out.raw[:r] != want: failures.append((name, level, len(want), r))
    lines.append(f"entropy cases: {len(cases)} stores x {len(sc.LEVELS)} levels in {time.perf_counter() - t0:.2f} s")
    _report(lines, failures)


def test_raw_offsets_resolve_by_the_serial_rule_and_code_as_the_oracle(gpu_lib, level_ctxs, oracle, buffers):
    out, back, back_lits = buffers
    cases = sc.repcode_cases()
    assert len(cases) > 250
    t0, lines, failures, wants = time.perf_counter(), [], [], {}
    ns, ls = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for name, raw, lits, src, rep in cases:
        arr, n = _seq_array(raw), len(raw)
        resolved = sc.resolve_reps(raw, rep)
        rep_arr = (ctypes.c_uint * 3)(*rep)
        for (c, strategy), (level, _) in zip(level_ctxs, sc.LEVELS):
            r = gpu_lib.ZSTDMI_debugEntropyBlockRaw(c.cctx, out, CAP, arr, n, lits, len(lits), src, rep_arr)
            assert r < (1 << 63), (name, level, r)
            assert gpu_lib.ZSTDMI_debugGetChunk(c.cctx, 0, back, 16384, ctypes.byref(ns), back_lits, 64, ctypes.byref(ls)) == 0
            assert ns.value == n and back_lits.raw[:ls.value] == lits, name
            got = [(back[i].offBase, back[i].litLength, back[i].mlBase) for i in range(n)]
            if got != resolved:
                first = next(i for i in range(n) if got[i] != resolved[i])
                failures.append((name, level, "codes", first, got[first], resolved[first]))
                continue                        # (the bytes follow the codes: one finding, not two)
            if (name, strategy) not in wants:
                wants[name, strategy] = oracle.entropy_block(resolved, lits, src, strategy)
            want = wants[name, strategy]
            assert not isinstance(want, int) and want, (name, want)
            lines.append(f"{name} L{level}: nbSeq {n} oracle {len(want)} B, gpu {r} B")
            if out.raw[:r] != want: failures.append((name, level, "bytes", len(want), r))
    lines.append(f"repcode cases: {len(cases)} stores x {len(sc.LEVELS)} levels in {time.perf_counter() - t0:.2f} s")
    _report(lines, failures)


def test_raw_hook_refuses_what_is_no_distance(gpu_lib, level_ctxs, buffers):
    """offBase below 4 is no distance + 3, a store above the hook's bounds is refused before anything is launched, and the plain
    hook's answer does not depend on what the raw one left behind"""
    out = buffers[0]
    c = level_ctxs[0][0]
    rep = (ctypes.c_uint * 3)(1, 4, 8)
    lits = bytes(40)
    assert gpu_lib.ZSTDMI_debugEntropyBlockRaw(c.cctx, out, CAP, _seq_array([(3, 1, 1)]), 1, lits, 40, sc.SRC, rep) > (1 << 63)
    assert gpu_lib.ZSTDMI_debugEntropyBlockRaw(c.cctx, out, CAP, _seq_array([(9, 1, 1)]), 1, lits, 40, sc.SRC + 1, rep) > (1 << 63)
    raw = [(7, 2, 3), (7, 2, 3), (11, 0, 5)]
    r1 = gpu_lib.ZSTDMI_debugEntropyBlockRaw(c.cctx, out, CAP, _seq_array(raw), 3, lits, 40, sc.SRC, rep)
    first = out.raw[:r1]
    r2 = gpu_lib.ZSTDMI_debugEntropyBlock(c.cctx, out, CAP, _seq_array(sc.resolve_reps(raw, (1, 4, 8))), 3, lits, 40, sc.SRC)
    assert 0 < r1 == r2 < (1 << 63) and out.raw[:r2] == first
