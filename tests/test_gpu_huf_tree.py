"""GPU tests for the Huffman table build (huf_tree_kernel): crafted histograms (tests/huf_cases.py, whose own claims
tests/test_huf_cases_cpu.py proves) through the entropy hook with no sequences, at level 1, against the oracle.  The contract is byte
identity; a Huffman-coded answer is first taken apart (verdict, then the code lengths its tree description holds against
zso_huf_buildLengths), because a wrong length or a wrong verdict still decodes and the bytes alone would only say "differs".  The table
runs twice on one context, the second time backwards: the tables, header bytes and slots live in a reused workspace, and a field that
a path forgets to write would otherwise be hidden by whatever the case before left there.
"""
import collections
import ctypes
import time

import pytest

import huf_cases as hc
import zstd_blocks as zb
import zstdsharp_amd as z

pytestmark = pytest.mark.gpu

CAP = hc.SRC + 1024


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = z.Compressor(1)
    yield c
    c.Dispose()


@pytest.fixture(scope="module")
def table(oracle):
    """(name, literals, srcSize, the oracle's block) of every case"""
    out = []
    for name, lits, exp in hc.cases():
        src = exp.get("src", len(lits))
        want = oracle.entropy_block([], lits, src, 1)
        assert not isinstance(want, int), (name, want)
        out.append((name, lits, src, want))
    return out


def _verdict(body):
    """what was decided, without the bytes -> a tuple that reads well in a report"""
    if not body: return ("raw block",)
    lit_type, _, _ = zb.literals_of(body)
    if lit_type != 2: return (("raw", "RLE")[lit_type] + " literals",)
    fmt = (body[0] >> 2) & 3
    lh = (3, 3, 4, 5)[fmt]
    return ("Huffman", f"{1 if fmt == 0 else 4} streams", f"{lh}-byte header", "FSE weights" if body[lh] < 128 else "4-bit weights")


def _described_lengths(oracle, body):
    """the code lengths a Huffman-coded section's tree description holds, through the oracle's HUF_readStats -> (lengths, tableLog)"""
    lh = (3, 3, 4, 5)[(body[0] >> 2) & 3]
    weights = ctypes.create_string_buffer(256)
    nsym, log, ranks = ctypes.c_uint32(0), ctypes.c_uint32(0), (ctypes.c_uint32 * 16)()
    r = oracle.lib().zso_huf_readStats(weights, ctypes.byref(nsym), ctypes.byref(log), ranks, body[lh:], len(body) - lh)
    if oracle.is_error(r): return None, 0
    return [log.value + 1 - w if w else 0 for w in weights.raw[:nsym.value]], log.value


def _oracle_lengths(oracle, lits):
    cnt = collections.Counter(lits)
    hist = [cnt.get(s, 0) for s in range(max(cnt) + 1)]
    out = ctypes.create_string_buffer(256)
    r = oracle.lib().zso_huf_buildLengths(out, (ctypes.c_uint32 * 256)(*hist), len(hist) - 1, hc.plan(hist)[0])
    assert not oracle.is_error(r), r
    return list(out.raw[:len(hist)]), r


def _run(gpu_lib, ctx, out, name, lits, src):
    r = gpu_lib.ZSTDMI_debugEntropyBlock(ctx.cctx, out, CAP, None, 0, lits, len(lits), src)
    assert r < (1 << 63), (name, r)
    return out.raw[:r]


def _report(lines, failures):
    print("\n".join(lines))
    assert not failures, f"{len(failures)} mismatches, the first: {failures[:8]}"


def test_tree_cases_match_the_oracle_phase_by_phase(gpu_lib, ctx, oracle, table):
    out = ctypes.create_string_buffer(CAP)
    assert len(table) >= 80
    _run(gpu_lib, ctx, out, *table[0][:3])                  # (the first call sizes the workspace: not part of the time per call)
    t0, lines, failures = time.perf_counter(), [], []
    for name, lits, src, want in table:
        got = _run(gpu_lib, ctx, out, name, lits, src)
        lines.append(f"{name}: {len(lits)} literals, oracle {len(want)} B, gpu {len(got)} B")
        if _verdict(got) != _verdict(want):
            failures.append((name, "verdict", _verdict(got), _verdict(want)))
            continue
        if want and zb.literals_of(want)[0] == 2:
            nb, log = _described_lengths(oracle, got)
            want_nb, want_log = _oracle_lengths(oracle, lits)
            if nb != want_nb or log != want_log:
                first = next((s for s in range(min(len(nb or []), len(want_nb))) if nb[s] != want_nb[s]), None)
                failures.append((name, "lengths", "unreadable description" if nb is None else f"tableLog {log}/{want_log}, {len(nb)}/{len(want_nb)} symbols",
                                 "first differing symbol", first, "got/want", None if first is None else (nb[first], want_nb[first])))
                continue                        # (the bytes follow the lengths: one finding, not two)
        if got != want:
            at = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
            failures.append((name, "bytes", f"first differing byte {at} of {len(got)}/{len(want)}"))
    dt = time.perf_counter() - t0
    lines.append(f"tree cases: {len(table)} blocks in {dt:.2f} s, {dt / len(table) * 1e3:.2f} ms per call")
    _report(lines, failures)


def test_second_pass_in_reverse_order_gives_the_same_answers(gpu_lib, ctx, table):
    out = ctypes.create_string_buffer(CAP)
    t0 = time.perf_counter()
    first = {name: _run(gpu_lib, ctx, out, name, lits, src) for name, lits, src, _ in table}
    failures = []
    for name, lits, src, want in reversed(table):
        got = _run(gpu_lib, ctx, out, name, lits, src)
        if got != first[name]:
            failures.append((name, "differs from the first pass", _verdict(got), _verdict(first[name]), len(got), len(first[name])))
        elif got != want:
            failures.append((name, "both passes differ from the oracle", _verdict(got), _verdict(want)))
    dt = time.perf_counter() - t0
    _report([f"two passes: {2 * len(table)} blocks in {dt:.2f} s, {dt / (2 * len(table)) * 1e3:.2f} ms per call"], failures)
