"""CPU tests of the content-defined cut rule, version 1: tests/content_cuts_cases.py (the numpy restatement) against the stored fixture
and against the rule's own properties, the resync condition the GPU test rests on, and zmi_cuts.h — the text the select kernel walks —
on the CPU: tests/host/cuts_harness.cpp, built with its own main under AddressSanitizer and UBSan, against tables exported from the
restatement.  No kernel is launched here."""
import json
import os
import subprocess

import numpy as np
import pytest

import content_cuts_cases as cc
from host_cc import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_reproduces_the_fixture():
    fixture = json.load(open(cc.GOLDEN))
    assert fixture["rule_version"] == cc.RULE_VERSION == 1
    assert os.path.getsize(cc.GOLDEN) < 65536
    assert len(fixture["cases"]) == 6
    assert fixture["cases"] == cc.golden_cases()


def test_gear_table_and_hash_window():
    assert cc.splitmix64(0) == 0xE220A8397B1DCDAF          # splitmix64's first output for the state 0 (the published test vector)
    # h(p) is the last 64 bytes' alone: equal tails give equal hashes, and the 65th byte back does not matter
    a, b = cc.base("rand")[:4096], cc.base("zipf")[:4096]
    ha, hb = cc.hashes(a[:1000] + b[1000:]), cc.hashes(b)
    assert np.array_equal(ha[1063:], hb[1063:]) and ha[1062] != hb[1062]
    # the rolling form
    h = 0
    for p, byte in enumerate(a[:300]):
        h = ((h << 1) + int(cc.GEAR[byte])) & cc.M64
        assert h == int(cc.hashes(a[:300])[p])


@pytest.mark.parametrize("avg_log", [12, 13, 14, 15, 16])
@pytest.mark.parametrize("kind", ["rand", "text", "zipf", "mixed", "flat"])
def test_piece_lengths(kind, avg_log):
    data = cc.base(kind)[:400000 + avg_log]
    sizes = cc.piece_sizes(data, avg_log)
    assert sum(sizes) == len(data) and all(0 < s <= cc.MAX for s in sizes)
    assert all(s >= cc.min_of(avg_log) for s in sizes[:-1])
    assert len(sizes) <= len(data) // cc.min_of(avg_log) + 1
    assert cc.piece_sizes(b"", avg_log) == []


def test_constant_byte_gives_only_forced_cuts():
    b = cc.flat_byte()
    for avg_log in cc.AVG_LOGS:
        assert len(cc.candidates(bytes([b]) * 300000, avg_log)) == 0
        assert cc.piece_sizes(bytes([b]) * 300000, avg_log) == [65536] * 4 + [300000 - 4 * 65536]


@pytest.mark.parametrize("kind", ["rand", "text", "zipf"])
def test_resync_after_an_insertion(kind):
    """the condition tests/test_gpu_content_cuts.py's resync test rests on: 1 MiB, seed 7, avgLog 12, three bytes inserted at offset 5000 —
    the piece lists differ in at most 8 leading pieces each and are equal from there on (3 here; 8 keeps the test from hiding a failure)"""
    data = cc.base(kind)
    a, b = cc.piece_sizes(data, 12), cc.piece_sizes(cc.insert_edit(data), 12)
    ia, ib = cc.resync(a, b)
    print(kind, "differing leading pieces:", ia, ib, "of", len(a), len(b))
    assert ia <= 8 and ib <= 8 and a[ia:] == b[ib:] and len(a) - ia > 100
    assert sum(a[:ia]) + 3 == sum(b[:ib]) and sum(a[:ia]) >= 5000


# ---- zmi_cuts.h on the CPU ----
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cuts") / "cuts_harness"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "cuts_harness.cpp")])
    return str(exe)


def run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_header_gear_table(harness):
    assert [int(x, 16) for x in run(harness, "gear").split()] == [int(g) for g in cc.GEAR]


def test_header_bound(harness):
    for avg_log in (12, 14, 16):
        for n in (0, 1, 4095, 4096, 65536, 1 << 20, (1 << 32) - 1, 1 << 40):
            assert int(run(harness, "bound", str(n), str(avg_log))) == cc.bound(n, avg_log)
    assert run(harness, "bound", str((1 << 64) - 1), "12").strip() == "overflow"
    assert run(harness, "bound", str((1 << 64) - 70000), "16").strip() == "overflow"


def test_header_walk_against_the_restatement(harness, tmp_path):
    """cut_walk — forced runs in one step, the candidate too close behind a forced cut — against one searchsorted per piece"""
    cases = []
    for kind in ("rand", "text", "zipf", "flat"):
        for avg_log in cc.AVG_LOGS:
            for n in (0, 1, cc.min_of(avg_log) - 1, cc.min_of(avg_log), cc.min_of(avg_log) + 1, 65535, 65536, 65537, 200000, 1 << 20):
                data = cc.base(kind)[:n]
                cases.append((n, avg_log, cc.candidates(data, avg_log).tolist()))
    # crafted lists: candidates at every distance around min and max from a piece start, and in every place behind a forced cut
    for avg_log in cc.AVG_LOGS:
        mn = cc.min_of(avg_log)
        for d in (mn - 1, mn, mn + 1, cc.MAX - 1, cc.MAX, cc.MAX + 1, cc.MAX + mn - 1, cc.MAX + mn, 2 * cc.MAX, 2 * cc.MAX + 1, 3 * cc.MAX + mn - 1):
            for tail in (0, 1, mn, cc.MAX, cc.MAX + 1):
                cases.append((mn + d + tail, avg_log, [mn, mn + d]))
                cases.append((mn + d + tail, avg_log, [mn, mn + d - 1, mn + d, mn + d + 1]))
        cases.append((5 * cc.MAX, avg_log, list(range(1, 5 * cc.MAX + 1, 7))))
        cases.append((300000, avg_log, list(range(1, 300001))))          # every position a candidate: all pieces are min
        # the largest source: ends are 32-bit words, and s + min passes 2^32 in front of the last piece
        top = (1 << 32) - 1
        for tail in ([top], [top - 10], [top - mn + 1, top], [top - mn, top - 1], [top - mn - 1], [top - cc.MAX - 1, top - cc.MAX + mn - 2], []):
            cases.append((top, avg_log, [mn, 2 * cc.MAX + 7] + tail))
        cases.append((top - 1, avg_log, [top - 3 * mn, top - 2]))
    path = tmp_path / "walk.txt"
    with open(path, "w") as f:
        for n, avg_log, cands in cases:
            cands = [c for c in cands if c <= n]
            ends = cc.select(np.array(cands, dtype=np.int64), n, avg_log)
            f.write(f"{n} {avg_log} {len(cands)} {len(ends)}\n{' '.join(map(str, cands))}\n{' '.join(map(str, ends))}\n")
    assert run(harness, "walk", str(path)).strip().splitlines()[-1] == f"walk: {len(cases)} cases bad=0"


def test_header_candidates_against_the_restatement(harness, tmp_path):
    for kind, avg_log in (("rand", 12), ("text", 14), ("zipf", 16), ("flat", 12)):
        data = cc.base(kind)[:300001]
        path = tmp_path / f"{kind}.bin"
        path.write_bytes(data)
        assert [int(x) for x in run(harness, "mark", str(path), str(avg_log)).split()] == cc.candidates(data, avg_log).tolist()
