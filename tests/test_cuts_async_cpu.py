"""CPU tests of the parallel cut selection (zmi_cut_rank.h: the successor rule, the doubling rounds, the scan), the text
content_cuts_async.hip's kernels run: tests/host/cut_rank_harness.cpp, built with its own main under AddressSanitizer and UBSan, against
piece ends from the numpy restatement of the rule (content_cuts_cases.select).  No kernel is launched here."""
import os
import subprocess

import pytest

import content_cuts_cases as cc
import cuts_async_cases as ca
from host_cc import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cutrank") / "cut_rank_harness"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "cut_rank_harness.cpp")])
    return str(exe)


def run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def write_cases(path, cases):
    with open(path, "w") as f:
        for case in cases:
            n, avg_log, cands = case
            ends = ca.expected(case)
            f.write(f"{n} {avg_log} {len(cands)} {len(ends)}\n{' '.join(map(str, cands))}\n{' '.join(map(str, ends))}\n")


def last_line(out):
    return out.strip().splitlines()[-1]


def test_round_count(harness):
    """ceil(log2(maxPieces + 1)): a path of P nodes in front of the end is covered by the rounds, and by no fewer"""
    for p, want in ((0, 0), (1, 1), (2, 2), (3, 2), (4, 3), (7, 3), (8, 4), (1025, 11), ((1 << 22) + 1, 23)):
        assert int(run(harness, "rounds", str(p))) == want
        assert (1 << want) >= p + 1 and (want == 0 or (1 << (want - 1)) < p + 1)


def test_rank_against_the_restatement(harness, tmp_path):
    """successor + rounds + scan against one searchsorted per piece: real lists, crafted pairs around min / max / max + min / k max, the
    comb, every position a candidate (the longest path: one round fewer would leave its tail unmarked), the 2^32 - 1 tails"""
    cases = ca.real() + ca.crafted()
    assert max(len(ca.expected(c)) for c in cases if c[0] == 300000) == 300000 // cc.min_of(12) + 1     # the longest path is in the table
    path = tmp_path / "rank.txt"
    write_cases(path, cases)
    line = last_line(run(harness, "rank", str(path)))
    print(line)
    assert line.startswith(f"rank: {len(cases)} cases bad=0 ")


def test_dense_clusters_are_jumped_over(harness, tmp_path):
    """a dense cluster, a gap above max, a dense cluster of 20 000 entries: a node's successor costs fewer than 64 entries read and
    zones left, however many candidates lie in the bad zone it lands in (a scan entry by entry would read min - 1 = 1023 of them)"""
    case = ca.clusters()
    n, avg_log, cands = case
    ends = ca.expected(case)
    # the case is what it claims to be: 20 000 entries behind a gap above max, and for the node at 3000 a bad zone that holds 900 of them
    first_b = next(c for c in cands if c > 3000)
    assert first_b - 3000 > cc.MAX and len([c for c in cands if c >= first_b]) == 20000
    assert len([c for c in cands if 3000 + cc.MAX < c <= 3000 + cc.MAX + cc.min_of(avg_log) - 1]) > 900
    assert any(e not in set(cands) for e in ends[:-1])          # (and the path itself takes a forced cut)
    path = tmp_path / "clusters.txt"
    write_cases(path, [case])
    line = last_line(run(harness, "rank", str(path)))
    print(line)
    assert line.startswith("rank: 1 cases bad=0 ")
    assert int(line.split("maxSteps=")[1]) < 64
