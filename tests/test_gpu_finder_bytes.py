"""The match finder still writes what it wrote: tests/golden/finder_bytes.json holds, for the smallest settings and input that reach
each instance of lz_kernel and lz_region_kernel (zstdsharp_amd/csrc/lz_fast.hip), the sizes and SHA-256 of this encoder's own output.
Determinism is part of the encoder's contract, so the hash is stable; every other GPU test checks round trips, sizes against the
oracle or equality between two entry points, none of which notices a finder that picks other matches.

A pull request that changes the finder's output on purpose regenerates the file with tests/golden/make_finder_bytes.py and says so.

Each case compresses, compares sizes and hash, checks that it took the path it was written for (the region parse's kernel among the
call's stage names or not; other bytes than the tile loop alone writes, or the same: make_finder_bytes.check_path), and decodes the
result: with the GPU decoder, and behind a dictionary with the oracle's too."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_finder_bytes as mfb  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = json.load(open(mfb.JSON_PATH))["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_finder_writes_the_recorded_bytes(gpu_lib, oracle, case):
    entries = mfb.entries_of(case)
    outs, names = mfb.run_case(case, entries)
    sizes, sha = mfb.digest(outs)
    print(f"{case['name']}: sizes {sizes} (recorded {case['sizes']}), stages {names}")
    assert sizes == case["sizes"]
    assert sha == case["sha256"]
    mfb.check_path(case, outs, names, entries)
    mfb.check_roundtrip(case, outs, entries, oracle)
