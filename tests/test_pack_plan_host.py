"""CPU tests of the pack arithmetic in zstdsharp_amd/csrc/zmi_batch_plan.h, the one statement of how ZSTDMI_compressPackAsync places a
call's entries in ONE stream on the device: what an entry answers without a destination of its own, its bytes and rows, the one answer
of the call (the lowest failing entry's, else frames plus table against the capacity), every chunk slot's address and the table's rows.
tests/host/pack_plan_harness.cpp is built with a stand-alone main under AddressSanitizer and UBSan (as tests/test_batch_plan_host.py
builds its harness) and run: the arithmetic, evaluated per entry and per slot as the kernels evaluate it, against a plain host loop.
No kernel is launched here."""
import os
import subprocess

import pytest

from host_cc import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pack_plan") / "pack_plan"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "pack_plan_harness.cpp")])
    return str(exe)


def run(exe, part):
    out = subprocess.run([exe, part], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_seeded_lists_with_failures_on_both_sides_of_a_cut(harness):
    # five framings x 6 seeded lists of 40 .. 239 entries (every seventh empty): the list as it is, under a chunk limit that cuts in the
    # middle, and with one oversize or NULL-source entry in front of and behind that cut, each with and without the limit
    assert run(harness, "lists").rstrip() == "lists: 300 runs 240 failing bad=0"


def test_entry_counts_at_the_scan_edges(harness):
    # n = 1, 16, 17, 1024, 1025, 16384 under five framings, seeded and all-empty; n = 0 in 17 and in 16 bytes
    assert run(harness, "counts").rstrip() == "counts: 62 runs bad=0"


def test_capacity_exact_one_short_and_without_room_for_the_table(harness):
    assert run(harness, "capacity").rstrip() == "capacity: 120 runs bad=0"
