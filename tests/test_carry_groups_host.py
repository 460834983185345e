"""CPU tests of zstdsharp_amd/csrc/zmi_carry.h, the one statement of which chunks of a pass form a carry group
(ZSTDMI_CCtx_setEntropyCarry) that seq_encode's carry instance and the host share.  tests/host/carry_groups_harness.cpp is built with a
stand-alone main under AddressSanitizer and UBSan (as tests/test_frame_layout_host.py builds its harness) and run: leaders and spans
in the arithmetic, the table and the single-frame form against a count done there, and the rounding of a pass under the single
frame.  No kernel is launched here."""
import os
import subprocess

import pytest

from host_cc import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("carry_groups") / "carry_groups"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "carry_groups_harness.cpp")])
    return str(exe)


def run(exe, part):
    out = subprocess.run([exe, part], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_arithmetic_form(harness):
    # frames of 1, 2, 5, 8, 9 and 17 blocks, every pass length up to three frames and two chunks
    out = run(harness, "arith")
    assert out.startswith("arith: ") and out.rstrip().endswith("bad=0")
    assert int(out.split()[1]) == sum(3 * fb + 2 for fb in (1, 2, 5, 8, 9, 17))


def test_table_form_with_entries_of_mixed_lengths(harness):
    out = run(harness, "table")
    assert out.startswith("table: ") and out.rstrip().endswith("bad=0")
    assert int(out.split()[1]) == 5 * 4


def test_single_form_on_and_off_a_group_boundary(harness):
    out = run(harness, "single")
    assert out.startswith("single: ") and out.rstrip().endswith("bad=0")
    assert int(out.split()[1]) == 7 * 7


def test_pass_rounding(harness):
    out = run(harness, "pass")
    assert out.startswith("pass: ") and out.rstrip().endswith("bad=0")
