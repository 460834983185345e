"""CPU tests of zstdsharp_amd/csrc/zmi_batch_plan.h, the one statement of how ZSTDMI_compressBatchAsync cuts a call's entries into
chunks on the device: the argument checks, an entry's chunk count, the chunk limit's refusal rule, which entry owns a chunk slot, and
the slot's record (from, len, frame word).  tests/host/batch_plan_harness.cpp is built with a stand-alone main under AddressSanitizer and
UBSan (as tests/test_frame_layout_host.py builds its harness) and run: the plan, evaluated per entry and per slot as the kernels
evaluate it, against a plain restatement of compress_entries' host loop.  No kernel is launched here."""
import os
import subprocess

import pytest

from host_cc import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("batch_plan") / "batch_plan"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "batch_plan_harness.cpp")])
    return str(exe)


def run(exe, part):
    out = subprocess.run([exe, part], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_plan_equals_the_host_loop(harness):
    # five framings (16 KiB x 4, 48 KiB x 5, 32 KiB x 8, and frameBlocks 0 at 32 and 64 KiB) x 8 lists, once under a bound of 4 MiB - 1
    # (sizes 0, 1, cb - 1, cb, cb + 1, frameBlocks * cb +- 1, 4 MiB - 1; failed entries of every kind in between; seeded lists) and once
    # under a bound of three chunks and a bit
    out = run(harness, "plan")
    assert out.startswith("plan: 80 lists ") and out.rstrip().endswith("bad=0")
    assert int(out.split()[3]) > 10000          # (chunks walked)


def test_refusal_rule_at_total_total_minus_one_and_one(harness):
    out = run(harness, "limit")
    assert out.startswith("limit: ") and out.rstrip().endswith("bad=0")
    assert int(out.split()[1]) >= 5 * 8 * 3


def test_owner_search_steps_over_entries_without_chunks(harness):
    assert run(harness, "owner").rstrip() == "owner: 7 tables bad=0"
