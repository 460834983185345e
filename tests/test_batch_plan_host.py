"""CPU tests of zstdsharp_amd/csrc/zmi_batch_plan.h, the one statement of how ZSTDMI_compressBatchAsync cuts a call's entries into
chunks on the device: the argument checks, an entry's chunk count, the chunk limit's refusal rule, which entry owns a chunk slot, and
the slot's record (from, len, frame word).  tests/host/batch_plan_harness.cpp is built with a stand-alone main under AddressSanitizer and
UBSan (as tests/test_frame_layout_host.py builds its harness) and run: the plan, evaluated per entry and per slot as the kernels
evaluate it, against a plain restatement of compress_entries' host loop.  The same harness holds zmi_batch_pass.h to account, the
header compress_entries calls for its host decisions: the fill of a pass's table (against the restatement and the device plan), the
layouts of the four tables, and the cut of a group into passes.  No kernel is launched here."""
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


# ---- zmi_batch_pass.h: what compress_entries itself calls (the group's cut into passes, the pass's table, its fill) ----

def test_host_fill_equals_the_restatement_and_the_device_plan(harness):
    # the same five framings x 8 lists without a limit: batch_pass_fill over each list's good entries, with and without destinations
    # and seek rows: from / len / frame word per chunk, entFirst, entDst relative to the lowest destination, entCap (~0 without
    # destinations), the seek column, lo and span
    out = run(harness, "fill")
    assert out.startswith("fill: 40 lists ") and out.rstrip().endswith("bad=0")
    assert int(out.split()[3]) > 10000          # (chunks walked)


def test_table_layouts(harness):
    # batch_pass_tab == the offset arithmetic it replaced over nCh {1, 2, 3, 255, 256, 16384} x nEnt {1, 2, nCh} x frame words x seek
    # rows x slots {0, 2, 3} x carry (nEnt <= nCh: 17 of the 18 pairs, 24 tables each, and with each pair the three tables of the
    # calls enqueued from the device, a pack's for 1, 2 and 5 frames an entry); all four tables: no column overlaps another, u64 and
    # CDictSlot columns 8-aligned, `bytes` covers the last
    assert run(harness, "layout").rstrip() == f"layout: {17 * (24 + 5)} cases bad=0"


def test_pass_cut_is_the_pack_round_cut(harness):
    # limits 1, 2, 16384; an entry of exactly the limit, one above what is left, one above the limit; seeded runs, with and without
    # entries that go alone in between: batch_pass_cut == compress_entries' old loop == ZSTDMI_compressPack's old round expression
    out = run(harness, "cut")
    assert out.startswith("cut: ") and out.rstrip().endswith("bad=0")
    assert int(out.split()[1]) > 1000


def test_group_key_in_both_meanings(harness):
    # 528 keys (prefix length x chunk size x blocks per frame x indexed x slot x Resolved with each of its ten fields changed once),
    # every pair, with and without per-entry CDicts: same_group == the six-clause condition it replaced, and symmetric
    assert run(harness, "group").rstrip() == f"group: 528 keys {528 * 528 * 2} pairs bad=0"
