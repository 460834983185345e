"""CPU tests of zstdsharp_amd/csrc/zmi_frame.h, the one statement of a frame header's bytes and of a block's place in its frame that
the encode kernels and the host share.  tests/host/frame_layout_harness.cpp is built with a stand-alone main under AddressSanitizer
and UBSan (as tests/test_ranges_abi.py builds its harness) and run: the header's size against its written bytes and a parser written
from the format, over every combination of frame length, dictID width, checksum and form; and a block's place in the arithmetic, the
table and the single-frame form, which must agree.  No kernel is launched here."""
import os
import subprocess

import pytest

from host_cc import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("frame_layout") / "frame_layout"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "frame_layout_harness.cpp")])
    return str(exe)


def run(exe, part):
    out = subprocess.run([exe, part], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_header_size_equals_written_bytes(harness):
    # 8 lengths x 4 dictID widths x checksum on/off x (single segment, no content size, windowLog 10/17/27 with and without the size)
    assert "header: 512 combinations bad=0" in run(harness, "header")


def test_block_place_agrees_across_forms(harness):
    out = run(harness, "place")
    assert out.startswith("place: ") and out.rstrip().endswith("bad=0")
    chunks, single = int(out.split()[1]), int(out.split()[3])
    # every size of the three geometries was walked: 4 * frameBlocks + 10 chunks each, 8 + frameBlocks of them in inputs of one frame
    assert chunks == 26 + 30 + 42 and single == 12 + 13 + 16
