"""CPU test of zstdsharp_amd/csrc/zmi_lit_ahead.h: where the serial literal decoders touch their Huffman stream ahead of the
exact look-ahead loads (decode_lit.hip, huf_decode_stream_fs).  tests/host/lit_ahead_harness.cpp is built with a stand-alone main
under AddressSanitizer and UBSan (as tests/test_frame_layout_host.py builds its harness) and run: every position from 16 bytes
below a stream's start to 1024, every stream size from 16 to 1024 and every distance of DESIGN 11's table; the 4 touched bytes
lie inside the stream, and are read there out of an exact-size allocation.  No kernel is launched here."""
import os
import re
import subprocess

from host_cc import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_touched_bytes_stay_inside_the_stream(tmp_path):
    exe = tmp_path / "lit_ahead"
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "zstdsharp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "lit_ahead_harness.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.match(r"lit_ahead: (\d+) offsets \(plain (\d+), low (\d+), high (\d+)\) built (\d+) sink [0-9a-f]+ bad=0", out.stdout)
    assert m, out.stdout[-2000:]
    n, plain, low, high, built = map(int, m.groups())
    # 1009 sizes x 6 distances x 1041 positions, and each of the three cases of the clamp was met
    assert n == 1009 * 6 * 1041 and plain + low + high == n and min(plain, low, high) > 0
    assert built % 128 == 0
