"""CPU test of the window logic of huf_decode_stream_fs (decode_lit.hip): the function's text is lifted out of the .hip file
as in test_lit_decoder_host.py and compiled, with AddressSanitizer and UBSan, into a stand-alone program
(tests/host/lit_window_harness.cpp) that decodes streams of the longest and the shortest codes, every symbol count at which the
function changes form, and streams of 15 to 64 bytes; the program counts how many cases went through the steady groups, the
general groups and the plain bit reader and fails if one of them was never taken."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_window_logic_on_the_host(tmp_path):
    src = open(os.path.join(ROOT, "zstdsharp_amd", "csrc", "decode_lit.hip")).read()
    a = src.index("template <u32 IDX, bool PAIRS>\n__device__ __forceinline__ bool huf_decode_stream_fs")
    b = src.index("// ------------------------------------------------------------------------------------------------\n// literals, fast path")
    (tmp_path / "fs.inc").write_text(src[a:b].replace("__device__ __forceinline__", "static inline").replace("__restrict__", ""))
    hdr = open(os.path.join(ROOT, "zstdsharp_amd", "csrc", "zmi_decode.h")).read()
    bb = hdr[hdr.index("struct BackBits {"):hdr.index("struct SeqSym")].replace("__device__ __forceinline__", "inline")
    (tmp_path / "bb.inc").write_text(bb)
    shutil.copy(os.path.join(ROOT, "tests", "host", "lit_window_harness.cpp"), tmp_path / "t.cpp")
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), str(tmp_path / "t.cpp")], cwd=tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, cwd=tmp_path)
    print(out.stdout[-600:])
    assert out.returncode == 0 and "done bad=0" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"cases (\d+) steady (\d+) general (\d+) reader (\d+)", out.stdout)
    assert m and all(int(x) > 0 for x in m.groups()), out.stdout[-600:]
