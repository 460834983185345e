"""Generates tests/golden/pysrc_4m.xz: the first 4 MiB of the Python sources of CPython 3.10's standard library (Lib/**/*.py in
sorted path order, concatenated; PSF License), the real-world source code the far-history ratio test of test_gpu_history.py
compresses.  Run ONCE with the path of a CPython 3.10 Lib/ directory; the output is committed and the tests only read it.

usage: python tests/golden/make_pysrc.py /path/to/cpython/Lib
"""
import glob
import hashlib
import lzma
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SIZE = 4 << 20

if __name__ == "__main__":
    lib = sys.argv[1]
    data = b""
    for f in sorted(glob.glob(os.path.join(lib, "**", "*.py"), recursive=True)):
        data += open(f, "rb").read()
        if len(data) >= SIZE:
            break
    data = data[:SIZE]
    assert len(data) == SIZE, len(data)
    open(os.path.join(HERE, "pysrc_4m.xz"), "wb").write(lzma.compress(data, preset=9 | lzma.PRESET_EXTREME))
    print("pysrc_4m.xz: sha256 of the content", hashlib.sha256(data).hexdigest())
