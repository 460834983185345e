"""The host C++ compiler for the stand-alone harnesses under tests/host (no package import: a harness needs a compiler and a header)."""
import os
import shutil

import pytest


def host_compiler():
    """a host C++ compiler: g++ where there is one, else the clang++ behind the hipcc that builds the library (HIPCC as build() reads it).
    The library cannot be built without the latter, so none at all is an error of the machine, not a reason to skip."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang++")
    for cxx in (shutil.which("g++"), shutil.which("clang++"), rocm_clang if os.path.exists(rocm_clang) else None, "/opt/rocm/llvm/bin/clang++"):
        if cxx and os.path.exists(cxx):
            return cxx
    pytest.fail("no host C++ compiler: neither g++ nor the clang++ that hipcc drives")
