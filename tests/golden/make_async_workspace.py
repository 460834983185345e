"""Generates tests/golden/async_workspace_d.json: what ZSTDMI_batchAsyncWorkspaceD and ZSTDMI_rangesAsyncWorkspaceD answer over a fixed
list of limits (pure host arithmetic, no device).  Run ONCE against the library of the commit BEFORE the decoder's batch paths were
folded onto one list layout and one buffer table ("One list layout"): `python tests/golden/make_async_workspace.py
path/to/that/libzstd_mi355x.so`.  tests/test_async_workspace_golden.py holds every later library to these numbers."""
import ctypes, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from zstdsharp_amd import _ffi

MiB, C = 1 << 20, (1 << 20) + 5
F26, B32, C48, T27 = 1 << 26, 0xFFFFFFF0, 1 << 48, 1 << 27

# (maxEntries, srcSizeBound, maxContent, maxFrames, maxBlocks, maxSequences)
BATCH = [
    (64, 4096, MiB, 0, 0, 0), (64, 4096, MiB, 64, 0, 0), (64, 4096, MiB, 0, 64 + 64, 0), (64, 4096, MiB, 0, 0, MiB // 3 + 64),    # every default, and each one said
    (64, 4096, MiB, 64, 128, MiB // 3 + 64), (64, 4096, MiB, 100, 300, 50000), (1, 1, 1, 0, 0, 0), (777, 12345, C, 0, 0, 0), (777, 12345, C, 200, 0, 0),
    (777, 12345, C, 0, 5, 0), (777, 12345, C, 0, 0, 10), (257, 4096, 3 * MiB + 1, 513, 2049, 7),
    (0, 4096, MiB, 0, 0, 0), (64, 0, MiB, 0, 0, 0), (64, 4096, 0, 0, 0, 0),                                                          # a zero where none is allowed
    (64, 4 * MiB, MiB, 0, 0, 0), (64, 4 * MiB + 1, MiB, 0, 0, 0),                                                                    # each limit at its largest, and one above
    (F26, 4096, MiB, 0, 0, 0), (F26 + 1, 4096, MiB, 0, 0, 0), (64, 4096, MiB, F26, 0, 0), (64, 4096, MiB, F26 + 1, 0, 0),
    (B32, 4096, MiB, 1, 0, 0), (B32 + 1, 4096, MiB, 1, 0, 0), (64, 4096, MiB, 0, B32, 0), (64, 4096, MiB, 0, B32 + 1, 0),
    (64, 4096, C48, 0, B32, 0), (64, 4096, C48 + 1, 0, B32, 0), (64, 4096, C48, 1, 0, 0), (64, 4096, MiB, 0, 0, C48), (64, 4096, MiB, 0, 0, C48 + 1),
]
# (maxRanges, maxRangeBytes, maxContent, maxFrames, maxBlocks, maxSequences, tableEntries)
RANGES = [
    (64, 8192, MiB, 0, 0, 0, 1000), (64, 8192, MiB, 1000, 0, 0, 1000), (64, 8192, MiB, 0, 1000 + 64, 0, 1000), (64, 8192, MiB, 0, 0, MiB // 3 + 64, 1000),
    (64, 8192, MiB, 1000, 1064, MiB // 3 + 64, 1000), (64, 8192, MiB, 100, 300, 50000, 1000), (1, 1, 1, 0, 0, 0, 1), (777, 12345, C, 200, 0, 0, 777),
    (64, 8192, MiB, 0, 0, 0, 0), (64, 8192, MiB, 0, 0, 0, 1), (64, 8192, MiB, 100, 0, 0, 0), (64, 8192, MiB, 100, 0, 0, 1), (64, 8192, MiB, 100, 0, 0, 99),      # the table against maxFrames
    (64, 8192, MiB, 100, 0, 0, 100), (64, 8192, MiB, 100, 0, 0, 101), (64, 8192, MiB, 100, 300, 50000, 100000), (64, 8192, MiB, 0, 5, 10, 1025),
    (0, 8192, MiB, 0, 0, 0, 1000), (64, 0, MiB, 0, 0, 0, 1000), (64, 8192, 0, 0, 0, 0, 1000),
    (64, 4 * MiB, MiB, 0, 0, 0, 1000), (64, 4 * MiB + 1, MiB, 0, 0, 0, 1000), (B32, 8192, MiB, 0, 0, 0, 1000), (B32 + 1, 8192, MiB, 0, 0, 0, 1000),
    (64, 8192, MiB, 100, 0, 0, T27), (64, 8192, MiB, 100, 0, 0, T27 + 1), (64, 8192, MiB, 0, 0, 0, F26), (64, 8192, MiB, 0, 0, 0, F26 + 1),
    (64, 8192, MiB, F26, 0, 0, 1000), (64, 8192, MiB, F26 + 1, 0, 0, 1000), (64, 8192, MiB, 0, B32, 0, 1000), (64, 8192, MiB, 0, B32 + 1, 0, 1000),
    (64, 8192, C48, 0, B32, 0, 1000), (64, 8192, C48 + 1, 0, B32, 0, 1000), (64, 8192, C48, 1, 0, 0, 1000), (64, 8192, MiB, 0, 0, C48, 1000), (64, 8192, MiB, 0, 0, C48 + 1, 1000),
]


def answers(lib):
    lib.ZSTDMI_batchAsyncWorkspaceD.restype, lib.ZSTDMI_batchAsyncWorkspaceD.argtypes = _ffi.SIGNATURES["ZSTDMI_batchAsyncWorkspaceD"]
    lib.ZSTDMI_rangesAsyncWorkspaceD.restype, lib.ZSTDMI_rangesAsyncWorkspaceD.argtypes = _ffi.SIGNATURES["ZSTDMI_rangesAsyncWorkspaceD"]
    batch = [dict(limits=list(t), bytes=lib.ZSTDMI_batchAsyncWorkspaceD(ctypes.byref(_ffi.DBatchLimits(*t)))) for t in BATCH]
    ranges = [dict(limits=list(t[:6]), tableEntries=t[6], bytes=lib.ZSTDMI_rangesAsyncWorkspaceD(ctypes.byref(_ffi.DRangesLimits(*t[:6])), t[6])) for t in RANGES]
    return dict(generator="tests/golden/make_async_workspace.py", batch=batch, ranges=ranges)


if __name__ == "__main__":
    with open(os.path.join(HERE, "async_workspace_d.json"), "w") as f:
        json.dump(answers(ctypes.CDLL(sys.argv[1])), f, indent=1)
        f.write("\n")
