"""CPU test: ZSTDMI_batchAsyncWorkspaceD and ZSTDMI_rangesAsyncWorkspaceD answer what the library answered before the decoder's work
lists got one layout and the async core one buffer table (tests/golden/async_workspace_d.json, recorded from that library by
tests/golden/make_async_workspace.py): every default left at 0 and said, the table's entries against maxFrames, each limit at its
largest admitted value and one above it (0).  Pure host arithmetic: no device is touched."""
import ctypes
import json
import os

from zstdsharp_amd import _ffi

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "async_workspace_d.json")))


def test_workspace_calls_answer_the_recorded_bytes():
    lib = _ffi.load()
    for rows in (GOLDEN["batch"], GOLDEN["ranges"]):        # (the fixture is the one the generator's list makes: refusals and sizes)
        assert len(rows) >= 24 and sum(1 for r in rows if r["bytes"] == 0) >= 8 and sum(1 for r in rows if r["bytes"] > 0) >= 16
    assert {r["tableEntries"] for r in GOLDEN["ranges"]} >= {0, 1, 99, 100, 101, 1 << 27, (1 << 27) + 1}
    for r in GOLDEN["batch"]:
        assert lib.ZSTDMI_batchAsyncWorkspaceD(ctypes.byref(_ffi.DBatchLimits(*r["limits"]))) == r["bytes"], r
    for r in GOLDEN["ranges"]:
        assert lib.ZSTDMI_rangesAsyncWorkspaceD(ctypes.byref(_ffi.DRangesLimits(*r["limits"])), r["tableEntries"]) == r["bytes"], r
