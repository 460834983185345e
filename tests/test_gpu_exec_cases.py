"""GPU tests (run with -m gpu on an MI355X): match execution on the crafted dependency chains of tests/exec_cases.py — the one-wave
executor, the wide executor at every width, the origin path, and the copy routines beneath them (DESIGN.md "Parity").

The yardstick is the forge's serial executor (tests/zstd_forge.py `execute`), which the oracle confirms on the CPU
(tests/test_exec_cases_cpu.py); the comparison is exact.  A missed dependency is a race that nothing reports, so every destination
is a device buffer filled with a poison byte first, every setting runs twice with two poisons (a stale read cannot give the
expected byte both times), and 64 guard bytes behind each result must keep the poison."""
import ctypes

import numpy as np
import pytest

import exec_cases as E
import oracle_lib
import zstdsharp_amd as z
from zstdsharp_amd.batch import decompress_batch_async
from zstdsharp_amd.errors import ZSTD_ErrorCode, get_error_code, is_error

pytestmark = pytest.mark.gpu

POISONS = (0xA5, 0x5A)
GUARD = 64
WIDTHS = (1, 2, 4, 8, 16)
CORRUPTION = int(ZSTD_ErrorCode.ZSTD_error_corruption_detected)
DDICT_IDS = (4242, 777777)


def group_of(tags):
    return "padded" if "padded" in tags else tags[0]


GROUPS = ("chain", "touch", "span", "block-edge", "copy-sweep", "literals", "dict", "negative", "padded")
assert {group_of(c[1]) for c in E.CASES} == set(GROUPS)


class Entry:
    def __init__(self, name, tags, blob, content, dic, at):
        self.name, self.tags, self.blob, self.content, self.dic, self.at = name, tags, blob, content, dic, at
        self.valid = content is not None
        self.cap = len(content) if self.valid else E.SPECS[name].stated_size()


class Table:
    """every case forged once, the frames side by side in one device tensor (64-byte aligned), one destination buffer for all"""

    def __init__(self, cases):
        import torch
        self.torch = torch
        self.entries, parts, at = [], [], 0
        for name, tags, blob, content, dic in cases:
            self.entries.append(Entry(name, tags, blob, content, dic, at))
            pad = -len(blob) % 64
            parts.append(blob + bytes(pad))
            at += len(blob) + pad
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).cuda()
        self.dst = torch.empty(max(e.cap for e in self.entries) + GUARD, dtype=torch.uint8, device="cuda")

    def group(self, g):
        return [e for e in self.entries if group_of(e.tags) == g]

    def decode(self, lib, d, e, poison):
        """one ZSTDMI_decompressDevice call into the poisoned buffer -> None, or what is wrong"""
        n = e.cap
        self.dst[:n + GUARD].fill_(poison)
        self.torch.cuda.synchronize()
        r = lib.ZSTDMI_decompressDevice(d.dctx, self.dst.data_ptr(), n, self.src.data_ptr() + e.at, len(e.blob))
        host = self.dst[:n + GUARD].cpu().numpy()
        if not (host[n:] == poison).all():
            return "guard bytes written"
        if not e.valid:
            return None if is_error(r) and int(get_error_code(r)) == CORRUPTION else f"negative answered {r if not is_error(r) else -int(get_error_code(r))}"
        if is_error(r) or r != n:
            return f"returned {-int(get_error_code(r)) if is_error(r) else r}, not {n}"
        if host[:n].tobytes() != e.content:
            bad = np.flatnonzero(host[:n] != np.frombuffer(e.content, dtype=np.uint8))
            return f"{bad.size} wrong bytes, first at {bad[:4].tolist()} (poison there: {(host[bad] == poison).sum()})"
        return None

    def sweep(self, lib, entries, setup, after=None):
        """the entries under one setting, once per poison; cases behind the raw dictionary on a context that has loaded it"""
        plain, dicted = z.Decompressor(), z.Decompressor()
        try:
            dicted.LoadDictionary(E.dictionary())
            for d in (plain, dicted):
                setup(d)
            wrong = []
            for poison in POISONS:
                for e in entries:
                    d = dicted if e.dic else plain
                    w = self.decode(lib, d, e, poison)
                    if w:
                        wrong.append((e.name, hex(poison), w))
                    elif after:
                        after(d, e)
            assert not wrong, (len(wrong), wrong[:6])
        finally:
            plain.Dispose()
            dicted.Dispose()


@pytest.fixture(scope="module")
def table(gpu_lib):
    return Table([(name, tags) + build() for name, tags, build, valid in E.CASES])


def settings(lib, **kw):
    names = {"waves": "ZSTDMI_DCtx_setExecWaves", "long_frames": "ZSTDMI_DCtx_setLongFrames", "overlap": "ZSTDMI_DCtx_setOverlap",
             "literals": "ZSTDMI_DCtx_setLiteralDecoder", "profiling": "ZSTDMI_DCtx_setProfiling"}

    def setup(d):
        for k, v in kw.items():
            assert getattr(lib, names[k])(d.dctx, v) == 0, (k, v)
    return setup


def stages(lib, d):
    ms = (ctypes.c_float * 24)(); names = (ctypes.c_char_p * 24)()
    k = lib.ZSTDMI_DCtx_getStageTimes(d.dctx, ms, names, 24)
    return {names[i].decode() for i in range(k)}


# ---------------------------------------------------------------------------------------------- one call per case and setting
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("waves", WIDTHS)
def test_every_width_walks_every_case(gpu_lib, table, waves, group):
    """exec_matches_kernel (1) and exec_matches_wide_kernel<2 .. 16>, the origin path off: the padded frames are walked too"""
    table.sweep(gpu_lib, table.group(group), settings(gpu_lib, waves=waves, long_frames=1))


def test_origin_path_on_the_padded_cases(gpu_lib, table):
    """ZSTDMI_DCtx_setLongFrames(2): every frame of 1 MiB or more by origin pointers — and it did take that path"""
    def took_it(d, e):
        if e.valid:
            assert "origin_jump" in stages(gpu_lib, d), e.name
    padded = table.group("padded")
    assert len(padded) > 50 and all(e.cap >= (1 << 20) for e in padded)
    table.sweep(gpu_lib, padded, settings(gpu_lib, long_frames=2, profiling=1), took_it)


@pytest.mark.parametrize("group", GROUPS)
def test_literal_decoder_beside_the_sequence_decoder(gpu_lib, table, group):
    """ZSTDMI_DCtx_setOverlap(2)"""
    table.sweep(gpu_lib, table.group(group), settings(gpu_lib, overlap=2))


@pytest.mark.parametrize("lit", [1, 2, 3], ids=["serial-literals", "selfsync-literals", "compact-literals"])
def test_every_literal_decoder_on_the_literal_runs(gpu_lib, table, lit):
    entries = table.group("literals")
    assert len(entries) == 44
    table.sweep(gpu_lib, entries, settings(gpu_lib, literals=lit))


# ------------------------------------------------------------------------------------------------------------- batch calls
def dictionary_free(table):
    return [e for e in table.entries if e.valid and not e.dic]


class Layout:
    """destinations of a batch carved from one poisoned tensor at odd offsets, GUARD bytes or more between them"""

    def __init__(self, table, entries, poison):
        t = table.torch
        self.table, self.entries, self.poison = table, entries, poison
        self.at, at = [], 1
        for e in entries:
            self.at.append(at)
            at = (at + e.cap + GUARD) | 1
        self.dst = t.full((at + GUARD,), poison, dtype=t.uint8, device="cuda")
        self.srcs = [table.src.data_ptr() + e.at for e in entries]
        self.dsts = [self.dst.data_ptr() + a for a in self.at]

    def check(self, got):
        """got[i]: the size entry i reported, or its error code as a negative number"""
        host = self.dst.cpu().numpy()
        rest = host.copy()
        wrong = []
        for e, a, g in zip(self.entries, self.at, got):
            if not e.valid:
                if g != -CORRUPTION:
                    wrong.append((e.name, g))
                rest[a:a + e.cap] = self.poison
                continue
            if g != e.cap or host[a:a + g].tobytes() != e.content:
                wrong.append((e.name, g))
            rest[a:a + e.cap] = self.poison
        assert not wrong, (len(wrong), wrong[:6])
        bad = np.flatnonzero(rest != self.poison)
        assert bad.size == 0, f"bytes outside the results were written, first at {bad[:4]}"


def with_a_negative(table):
    entries = dictionary_free(table)
    neg = next(e for e in table.entries if e.name == "neg_last_lane_of_batch_kb256")
    return entries[:len(entries) // 2] + [neg] + entries[len(entries) // 2:]


def test_one_batch_call_over_every_case(gpu_lib, table):
    """ZSTDMI_decompressBatch: the dictionary-free cases as entries of one call, a negative in the middle, which fails alone"""
    entries = with_a_negative(table)
    n = len(entries)
    assert n > 250
    with z.Decompressor() as d:
        for poison in POISONS:
            lay = Layout(table, entries, poison)
            got = (ctypes.c_size_t * n)()
            table.torch.cuda.synchronize()
            r = gpu_lib.ZSTDMI_decompressBatch(d.dctx, (ctypes.c_void_p * n)(*lay.srcs), (ctypes.c_size_t * n)(*[len(e.blob) for e in entries]), n,
                                               (ctypes.c_void_p * n)(*lay.dsts), (ctypes.c_size_t * n)(*[e.cap for e in entries]), got)
            assert not is_error(r), gpu_lib.ZSTD_getErrorName(r)
            lay.check([-int(get_error_code(g)) if is_error(g) else int(g) for g in got])


def test_one_async_batch_call_over_every_case(gpu_lib, table):
    """ZSTDMI_decompressBatchAsync: the same entries through the instances that take their counts from device memory"""
    t = table.torch
    entries = with_a_negative(table)
    n = len(entries)
    with z.Decompressor() as d:
        d.PrepareBatchAsync(n, max(len(e.blob) for e in entries), sum(e.cap for e in entries) + 1024 * n, n)
        for poison in POISONS:
            lay = Layout(table, entries, poison)
            cols = [t.tensor(c, dtype=t.int64, device="cuda") for c in (lay.srcs, [len(e.blob) for e in entries], lay.dsts, [e.cap for e in entries])]
            out = decompress_batch_async(d, *cols)
            t.cuda.synchronize()
            lay.check([int(x) for x in out.cpu().tolist()])


def test_every_case_in_one_call(gpu_lib, table):
    """the dictionary-free cases as one run of frames in one ZSTDMI_decompressDevice call: the call picks the width (and the path of
    the padded frames) itself"""
    t = table.torch
    entries = dictionary_free(table)
    src = t.from_numpy(np.frombuffer(b"".join(e.blob for e in entries), dtype=np.uint8).copy()).cuda()
    want = b"".join(e.content for e in entries)
    with z.Decompressor() as d:
        assert gpu_lib.ZSTDMI_DCtx_setExecWaves(d.dctx, 0) == 0
        for poison in POISONS:
            dst = t.full((len(want) + GUARD,), poison, dtype=t.uint8, device="cuda")
            t.cuda.synchronize()
            r = gpu_lib.ZSTDMI_decompressDevice(d.dctx, dst.data_ptr(), len(want), src.data_ptr(), src.numel())
            assert not is_error(r) and r == len(want), r
            host = dst.cpu().numpy()
            assert (host[len(want):] == poison).all()
            if host[:len(want)].tobytes() != want:
                at, wrong = 0, []
                for e in entries:
                    if host[at:at + e.cap].tobytes() != e.content:
                        wrong.append(e.name)
                    at += e.cap
                assert not wrong, (hex(poison), len(wrong), wrong[:8])


# ------------------------------------------------------------------------------------- the dictionary family through a DDict set
@pytest.fixture(scope="module")
def ddict_table(gpu_lib):
    """the dictionary cases forged anew behind two FORMATTED dictionaries in turn, each frame naming its dictionary's ID
    -> (table, the two DDicts)"""
    sample = bytes(range(32, 127)) * 20
    formatted = [oracle_lib.make_dictionary(E.dictionary(k), sample, DDICT_IDS[k]) for k in (0, 1)]
    cases = []
    for i, (name, tags, build, valid) in enumerate(c for c in E.CASES if E.SPECS[c[0]].dict_size):
        k = i % 2
        blob, content = E.SPECS[name].forge(history=E.dictionary(k), did=4, did_value=DDICT_IDS[k])
        cases.append((name, tags, blob, content, None))
    dds = [z.DDict(f) for f in formatted]
    assert [dd.dict_id for dd in dds] == list(DDICT_IDS)
    yield Table(cases), dds
    for dd in dds:
        dd.Dispose()


@pytest.mark.parametrize("waves,long_frames", [(w, 1) for w in WIDTHS] + [(0, 2)], ids=[f"waves{w}" for w in WIDTHS] + ["origin"])
def test_dictionary_cases_through_a_ddict_set(gpu_lib, ddict_table, waves, long_frames):
    """ZSTD_d_refMultipleDDicts with two DDicts: the kSet instances, whose dictionary part is copied by lane_copy"""
    tab, dds = ddict_table
    entries = [e for e in tab.entries if long_frames == 1 or "padded" in e.tags]
    assert len(entries) > 30 and any(not e.valid for e in tab.entries)
    with z.Decompressor() as d:
        d.SetParameter(z.ZSTD_d_refMultipleDDicts, 1)
        for dd in dds:
            d.RefDDict(dd)
        settings(gpu_lib, waves=waves, long_frames=long_frames, profiling=1)(d)
        wrong = []
        for poison in POISONS:
            for e in entries:
                w = tab.decode(gpu_lib, d, e, poison)
                if w:
                    wrong.append((e.name, hex(poison), w))
                    continue
                if e.valid:
                    assert gpu_lib.ZSTDMI_debugLastSetFrames(d.dctx) == 1, e.name
                if long_frames == 2 and e.valid:
                    assert "origin_jump" in stages(gpu_lib, d), e.name
        assert not wrong, (len(wrong), wrong[:6])
