"""The match-execution case table (tests/exec_cases.py) on the CPU: every frame decodes under the oracle to what the forge's serial
executor makes of it, every negative is refused, and every case is what its name says — recomputed here from the sequence list, with
the executors' dependency rule written out in exec_cases.rounds.  No GPU.  tests/test_gpu_exec_cases.py is the GPU side."""
import pytest

import exec_cases as E
import zstd_forge as F

BY_NAME = {c[0]: c for c in E.CASES}
# a family may leave out a batch size only where the 128 KiB block limit makes it impossible to write: none does
LEFT_OUT = {}


def tagged(tag):
    return [c[0] for c in E.CASES if tag in c[1]]


def test_every_valid_case_decodes_under_the_oracle(oracle):
    n = 0
    for name, tags, build, valid in E.CASES:
        if not valid:
            continue
        blob, content, dic = build()
        assert content is not None
        assert oracle.decompress(blob, len(content), dic) == content, name
        n += 1
    assert n > 300


def test_dictionary_cases_need_their_dictionary(oracle):
    """a dictionary case decoded without the dictionary, or behind another one, does not give its content"""
    for name in tagged("dict"):
        blob, content, dic = BY_NAME[name][2]()
        assert dic == E.dictionary() and len(dic) == E.DICT_SIZE
        assert oracle.decompress(blob, len(content)) != content, name
        assert oracle.decompress(blob, len(content), E.dictionary(1)) != content, name


def test_formatted_dictionary_frames_decode_under_the_oracle(oracle):
    """the frames the refMultipleDDicts test decodes: a dictionary ID in the header, the history a formatted dictionary's content"""
    sample = bytes(range(32, 127)) * 20
    for which, did in ((0, 4242), (1, 777777)):
        content_d = E.dictionary(which)
        formatted = oracle.make_dictionary(content_d, sample, did)
        assert formatted.endswith(content_d)
        for name in tagged("dict")[which::7]:
            blob, content = E.SPECS[name].forge(history=content_d, did=4, did_value=did)
            at = 5 if blob[4] & 0x20 else 6                 # (behind the window descriptor of a frame that is not single-segment)
            assert int.from_bytes(blob[at:at + 4], "little") == did and blob[4] & 3 == 3, name
            assert oracle.decompress(blob, len(content), formatted) == content, name


def test_the_oracle_refuses_every_negative(oracle):
    negs = [c for c in E.CASES if not c[3]]
    assert len(negs) >= 10 and all("negative" in c[1] for c in negs)
    for name, tags, build, valid in negs:
        blob, content, dic = build()
        assert content is None
        assert isinstance(oracle.decompress(blob, 2 << 20, dic), int), name
        # one byte nearer the frame is valid: the offset alone makes it a negative
        spec = E.SPECS[name]
        i, ov = spec.fix
        d, ml, off, ll = E.layout(spec.seqs())[i]
        assert off == spec.block_start() + d + spec.dict_size + 1, name


def test_chain_depth_is_the_batch_size():
    """every batch of a chain is as deep as it has sequences (two interleaved chains: half of that), so the first batch of a block of
    at least kB sequences is exactly kB deep at its kB"""
    for name in tagged("chain"):
        spec = E.SPECS[name]
        n, kB = len(spec.seqs()), spec.kB
        counts = [min(kB, n - b) for b in range(0, n, kB)]
        want = counts if spec.claim["depth"] == "full" else [(c + 1) // 2 for c in counts]
        assert E.rounds(spec.seqs(), kB, spec.block_start()) == want, name
        if n >= kB:
            assert want[0] == (kB if spec.claim["depth"] == "full" else kB // 2)
    for kB in E.KB:
        assert {len(E.SPECS[n].seqs()) for n in tagged("chain") if E.SPECS[n].kB == kB} == {kB - 1, kB, kB + 1, 2 * kB + 1}


def test_touch_pairs_differ_in_one_offset_and_in_one_round():
    for name in tagged("touch"):
        spec = E.SPECS[name]
        if spec.padded:
            continue
        cl, kB = spec.claim, spec.kB
        seqs, lay, start = spec.seqs(), E.layout(spec.seqs()), spec.block_start()
        assert len(seqs) == kB and E.rounds(seqs, kB, start) == [2 if cl["dep"] else 1], name
        p, c = cl["p"], cl["c"]
        _, lo, hi = E.source(lay[c], start)
        start_p, end_p = lay[p][0], lay[p][0] + lay[p][1]
        assert {"hi_eq": hi == start_p, "hi_plus1": hi == start_p + 1, "lo_eq": lo == end_p, "lo_minus1": lo == end_p - 1}[cl["rel"]], name
        # the producer is slow (the whole wave's copy, or a byte loop at a distance below 8), the consumer fast
        assert lay[p][1] > 64 or (lay[p][2] < 8 and lay[p][1] > 56), name
        assert 3 <= lay[c][1] <= 8 and lay[c][2] >= lay[c][1], name
        other = E.SPECS[cl["pair"]]
        assert other.claim["dep"] != cl["dep"] and other.claim["pair"] == name
        diff = [(a, b) for a, b in zip(seqs, other.seqs()) if a != b]
        assert len(diff) == 1 and diff[0][0][0] == diff[0][1][0] and diff[0][0][2] == diff[0][1][2] and abs(diff[0][0][1] - diff[0][1][1]) == 1, name
        assert [b for i, b in enumerate(spec.blocks) if i != spec.cb] == [b for i, b in enumerate(other.blocks) if i != other.cb]
        assert spec.blocks[spec.cb]["lit"] == other.blocks[other.cb]["lit"], name
    for kB in E.KB:
        places = {(E.SPECS[n].claim["p"], E.SPECS[n].claim["c"]) for n in tagged("touch") if E.SPECS[n].kB == kB}
        assert {(10, 11), (0, 63)} <= places
        if kB > 64:
            assert {(kB - 65, kB - 64), (0, kB - 1)} <= places


def test_span_cases_wait_for_the_lanes_they_name():
    for name in tagged("span"):
        spec = E.SPECS[name]
        cl = spec.claim
        seqs, lay, start = spec.seqs(), E.layout(spec.seqs()), spec.block_start()
        assert E.rounds(seqs, spec.kB, start) == cl["rounds"], name
        _, lo, hi = E.source(lay[cl["c"]], start)
        ends, starts = [d + ml for d, ml, _, _ in lay], [d for d, _, _, _ in lay]
        assert sum(e <= lo for e in ends[:cl["c"]]) == cl["jl"] and sum(s < hi for s in starts[:cl["c"]]) == cl["jh"], name
        if cl["jh"] == cl["jl"]:         # literals only, between two match outputs, touching both
            assert lo == ends[cl["jl"] - 1] and hi == starts[cl["jl"]], name


def test_block_edge_cases_lie_where_they_say():
    for name in tagged("block-edge"):
        spec = E.SPECS[name]
        cl, kB = spec.claim, spec.kB or 64
        seqs, lay, start = spec.seqs(), E.layout(spec.seqs()), spec.block_start()
        assert spec.cb == 1 and spec.blocks[0]["t"] == "raw" and start == E.FRONT
        assert E.rounds(seqs, kB, start) == cl["rounds"], name
        i = cl["seq"]
        _, lo, hi = E.source(lay[i], start)
        if cl["rel"] == "ends_at_start":
            assert lo < 0 and hi == 0
        elif cl["rel"] == "straddles":
            assert lo < 0 < hi
        elif cl["rel"] == "starts_at_start":
            assert lo == 0 < hi
        elif cl["rel"] == "inside_previous":
            assert i == kB and hi == lay[i - 1][0] + lay[i - 1][1] and lo >= lay[i - 1][0] and lay[i - 1][1] > 64
        else:
            assert cl["rel"] == "straddles_batches" and i == kB + 2
            assert lo == lay[kB - 2][0] and hi == lay[kB + 1][0] + lay[kB + 1][1]
    for kB in E.KB:
        assert sum(1 for n in tagged("block-edge") if E.SPECS[n].kB == kB) == 2


def test_copy_sweep_holds_every_pair_and_no_dependency():
    seen = []
    for name in tagged("copy-sweep"):
        spec = E.SPECS[name]
        if spec.padded:
            continue
        for d, ml, off, ll in E.layout(spec.seqs()):
            assert ll == off
            seen.append((ml, off))
        for kB in E.KB:
            assert set(E.rounds(spec.seqs(), kB, spec.block_start())) == {1}, name
    assert seen == E.sweep_pairs() and len(seen) == len(set(seen))
    for ml in E.SWEEP_ML:
        assert {off for m, off in seen if m == ml} >= set(E.SWEEP_OFF) | {ml - 1, ml, ml + 1}


def test_literal_cases_have_the_runs_they_say():
    kinds = {"raw": {"k": "raw"}, "rle": {"k": "rle"}, "huf": {"k": "huf", "streams": 4}, "treeless": {"k": "treeless", "streams": 4}}
    seen = set()
    for name in tagged("literals"):
        spec = E.SPECS[name]
        cl, blk = spec.claim, spec.blocks[spec.cb]
        assert all(blk["lit"][k] == v for k, v in kinds[cl["kind"]].items()), name
        lls = [s[0] for s in blk["seqs"]]
        if "runs" in cl:
            assert tuple(lls) == E.LIT_RUNS
        if "pieces" in cl:
            # place_literals_kernel: the runs above 32 bytes of one batch of 64, in 16-byte pieces
            assert len(lls) == 64 and sum((ll + 15) // 16 for ll in lls if ll > 32) == cl["pieces"], name
        if "trailing" in cl:
            assert len(blk["lit"]["data"]) - sum(lls) == cl["trailing"], name
        seen.add((cl["kind"], next(k + str(cl[k]) if k != "runs" else k for k in ("runs", "pieces", "trailing") if k in cl)))
    assert len(seen) == 4 * (1 + len(E.LIT_PIECES) + len(E.LIT_TRAILING))


def test_dict_cases_reach_as_far_as_they_say():
    backs = set()
    for name in tagged("dict"):
        spec = E.SPECS[name]
        cl = spec.claim
        lay, start = E.layout(spec.seqs()), spec.block_start()
        assert start == (E.PAD if spec.padded else 0) and spec.dict_size == E.DICT_SIZE
        q = lay[cl.get("seq", 1)]
        d, ml, off, _ = q
        dict_n, lo, hi = E.source(q, start)
        assert off - (start + d) == cl["back"] and dict_n == cl["dict_n"] and ml - dict_n == cl["rest"], name
        assert cl["back"] <= E.DICT_SIZE and (cl["rest"] == 0 or (start + lo, start + hi) == (0, cl["rest"]))          # what is left continues at the frame's first byte
        backs.add((cl["back"], cl["rest"]))
        assert (d < hi) == cl.get("holds_itself", False), name          # the source interval reaches over the match's own start
        if "reader" in cl:
            _, rlo, rhi = E.source(lay[cl["reader"]], start)
            assert (rlo, rhi) == (d, d + dict_n) and E.rounds(spec.seqs(), 64, start) == cl["rounds"], name
    assert {b for b, _ in backs} >= {1, 63, 64, 65, E.DICT_SIZE} and {r for _, r in backs} == {0, 1, 30, 100}
    assert (E.DICT_SIZE, 0) in backs and (E.DICT_SIZE, 100) in backs          # off == position + dictSize exactly


@pytest.mark.parametrize("tag", E.PER_KB)
def test_every_batch_size_has_its_cases(tag):
    for kB in E.KB:
        if (tag, kB) not in LEFT_OUT:
            assert any(E.SPECS[n].kB == kB for n in tagged(tag)), (tag, kB)
    for kB in E.KB:
        assert any(E.SPECS[n].kB == kB and not E.SPECS[n].padded for n in tagged("negative")), kB
    assert all(tagged(t) for t in E.TAGS)


def test_sizes_and_padding():
    for name, tags, build, valid in E.CASES:
        spec = E.SPECS[name]
        assert spec.padded == ("padded" in tags) == name.endswith("_padded") or name.startswith("pad_"), name
        if not valid:
            continue
        n = len(build()[1])
        if spec.padded:
            assert (1 << 20) <= n <= int(1.2 * (1 << 20)), name
            assert build()[1][:E.PAD] == b"".join(bytes([b["byte"]]) * b["size"] for b in spec.all_blocks()[:E.PAD_BLOCKS])
        else:
            assert n <= F.BLOCK_MAX, name
    # what the issue asks to be padded
    padded = set(tagged("padded"))
    assert {n + "_padded" for n in tagged("chain") if E.SPECS[n].kB == 1024 and not E.SPECS[n].padded} <= padded
    assert all(any(E.SPECS[n].kB == kB for n in padded if n.startswith("touch_")) for kB in E.KB)
    assert {n + "_padded" for n in tagged("span") + tagged("dict") if not E.SPECS[n].padded and "holds_itself" not in E.SPECS[n].claim} <= padded
    assert {"copy_sweep_0_padded", "pad_copy_from_1mib_back", "pad_offset_1_whole_block"} <= padded and any(n.startswith("neg_") for n in padded)
    assert E.SPECS["pad_copy_from_1mib_back"].seqs() == [(0, (1 << 20) + 3, 131072)] and E.SPECS["pad_offset_1_whole_block"].seqs() == [(0, 1 + 3, 131072)]


def test_the_table_is_deterministic():
    name = "touch_wave_seam_bytewise_lo_minus1_kb256"
    assert E.SPECS[name].forge() == E.SPECS[name].forge() == BY_NAME[name][2]()[:2]
