"""CPU tests of the sequence encoder's case tables (tests/seq_cases.py): what tests/test_gpu_seq_encode.py relies on is proven here,
against the oracle and against the decoder's repcode rule, without a GPU."""
import pytest

import seq_cases as sc
import zstd_blocks as zb

# cases the oracle answers with "store raw": the GPU test compares a bare 0 for them, so they are few and each has its reason
RAW_CASES = {"widest_16384_raw": "16 384 sequences of 61 bits: the stream is longer than the block (the overflow path)"}


@pytest.fixture(scope="module")
def entropy():
    return sc.entropy_cases()


@pytest.fixture(scope="module")
def repcode():
    return sc.repcode_cases()


@pytest.fixture(scope="module")
def answers(oracle, entropy):
    """(name, strategy) -> the oracle's block"""
    out = {}
    for name, seqs, lits, src, _ in entropy:
        for st in sc.STRATEGIES:
            out[name, st] = oracle.entropy_block(seqs, lits, src, st)
    return out


def test_code_tables_are_consistent():
    for c, base in enumerate(sc.LL_BASE[:sc.MAX_LL_CODE + 1]):
        top = min(base + (1 << sc.LL_BITS[c]) - 1, 65535)
        assert sc.ll_code(base) == c == sc.ll_code(top) and (c == 0 or sc.ll_code(base - 1) == c - 1)
    for c, base in enumerate(sc.ML_BASE[:sc.MAX_ML_CODE + 1]):
        top = min(base + (1 << sc.ML_BITS[c]) - 1, 65535)
        assert sc.ml_code(base) == c == sc.ml_code(top) and (c == 0 or sc.ml_code(base - 1) == c - 1)
    for a, (max_code, _, log, _, norm) in enumerate(sc.ALPHABETS):
        assert sum(abs(n) for n in norm) == 1 << log and len(norm) == (29 if a == 1 else max_code + 1)
    assert sc.extra_bits((0xFFFFFFFF, 65535, 65535)) == 31 + 15 + 15


def test_names_are_unique_and_stores_within_the_hooks_bounds(entropy, repcode):
    for table in (entropy, repcode):
        names = [c[0] for c in table]
        assert len(set(names)) == len(names)
        for name, seqs, lits, src, _ in table:
            assert len(seqs) <= 16384 and len(lits) <= src <= 65536, name
            assert all(1 <= o < 1 << 32 and 0 <= l < 65536 and 0 <= m < 65536 for o, l, m in seqs), name
    assert all(o >= 4 for _, raw, *_ in repcode for o, _, _ in raw), "a raw offset is a distance + 3"
    assert all(len(lits) <= 63 for name, _, lits, *_ in entropy if not name.startswith("ramp_"))
    assert all(len(lits) <= 63 for _, _, lits, *_ in repcode)


# --------------------------------------------------------------------------------------------------------------- repcodes
def test_resolved_codes_decode_to_the_raw_offsets(repcode):
    """the decoder's rule, run over resolve_reps' output, gives back every distance; and a full offset is only written where no
    usable history entry equals the distance"""
    for name, raw, _, _, rep in repcode:
        hist = list(rep)
        for (code, ll, mlb), (off_base, ll_raw, mlb_raw) in zip(sc.resolve_reps(raw, rep), raw):
            assert (ll, mlb) == (ll_raw, mlb_raw)
            ll0 = ll == 0
            if code > 3:
                usable = [hist[1], hist[2], hist[0] - 1 if hist[0] > 1 else 0] if ll0 else hist
                assert code - 3 not in [h for h in usable if h], (name, "a full offset where a repcode would do")
            off, hist = sc.history_after(code, ll0, hist)
            assert off == off_base - 3 and off > 0, name


def test_every_kind_of_hit_meets_the_batch_edges(repcode):
    """each of the seven kinds at the first and at the last lane of a 64-sequence batch, and in a batch other than the first"""
    where = {k: set() for k in sc.KINDS}
    for _, raw, _, _, rep in repcode:
        for i, kind in enumerate(sc.classify(raw, rep)):
            if kind: where[kind].add(i)
    for kind, idx in where.items():
        assert any(i % 64 == 0 for i in idx) and any(i % 64 == 63 for i in idx) and any(i >= 64 for i in idx), kind
    named = {name: (raw, rep) for name, raw, _, _, rep in repcode}
    for kind in sc.KINDS:
        for at in (0, 1, 62, 63, 64, 65, 127, 128):
            raw, rep = named[f"{kind}@{at}"]
            assert sc.classify(raw, rep)[at] == kind
    for n, swap in ((64, 67), (130, 133), (61, 64), (125, 128)):
        raw, rep = named[f"carried_{n}"]
        kinds = sc.classify(raw, rep)
        assert kinds[3:swap] == ["rep0"] * n and kinds[swap:swap + 2] == ["rep1", "rep2"]
        raw, rep = named[f"carried_ll0_{n}"]
        assert sc.classify(raw, rep)[swap:swap + 3] == ["ll0_rep1", "ll0_rep2", "ll0_rep0m1"]
    raw, rep = named["rep0m1_rep0_is_1"]
    assert [c for c, _, _ in sc.resolve_reps(raw, rep)].count(3) == 0 and sum(1 for _, ll, _ in raw if ll == 0) == 4
    assert {rep for name, _, _, _, rep in repcode if name.startswith("random_")} == {(0, 0, 0), (1, 4, 8), (700, 40, 9)}
    sizes = [len(raw) for name, raw, *_ in repcode if name.startswith("random_")]
    assert len(sizes) == 200 and min(sizes) >= 1 and max(sizes) <= 400 and max(sizes) > 256


# --------------------------------------------------------------------------------------------------------------- entropy
def test_the_oracle_answers_every_entropy_case(entropy, answers):
    for name, seqs, _, _, exp in entropy:
        for st in sc.STRATEGIES:
            got = answers[name, st]
            assert not isinstance(got, int), (name, st, got)
            assert (got == b"") == bool(exp.get("raw")) == ("raw" in name.split("_")), (name, st, len(got))
    raw = {name for (name, _), got in answers.items() if got == b""}
    assert raw == set(RAW_CASES), "only the named cases may come out 'store raw'"


def test_mode_bytes_literal_types_and_sizes_are_the_ones_named(entropy, answers):
    named = 0
    for name, seqs, lits, _, exp in entropy:
        for st in sc.STRATEGIES:
            got = answers[name, st]
            if not got: continue
            lit_type, nb_seq, mode_byte = zb.parse_block(got)
            assert nb_seq == len(seqs), name
            if seqs:
                modes = zb.modes_of(mode_byte)
                assert mode_byte & 3 == 0 and modes == sc.modes_by_rule(seqs)[st], (name, st, modes)
                if "modes" in exp:
                    assert modes == exp["modes"][st], (name, st, modes); named += 1
            assert lit_type == exp.get("lits", 0), (name, st, lit_type)
            if "size" in exp: assert len(got) == exp["size"], (name, len(got))
    assert named > 200
    by_name = {name: seqs for name, seqs, *_ in entropy}
    # the thresholds flip where the rule says, for every strategy, on the oracle itself
    for st, ll_min, of_min in ((1, 72, 36), (2, 64, 32), (3, 56, 28)):
        for n in (27, 28, 31, 32, 35, 36, 55, 56, 63, 64, 71, 72):
            ll, of, ml = zb.modes_of(zb.parse_block(answers[f"threshold_flat_{n}", st])[2])
            assert (ll, of, ml) == (0 if n < ll_min else 2, 0 if n < of_min else 2, 0 if n < ll_min else 2), (st, n)
    # all codes equal: predefined up to two sequences, RLE above; offset codes above 28 are never predefined
    for n in (1, 2, 3, 200):
        assert zb.modes_of(zb.parse_block(answers[f"equal_all_{n}", 1])[2]) == ((0, 0, 0) if n <= 2 else (1, 1, 1))
    for code in (29, 30, 31):
        for n in (2, 3, 200):
            assert zb.modes_of(zb.parse_block(answers[f"of{code}_equal_{n}", 1])[2])[1] == 1
            assert zb.modes_of(zb.parse_block(answers[f"of{code}_mixed_{n}", 1])[2])[1] == 2
    for name, alphabet, codes in (("ml_0_51", 2, {0, 51}), ("of_0_31", 1, {0, 31}), ("ll_0_34", 0, {0, 34})):
        assert {sc.codes_of(s)[alphabet] for s in by_name[name]} == codes
        assert zb.modes_of(zb.parse_block(answers[name, 1])[2])[alphabet] == 2
    for name, times in (("last_code_once", 1), ("last_code_twice", 2)):
        last = sc.codes_of(by_name[name][-1])
        for a in range(3):
            assert sum(1 for s in by_name[name] if sc.codes_of(s)[a] == last[a]) == times


def test_description_branches_are_the_ones_named(entropy):
    seen = set()
    for name, seqs, _, _, exp in entropy:
        if "branch" not in exp: continue
        alphabet, label = exp["branch"]
        for st in sc.STRATEGIES:
            mode, _, _, labels = sc.plan_table(seqs, alphabet, st)
            assert mode == 2 and label in labels, (name, st, labels)
            assert ("M2" in labels) == label.startswith("M2"), (name, labels)
            seen |= labels
    main = [name for name, seqs, _, _, exp in entropy if exp.get("branch", (0, ""))[1] == "M2-main"]
    assert len(main) >= 3
    assert {"low+1", "low-1", "rtb-up", "primary-negative", "M2-main", "M2-second-pass", "M2-total-zero"} <= seen
    assert not set(sc.M2_NOT_FOUND) & seen
    by_name = {name: seqs for name, seqs, *_ in entropy}
    for n1 in (2047, 2048, 2049):        # the switch is on the count without the last sequence
        assert len(by_name[f"lowprob_{n1}"]) == n1 + 1


def test_bit_counts_follow_the_oracle_and_meet_every_alignment(entropy, answers):
    """the Python-side bit counts are exact (checked on every block that describes no table, where the stream's size can be read off
    the oracle's block), every lane shift 0..31 occurs in the drawn-width stores, and every count of carried bits in the carry ones"""
    checked = 0
    for name, seqs, lits, _, _ in entropy:
        if not seqs or len(seqs) > 300: continue
        for st in sc.STRATEGIES:
            got = answers[name, st]
            modes = zb.modes_of(zb.parse_block(got)[2])
            if 2 in modes: continue
            head = zb.literals_of(got)[2] + (1 if len(seqs) < 128 else 2) + 1 + modes.count(1)
            assert sc.bitstream_bytes(seqs, st) == len(got) - head, (name, st); checked += 1
    assert checked > 100
    widest = [(0xFFFFFFFF, 65535, 65535)] * 64
    assert sc.field_bits(widest, 1)[0] == [61] * 64              # (one code per alphabet: RLE tables, whose states emit nothing)
    for st in sc.STRATEGIES:
        lanes, carried = set(), set()
        for name, seqs, *_ in entropy:
            if name.startswith("widths_"): lanes |= sc.lane_alignments(seqs, st)
            if name.startswith("carry_"):
                assert len(seqs) == 80
                carried.add(sc.carry_alignments(seqs, st)[0])
        assert lanes == set(range(32)) and carried == set(range(32)), st
