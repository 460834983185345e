"""CPU tests of the Huffman table build's case table (tests/huf_cases.py): what tests/test_gpu_huf_tree.py relies on is proven here,
against the oracle, without a GPU: the Python model of HUF_sort / HUF_buildTree / HUF_setMaxHeight gives the oracle's lengths, every
case takes the branches and meets the figures it claims, and the oracle's verdict on every case is the one named."""
import collections
import ctypes
import random

import pytest

import huf_cases as hc
import zstd_blocks as zb

# cases the oracle answers with "store raw": the GPU test compares a bare 0 for them, which says nothing about the tree, so they are
# few, each is one side of a verdict's threshold, and each names the neighbour on the compressed side
RAW_CASES = {
    "desc_equal_192_raw": "192 described weights, all equal: not FSE-codable (one symbol) and too many for the 4-bit form, HUF_writeCTable fails",
    "desc_equal_224_raw": "224 described weights, all equal: HUF_writeCTable fails",
    "verdict_largest_12_raw": "largest == (n >> 7) + 4: HUF_compress does not try",
    "verdict_sample_68_raw": "a suspect block of 40 960 literals whose two 4 KiB samples hold no frequent byte (34 + 34 <= 68)",
    "verdict_size_63_raw": "63 literals and fewer are never Huffman-coded",
}


class Row:
    """one case with everything the tests look at, computed once"""

    def __init__(self, oracle, name, lits, exp):
        self.name, self.lits, self.exp = name, lits, exp
        cnt = collections.Counter(lits)
        self.hist = [cnt.get(s, 0) for s in range(max(cnt) + 1)]
        self.n, self.src = len(lits), exp.get("src", len(lits))
        self.answer = oracle.entropy_block([], lits, self.src, 1)
        self.rle = len(cnt) == 1
        if not self.rle:
            self.max_bits, self.max_sv = hc.plan(self.hist)
            self.nb, self.log, self.labels = hc.lengths(self.hist, self.max_bits)


@pytest.fixture(scope="module")
def rows(oracle):
    return [Row(oracle, *c) for c in hc.cases()]


def _oracle_lengths(oracle, hist, max_bits):
    out = ctypes.create_string_buffer(256)
    r = oracle.lib().zso_huf_buildLengths(out, (ctypes.c_uint32 * 256)(*hist), len(hist) - 1, max_bits)
    assert not oracle.is_error(r), r
    return list(out.raw[:len(hist)]), r


def _kraft_is_one(nb, log):
    return sum(1 << (log - b) for b in nb if b) == 1 << log


def _frame_of(body, size):
    """one compressed block as a whole frame: single segment, 4-byte content size, no checksum"""
    return zb.MAGIC + bytes([0xA0]) + size.to_bytes(4, "little") + (1 + (2 << 1) + (len(body) << 3)).to_bytes(3, "little") + body


def test_names_are_unique_and_sizes_within_the_hooks_bounds(rows):
    names = [r.name for r in rows]
    assert len(set(names)) == len(names) and 80 <= len(names) <= 300
    for r in rows:
        assert 1 <= r.n <= r.src <= 65536, r.name
    # no histogram larger than it needs: only the log2 buckets (counts >= 165 over 200 symbols), the depths a small block cannot
    # reach, the 40 960-byte sample and the header's size steps take more than 16 KiB
    large = {r.name for r in rows if r.n > 16384}
    assert all(n.startswith(("sort_bucket_2", "sort_ties_", "len_fib_2", "verdict_sample_", "desc_equal_")) or n == "verdict_size_16384" for n in large), large
    assert sum(1 for r in rows if r.n <= 4096) > len(rows) * 2 // 3


def test_optimal_table_log_restated():
    for n, max_sv, want in ((64, 1, 5), (64, 255, 7), (69, 12, 5), (256, 6, 6), (1024, 85, 8), (1025, 255, 9), (4096, 39, 10), (4097, 255, 11), (65536, 255, 11), (98, 65, 7)):
        assert hc.optimal_table_log(11, n, max_sv) == want, (n, max_sv)


def test_model_gives_the_oracles_lengths(oracle, rows):
    """on every case, and on seeded random histograms of the shapes the cases were searched among"""
    hists = [(r.name, r.hist) for r in rows if not r.rle]
    rng = random.Random(11)
    for i in range(400):
        hist = [rng.choice((0, 1, 1, 2, 3, 1 << rng.randrange(10), rng.randrange(1, 300))) for _ in range(rng.randrange(2, 257))]
        while hist and not hist[-1]: hist.pop()
        if sum(1 for c in hist if c) >= 2 and 64 <= sum(hist) <= 65536: hists.append((f"random_{i}", hist))
    assert len(hists) > 400
    for name, hist in hists:
        max_bits, max_sv = hc.plan(hist)
        nb, log, _ = hc.lengths(hist, max_bits)
        want_nb, want_log = _oracle_lengths(oracle, hist, max_bits)
        assert nb == want_nb and log == want_log, (name, [(s, a, b) for s, (a, b) in enumerate(zip(nb, want_nb)) if a != b][:4], log, want_log)
        assert _kraft_is_one(nb, log) and max(nb) == log <= max_bits, name
        assert all((b > 0) == (c > 0) for b, c in zip(nb, hist)), name


def test_cases_take_the_branches_and_meet_the_figures_they_claim(rows):
    union, figures, logs = set(), collections.Counter(), {"clamp": set(), "no-clamp": set()}
    for r in rows:
        if r.rle: continue
        for label in r.exp.get("labels", ()):
            assert label in r.labels, (r.name, label, sorted(r.labels))
        for label, least in r.exp.get("min", {}).items():
            assert r.labels.get(label, 0) >= least, (r.name, label, r.labels.get(label))
        if "log" in r.exp: assert r.log == r.exp["log"], (r.name, r.log)
        if "maxsv" in r.exp: assert r.max_sv == r.exp["maxsv"], r.name
        assert ("clamp" in r.labels) != ("no-clamp" in r.labels), r.name
        if r.answer:                       # (a raw answer shows the GPU test nothing of the tree: it does not count)
            union |= set(r.labels)
            for k, v in r.labels.items(): figures[k] = max(figures[k], v)
            logs["clamp" if "clamp" in r.labels else "no-clamp"].add(r.log)
    assert set(hc.REQUIRED_LABELS) <= union, set(hc.REQUIRED_LABELS) - union
    for label, least in hc.REQUIRED_FIGURES.items():
        assert figures[label] >= least, (label, figures[label])
    assert logs["clamp"] >= set(range(5, 12)) and logs["no-clamp"] >= set(range(5, 12)), logs
    by_name = {r.name: r for r in rows}
    # the two forms of the overshoot, each without the other; the long ones
    assert "overshoot-no-rank1" not in by_name["len_step_down"].labels and "overshoot-rank1" in by_name["len_step_down"].labels
    assert by_name["len_overshoot_31"].labels["overshoot"] >= 8 and by_name["len_repay_37"].labels["repay"] >= 30
    assert by_name["len_fib_22"].labels["depth"] == 21 and by_name["len_tail_204"].labels["tail"] >= 200


# one comparison of the model flipped at a time (the text to find in huf_cases.py, its replacement) -> cases that must notice
FLIPS = (
    ("if cnt[high_pos] <= 2 * cnt[low_pos]:", "if cnt[high_pos] < 2 * cnt[low_pos]:", ("len_high_cheaper", "len_pow2_8")),
    ("if a[j][0] > pivot:", "if a[j][0] >= pivot:", ("sort_bucket_210_equal", "sort_seam_164_165", "sort_ties_250_of_7")),
    ("while j >= low and a[j][0] < key[0]:", "while j >= low and a[j][0] <= key[0]:", ("sort_ties_8_of_3", "sort_ties_11_of_7")),
    ("if high - low < 8:", "if high - low < 9:", ("sort_ties_9_of_2", "sort_ties_9_of_7", "sort_ties_19_of_2", "sort_ties_64_of_7")),
    ("if high - low < 8:", "if high - low < 7:", ("sort_ties_8_of_3", "sort_ties_25_of_3")),
    ("if idx - low < high - idx:", "if idx - low <= high - idx:", ("sort_ties_10_of_3", "sort_ties_11_of_7", "sort_ties_17_of_2")),
    ("if cnt[low_s] < cnt[low_n]: picks", "if cnt[low_s] <= cnt[low_n]: picks", ("len_high_cheaper", "len_rank_at_0")),
    ("for n in range(165, 191):", "for n in range(166, 191):", ("sort_seam_164_165",)),
    ("if nb[rank_last[d]] != max_bits - d:", "if False:", ("len_low_missing", "len_step_down")),
    ("nb[rank_last[1] + 1] -= 1", "nb[rank_last[1]] -= 1", ("len_step_down", "len_overshoot_31")),
    ('hit("low-missing"); break', 'hit("low-missing"); d -= 1; continue', ("len_geo_2.05_5",)),
    ('hit("high-missing"); d -= 1; continue', 'hit("high-missing"); break', ("len_high_missing", "len_repay_37")),
    ("src_bits = highbit(n - 1) - 1", "src_bits = highbit(n - 1) - 2", ("len_fib_10", "len_fib_18")),
)


def test_a_model_with_one_comparison_flipped_is_caught_by_named_cases(oracle, rows):
    """the table would catch the same slip in the kernel: each flip changes the lengths of the cases named (and of no RLE case)"""
    import types
    source = open(hc.__file__).read()
    by_name = {r.name: r for r in rows}
    for old, new, names in FLIPS:
        assert source.count(old) == 1, old
        flipped = types.ModuleType("huf_cases_flipped")
        exec(compile(source.replace(old, new), hc.__file__, "exec"), flipped.__dict__)
        for name in names:
            r = by_name[name]
            assert r.answer, name                                  # (a case the GPU test sees Huffman-coded)
            try:
                got = flipped.lengths(r.hist, flipped.plan(r.hist)[0])[:2]
            except (IndexError, TypeError, KeyError):
                continue                                           # (a flip that walks off the ranks is caught as well)
            assert got != (r.nb, r.log), (old, name)


def test_sort_cases_are_what_their_names_say(rows):
    by_name = {r.name: r for r in rows}
    in_bucket = lambda r: [c for c in r.hist if 165 <= c <= 255]
    for name in ("sort_bucket_250", "sort_bucket_210", "sort_bucket_210_ascending", "sort_bucket_210_descending", "sort_bucket_210_equal"):
        r = by_name[name]
        assert len(in_bucket(r)) == r.labels["bucket"] >= 128 and r.answer, name
    asc, desc, eq = (in_bucket(by_name[f"sort_bucket_210_{k}"]) for k in ("ascending", "descending", "equal"))
    assert asc == sorted(asc) and len(set(asc)) > 50 and desc == sorted(desc, reverse=True) and len(set(desc)) > 50 and len(set(eq)) == 1
    assert by_name["sort_bucket_250"].labels["qs-depth"] >= 5 and by_name["sort_bucket_210"].labels["qs-depth"] >= 4
    assert by_name["sort_bucket_210_equal"].labels["qs-partitions"] == 209          # the degenerate partition: one symbol a step
    for r in rows:
        if r.name.startswith("sort_ties_"):
            k, mod = int(r.name.split("_")[2]), int(r.name.split("_")[4])
            assert len(in_bucket(r)) == k == r.labels["bucket"] and len(set(in_bucket(r))) == mod and r.answer, r.name
    assert "insertion-8" in by_name["sort_ties_8_of_3"].labels and "insertion-9-partitioned" in by_name["sort_ties_9_of_2"].labels
    assert "insertion-8" in by_name["sort_bucket_8"].labels and "qs-partitions" not in by_name["sort_bucket_8"].labels
    assert "insertion-9-partitioned" in by_name["sort_bucket_9"].labels and by_name["sort_bucket_9"].labels["qs-partitions"] >= 1
    seam = by_name["sort_seam_164_165"]
    assert seam.hist.count(164) == seam.labels["bucket-164"] == 20 and seam.hist.count(165) == seam.labels["bucket"] == 20
    assert hc.get_index(164) == 164 and hc.get_index(165) == 165 and hc.get_index(255) == 165 and hc.get_index(256) == 166
    assert by_name["sort_two_symbols"].hist == [40, 24]
    far = by_name["sort_two_symbols_0_255"].hist
    assert len(far) == 256 and far[0] and far[255] and not any(far[1:255])
    assert {r.max_sv for r in rows if r.name.startswith("sort_maxsv_")} == {1, 63, 64, 127, 128, 129, 254, 255}
    for max_sv in (63, 64, 127, 128, 129, 254, 255):
        assert all(by_name[f"sort_maxsv_{max_sv}"].hist) and sum(1 for c in by_name[f"sort_maxsv_{max_sv}_holes"].hist if c) == 3


def test_the_oracles_verdict_on_every_case_is_the_one_named(oracle, rows):
    by_name = {r.name: r for r in rows}
    kinds = collections.Counter()
    for r in rows:
        got, exp = r.answer, r.exp
        assert not isinstance(got, int), (r.name, got)
        assert (got == b"") == bool(exp.get("raw")) == r.name.endswith("_raw"), (r.name, len(got))
        if "pair" in exp:
            assert exp["pair"] in by_name, r.name
        if not got:
            pair = by_name[exp["pair"]]                  # a raw answer has a neighbour that is Huffman-coded
            assert pair.answer and zb.literals_of(pair.answer)[0] == 2, r.name
            continue
        lit_type, regen, size = zb.literals_of(got)
        assert lit_type == exp.get("lits", 2) and regen == r.n and len(got) == size + 1 and got[size] == 0, (r.name, lit_type)
        if lit_type != 2: continue
        fmt = (got[0] >> 2) & 3
        streams, lh = (1 if fmt == 0 else 4), (3, 3, 4, 5)[fmt]
        assert streams == (1 if r.n < 256 else 4) and lh == 3 + (r.n >= 1024) + (r.n >= 16384), r.name
        assert streams == exp.get("streams", streams) and lh == exp.get("lh", lh), (r.name, streams, lh)
        hdr = got[lh]
        if "hdr" in exp:
            assert (hdr < 128) if exp["hdr"] == "fse" else hdr == exp["hdr"], (r.name, hdr)
        if "csize" in exp: assert size - lh == exp["csize"], (r.name, size - lh)
        kinds["fse" if hdr < 128 else ("raw4-odd" if (hdr - 127) & 1 else "raw4-even")] += 1      # hdr - 127 weights = maxSymbolValue
        # the description, read back, holds the model's lengths
        weights = ctypes.create_string_buffer(256)
        nsym, log, ranks = ctypes.c_uint32(0), ctypes.c_uint32(0), (ctypes.c_uint32 * 16)()
        used = oracle.lib().zso_huf_readStats(weights, ctypes.byref(nsym), ctypes.byref(log), ranks, got[lh:], len(got) - lh)
        assert not oracle.is_error(used) and nsym.value == r.max_sv + 1 and log.value == r.log, r.name
        assert [log.value + 1 - w if w else 0 for w in weights.raw[:nsym.value]] == r.nb, r.name
    assert {r.name for r in rows if r.answer == b""} == set(RAW_CASES), "only the named cases may come out 'store raw'"
    assert kinds["fse"] > 20 and kinds["raw4-odd"] > 5 and kinds["raw4-even"] > 5, kinds
    # the descriptions named for their weights
    for name, hdr in (("desc_equal_32", 159), ("desc_equal_64", 191), ("desc_equal_128", 255)):
        r = by_name[name]
        assert len(set(r.nb[:-1])) == 1 and r.max_sv <= 128 and r.answer[(3, 3, 4, 5)[(r.answer[0] >> 2) & 3]] == hdr == 127 + r.max_sv
    for name in ("desc_equal_192_raw", "desc_equal_224_raw"):
        r = by_name[name]
        assert len(set(r.nb[:-1])) == 1 and r.max_sv > 128
        # (Huffman would be "compressed enough" by far, a description of the largest size included: the failure alone decides)
        assert sum(b * c for b, c in zip(r.nb, r.hist)) // 8 + 6 + 4 + 128 < r.n - hc.min_gain(r.n) - 1000
    once = by_name["desc_weights_once"]
    assert len(set(once.nb[:-1])) == len(once.nb) - 1
    # 255 weights of six values: the longest weight stream in the table, over 600 bits for the two chains to place
    longest = by_name["desc_fse_255_weights"]
    assert longest.max_sv == 255 and len(set(longest.nb)) >= 6 and longest.answer[4] > 80
    assert longest.answer[4] == max(r.answer[(3, 3, 4, 5)[(r.answer[0] >> 2) & 3]] for r in rows if r.answer and r.answer[0] & 3 == 2 and r.answer[(3, 3, 4, 5)[(r.answer[0] >> 2) & 3]] < 128)


def test_verdict_pairs_sit_on_both_sides_of_their_thresholds(rows):
    by_name = {r.name: r for r in rows}
    low, high, in_64k = by_name["verdict_largest_12_raw"], by_name["verdict_largest_13"], by_name["verdict_largest_12_in_64k"]
    assert low.n == high.n == 1024 and max(low.hist) == (1024 >> 7) + 4 and max(high.hist) == (1024 >> 7) + 5 and in_64k.lits == low.lits
    for n in (100, 5000):
        assert by_name[f"verdict_rle_{n}"].hist == [n] and by_name[f"verdict_all_but_one_{n}"].hist == [n - 1, 1]
        assert zb.literals_of(by_name[f"verdict_rle_{n}"].answer) == (1, n, 3 if n < 4096 else 4)
    small, big = by_name["verdict_gain_378"], by_name["verdict_gain_379"]
    n = small.n
    assert small.hist == big.hist and small.lits != big.lits and small.src == big.src == hc.SRC
    assert zb.literals_of(small.answer)[2] - 3 == n - hc.min_gain(n) - 1
    # the raw side's size, from the compressed side's description and the model's lengths: exactly one byte more
    def streams_bytes(r):
        seg = (r.n + 3) // 4
        return 6 + sum(sum(r.nb[b] for b in r.lits[k * seg:(k + 1) * seg if k < 3 else r.n]) // 8 + 1 for k in range(4))
    h_size = zb.literals_of(small.answer)[2] - 3 - streams_bytes(small)
    assert h_size + streams_bytes(big) == n - hc.min_gain(n) and zb.literals_of(big.answer) == (0, n, n + 2)
    for name, total, n in (("verdict_sample_68_raw", 68, 40960), ("verdict_sample_69", 69, 40960), ("verdict_sample_68_at_40959", 68, 40959)):
        r = by_name[name]
        sampled = max(collections.Counter(r.lits[:4096]).values()) + max(collections.Counter(r.lits[-4096:]).values())
        assert r.n == n and sampled == total == r.exp["sample"] and total - 68 == (0 if "68" in name else 1), name
        assert max(r.hist) > (r.n >> 7) + 4, name                                   # the whole block's own check would let it pass
    assert ((2 * 4096) >> 7) + 4 == 68
    for n in (63, 64, 255, 256, 1023, 1024, 16383, 16384):
        assert by_name[f"verdict_size_{n}" + ("_raw" if n == 63 else "")].n == n


def test_the_oracles_sections_decode_to_the_literals(oracle, rows):
    """keeps the oracle's own encoder honest: its block, framed, decodes to the case's literals"""
    decoded = 0
    for r in rows:
        if not r.answer: continue
        assert zb.literals_of(r.answer)[1] == r.n, r.name
        assert oracle.decompress(_frame_of(r.answer, r.n), r.n) == r.lits, r.name
        decoded += 1
    assert decoded == len(rows) - len(RAW_CASES)
