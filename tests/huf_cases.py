"""Crafted literal histograms for the Huffman table build (huf_tree_kernel in huf_enc.hip), in plain Python: no GPU, no oracle, no numpy.

  lengths(count, max_bits) -> (nbBits per symbol, tableLog, labels)    HUF_sort + HUF_buildTree + HUF_setMaxHeight, restated
  cases()                  -> [(name, literals, expectations)]

The model labels the cases; it never judges the GPU: that is the oracle's part (zso_huf_buildLengths for the lengths,
zso_entropy_block for the bytes).  tests/test_huf_cases_cpu.py proves the model against the oracle on every case and proves that
every case is what its expectations say; tests/test_gpu_huf_tree.py runs the table through the kernel.

labels: a dict; `label in labels` says that the branch ran, the value counts how often (or is the extreme's figure).

  HUF_setMaxHeight
    "no-clamp"            the tree is no deeper than max_bits: nothing to do
    "clamp"               it is deeper: the tail is cut to max_bits and the debt repaid
    "high-missing"        the walk down from highbit(totalCost) + 1 skips a rank that holds no symbol (`continue`)
    "low-missing"         ... stops because the rank below holds none (`lowPos == noSymbol`)
    "high-cheaper"        ... stops because lengthening the high symbol costs no more than two low ones (`highTotal <= lowTotal`)
    "step-down"           ... goes one rank down (`highTotal > lowTotal`)
    "down-to-1"           ... ends at rank 1 without a break
    "walk-up"             the rank arrived at holds no symbol: `while (n <= 12 && rankLast[n] == noSymbol) n++`
    "fill-lower"          the lengthened symbol becomes the last of a rank that held none (`rankLast[n - 1] == noSymbol`)
    "rank-at-0"           the lengthened symbol was position 0 (`rankLast[n] == 0`)
    "rank-exhausted"      the symbol in front of the lengthened one has another length: the rank is empty from now on
    "rank-continues"      ... has the same length
    "overshoot-rank1"     totalCost < 0, repaid through an existing rankLast[1]
    "overshoot-no-rank1"  totalCost < 0 with rankLast[1] missing: the first symbol of the clamped run is shortened
  figures
    "depth"               the deepest leaf before the clamp
    "tail"                symbols the clamp cut (those deeper than max_bits)
    "repay"               steps of the `totalCost > 0` loop
    "overshoot"           steps of the `totalCost < 0` loop
  HUF_sort
    "bucket"              symbols in the largest log2 bucket (counts >= 165 share a bucket per power of two)
    "bucket-164"          symbols of count 164: the last linear index, which the reference's loop also hands to the quicksort
    "qs-depth"            nested HUF_simpleQuickSort calls, the outermost being 1 (a call that only insertion-sorts counts)
    "qs-partitions"       calls of HUF_quickSortPartition
    "insertion-8" / "insertion-9-partitioned"   a whole bucket of 8 is insertion-sorted, one of 9 is partitioned first

expectations (a dict, every key optional; the histogram is the literals' own):
  "labels": (...)         labels lengths() must report
  "min": {label: n}       figures lengths() must reach
  "log": n                the final tableLog
  "src": n                the block's srcSize for the hook (default: len(literals)); 65536 where the block's own "compressed enough"
                          check would hide the literals' verdict
  "raw": True             the oracle answers "store raw" for the whole block (such a case's name ends in _raw; the CPU test lists them
                          with their reasons)
  "lits": 0 | 1 | 2       the literals section's type (raw / RLE / Huffman-coded); default 2
  "streams": 1 | 4, "lh": 3 | 4 | 5      the section header's kind
  "hdr": "fse" | n        the tree description's header byte: below 128 (FSE-compressed weights), or this value (128 and above: 4-bit weights)
  "maxsv": n              the largest byte value that occurs
  "sample": n             the sum of the most frequent bytes' counts in the first and in the last 4 KiB
  "csize": n              the section's size behind its header (cLitSize)
  "pair": name            the neighbouring case on the other side of the threshold

The verdict thresholds have a case on either side, but for one.  `hSize + 12 >= n` cannot decide a block of its own: with no earlier
table a section is tried only above 63 literals, so hSize would have to reach 52, which takes more than a hundred described weights of
some four bits of entropy each; 64 to 140 literals cannot give a tree that varied (most weights are 0 or those of a count of 1 or 2).
And where it does hold, the streams take at least 9 bytes, so `cLitSize >= n - minGain(n)` holds as well: the answer is raw either way.
"""
import random

SRC = 65536
NO = None


def highbit(v):
    return v.bit_length() - 1


def min_gain(n):
    return (n >> 6) + 2


def optimal_table_log(max_log, n, max_sv):
    """FSE_optimalTableLog_internal with minus = 1 (HUF_optimalTableLog below btultra)"""
    src_bits = highbit(n - 1) - 1
    t = min(max_log, src_bits)
    return min(max(t, min(highbit(n) + 1, highbit(max_sv) + 2), 5), 12)


# ---------------------------------------------------------------------------------------------------------------
# HUF_sort
# ---------------------------------------------------------------------------------------------------------------
def get_index(c):
    return c if c < 165 else highbit(c) + 158


def _insertion_sort(a, low, high):
    for i in range(low + 1, high + 1):
        key, j = a[i], i - 1
        while j >= low and a[j][0] < key[0]:
            a[j + 1] = a[j]; j -= 1
        a[j + 1] = key


def _partition(a, low, high):
    pivot, i = a[high][0], low - 1
    for j in range(low, high):
        if a[j][0] > pivot:
            i += 1; a[i], a[j] = a[j], a[i]
    a[i + 1], a[high] = a[high], a[i + 1]
    return i + 1


def _quick_sort(a, low, high, labels, depth):
    labels["qs-depth"] = max(labels.get("qs-depth", 0), depth)
    if high - low < 8:
        _insertion_sort(a, low, high)
        return
    while low < high:
        idx = _partition(a, low, high)
        labels["qs-partitions"] = labels.get("qs-partitions", 0) + 1
        if idx - low < high - idx:
            _quick_sort(a, low, idx - 1, labels, depth + 1); low = idx + 1
        else:
            _quick_sort(a, idx + 1, high, labels, depth + 1); high = idx - 1


def huf_sort(count, labels):
    """count[0 .. maxSymbolValue] -> [(count, symbol)] in the reference's order: descending count; equal counts below 165 by symbol,
    the log2 buckets as the quicksort leaves them"""
    base, curr = [0] * 192, [0] * 192
    for c in count: base[get_index(c)] += 1
    for n in range(191, 0, -1):
        base[n - 1] += base[n]; curr[n - 1] = base[n - 1]
    nodes = [None] * len(count)
    for s, c in enumerate(count):
        r = get_index(c) + 1
        nodes[curr[r]] = (c, s); curr[r] += 1
    for n in range(165, 191):
        size, start = curr[n] - base[n], base[n]
        if n == 165:
            if size: labels["bucket-164"] = size
        elif size:
            labels["bucket"] = max(labels.get("bucket", 0), size)
        if size == 8: labels["insertion-8"] = 1
        if size == 9: labels["insertion-9-partitioned"] = 1
        if size > 1: _quick_sort(nodes, start, start + size - 1, labels, 1)
    return nodes


# ---------------------------------------------------------------------------------------------------------------
# HUF_buildTree, HUF_setMaxHeight
# ---------------------------------------------------------------------------------------------------------------
def build_tree(nodes):
    """nodes: huf_sort's answer -> (nbBits by position, nonNullRank)"""
    cnt = {i: c for i, (c, _) in enumerate(nodes)}
    parent = {}
    rank = len(nodes) - 1
    while cnt[rank] == 0: rank -= 1
    low_s, node_nb = rank, 256
    root, low_n = node_nb + low_s - 1, node_nb
    cnt[node_nb] = cnt[low_s] + cnt[low_s - 1]
    parent[low_s] = parent[low_s - 1] = node_nb
    node_nb += 1; low_s -= 2
    for n in range(node_nb, root + 1): cnt[n] = 1 << 30
    cnt[-1] = 1 << 31
    while node_nb <= root:
        picks = []
        for _ in range(2):
            if cnt[low_s] < cnt[low_n]: picks.append(low_s); low_s -= 1
            else: picks.append(low_n); low_n += 1
        cnt[node_nb] = cnt[picks[0]] + cnt[picks[1]]
        parent[picks[0]] = parent[picks[1]] = node_nb
        node_nb += 1
    bits = {root: 0}
    for n in range(root - 1, 255, -1): bits[n] = bits[parent[n]] + 1
    return [bits[parent[n]] + 1 for n in range(rank + 1)], rank


def set_max_height(nb, cnt, max_bits, labels):
    """nb: code lengths by position (changed in place), cnt: counts by position -> the final tableLog"""
    def hit(label, by=1): labels[label] = labels.get(label, 0) + by
    last = len(nb) - 1
    largest = nb[last]
    labels["depth"] = largest
    if largest <= max_bits:
        hit("no-clamp")
        return largest
    hit("clamp")
    total, base_cost, n = 0, 1 << (largest - max_bits), last
    while nb[n] > max_bits:
        total += base_cost - (1 << (largest - nb[n]))
        nb[n] = max_bits; n -= 1
    labels["tail"] = last - n
    while nb[n] == max_bits: n -= 1
    total >>= largest - max_bits
    rank_last, current = [NO] * 14, max_bits
    for pos in range(n, -1, -1):
        if nb[pos] >= current: continue
        current = nb[pos]
        rank_last[max_bits - current] = pos
    while total > 0:
        hit("repay")
        d = highbit(total) + 1
        while d > 1:
            high_pos, low_pos = rank_last[d], rank_last[d - 1]
            if high_pos is NO:
                hit("high-missing"); d -= 1; continue
            if low_pos is NO:
                hit("low-missing"); break
            if cnt[high_pos] <= 2 * cnt[low_pos]:
                hit("high-cheaper"); break
            hit("step-down"); d -= 1
        else:
            hit("down-to-1")
        while d <= 12 and rank_last[d] is NO:
            hit("walk-up"); d += 1
        total -= 1 << (d - 1)
        nb[rank_last[d]] += 1
        if rank_last[d - 1] is NO:
            hit("fill-lower"); rank_last[d - 1] = rank_last[d]
        if rank_last[d] == 0:
            hit("rank-at-0"); rank_last[d] = NO
        else:
            rank_last[d] -= 1
            if nb[rank_last[d]] != max_bits - d:
                hit("rank-exhausted"); rank_last[d] = NO
            else:
                hit("rank-continues")
    while total < 0:
        hit("overshoot")
        if rank_last[1] is NO:
            hit("overshoot-no-rank1")
            while nb[n] == max_bits: n -= 1
            nb[n + 1] -= 1
            rank_last[1] = n + 1
            total += 1
            continue
        hit("overshoot-rank1")
        nb[rank_last[1] + 1] -= 1
        rank_last[1] += 1
        total += 1
    return max_bits


def lengths(count, max_bits):
    """count: a histogram with at least two symbols that occur -> (nbBits per symbol up to the last that occurs, tableLog, labels)"""
    count = list(count)
    while not count[-1]: count.pop()
    labels = {}
    nodes = huf_sort(count, labels)
    nb, rank = build_tree(nodes)
    table_log = set_max_height(nb, [c for c, _ in nodes], max_bits, labels)
    out = [0] * len(count)
    for pos in range(rank + 1): out[nodes[pos][1]] = nb[pos]
    return out, table_log, labels


def plan(hist):
    """what the encoder asks of the table build for this histogram -> (max_bits, maxSymbolValue)"""
    max_sv = max(s for s, c in enumerate(hist) if c)
    return optimal_table_log(11, sum(hist), max_sv), max_sv


def literals_of_histogram(hist, seed=7):
    """the histogram's bytes in a fixed-seed shuffle: the four streams differ, the counts are exact"""
    lits = [s for s, c in enumerate(hist) for _ in range(c)]
    random.Random(seed).shuffle(lits)
    return bytes(lits)


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
def _fib(k):
    a, b, out = 1, 1, []
    for _ in range(k):
        out.append(a); a, b = b, a + b
    return out


def _chain(depth, top):
    """1, 1, 2, 4, ... and one large count: a tree of exactly `depth` levels, no deeper than the table log its size allows"""
    return [1, 1] + [1 << i for i in range(1, depth - 1)] + [top]


def _geo(g, period, k):
    return [int(g ** (i % period)) for i in range(k)]


def _zipf(max_sv):
    return [max(1, 400 // (i + 1)) for i in range(max_sv + 1)]


def _decaying(n):
    """n bytes over at most 20 symbols whose counts fall by a quarter from one to the next"""
    w = [0.75 ** i for i in range(20)]
    hist = [int(n * x / sum(w)) for x in w]
    hist[0] += n - sum(hist)
    while not hist[-1]: hist.pop()
    return hist


def _sampled(n, head_max, tail_max):
    """n >= 8192 literals whose first and last 4 KiB are nearly flat (their most frequent bytes occur head_max and tail_max times)
    around a skewed body of 2 bits a byte: what HUF_compress's pre-check of a suspect block samples"""
    def flat(most, seed):
        k = (4096 - most) // 34
        hist = [most] + [34] * k + [4096 - most - 34 * k]
        assert max(hist) == most and len(hist) <= 256
        return literals_of_histogram(hist, seed)
    m = n - 8192
    body = literals_of_histogram([0] * 97 + [m - m // 4 - 2 * (m // 8), m // 4, m // 8, m // 8], 3)
    return flat(head_max, 1) + body + flat(tail_max, 2)


# histograms a seeded random search found and shrank (find_histograms below): (name, counts, labels claimed)
FOUND = [
    ("high_missing", [33, 1, 1, 1, 1, 2, 3, 18, 4], ("clamp", "high-missing", "down-to-1", "fill-lower", "rank-continues")),
    ("low_missing", [1, 14, 1, 1, 17, 5, 2, 1, 1, 1, 1, 19],
     ("clamp", "low-missing", "high-missing", "step-down", "walk-up", "rank-exhausted", "overshoot-rank1", "overshoot-no-rank1")),
    ("high_cheaper", [4, 1, 8, 6, 2, 1, 1, 8, 6, 2, 2, 1, 2, 1, 2, 1, 2, 6, 8], ("clamp", "high-cheaper", "rank-continues")),
    ("step_down", [33, 1, 1, 1, 11, 14, 2, 1], ("clamp", "step-down", "down-to-1", "walk-up", "fill-lower", "rank-exhausted", "overshoot-rank1")),
    ("down_to_1", [1, 1, 1, 3, 1, 3, 3, 1, 2, 2, 2, 2, 1, 1, 1, 6, 3, 6, 1, 1, 3, 6, 6, 1, 6], ("clamp", "down-to-1", "fill-lower", "rank-continues")),
    ("walk_up", [34, 1, 1, 1, 1, 1, 1, 1, 1, 18, 4],
     ("clamp", "walk-up", "low-missing", "high-missing", "step-down", "rank-exhausted", "overshoot-rank1", "overshoot-no-rank1")),
    ("rank_at_0", [11, 1, 9, 8, 15, 4, 1, 1, 1, 1, 1, 4, 1, 1, 3, 2], ("clamp", "rank-at-0", "high-cheaper")),
    ("rank_exhausted", [1, 1, 1, 4, 2, 34, 21], ("clamp", "rank-exhausted", "down-to-1", "fill-lower")),
    ("clamp_log7", [1, 1, 0, 0, 1, 1, 1, 1, 3, 1, 2, 3, 1, 1, 2, 2, 1, 2, 9, 17, 3, 5, 1, 1, 3, 9, 0, 1, 1, 1, 9, 1, 1], ("clamp", "down-to-1", "fill-lower")),
]
FOUND_LOGS = {"high_missing": 5, "low_missing": 5, "high_cheaper": 6, "step_down": 5, "down_to_1": 6, "walk_up": 5, "rank_at_0": 5,
              "rank_exhausted": 5, "clamp_log7": 7}

# the literals' verdict "compressed enough" (cLitSize < n - minGain(n)) on both sides of its threshold: one histogram, whose
# description takes 40 bytes, in two shuffles; the four streams' padding makes the section 378 bytes in one and 379 in the other
_GAIN_HIST = [(1, 1, 2, 2, 3, 4, 6)[(i * 5 + i // 7) % 7] for i in range(135)] + [20]
_GAIN_SEEDS = (1, 3)


def cases():
    out = []

    def add(name, hist, exp=None, seed=7, lits=None):
        exp = dict(exp or {})
        out.append((name, literals_of_histogram(hist, seed) if lits is None else lits, exp))
    # ---- length limiting
    for name, hist, labels in FOUND:
        add(f"len_{name}", hist, {"labels": labels, "log": FOUND_LOGS[name]})
    for k, log in ((9, 5), (10, 6), (12, 7), (13, 8), (15, 9), (16, 10), (18, 11)):       # Fibonacci counts: the deepest tree a size allows
        add(f"len_fib_{k}", _fib(k), {"labels": ("clamp", "high-cheaper", "rank-exhausted"), "log": log, "min": {"depth": k - 1}})
    add("len_fib_8_padded", _fib(8) + [3] * 5, {"labels": ("clamp", "down-to-1", "fill-lower"), "log": 5})
    add("len_fib_21", _fib(21), {"labels": ("clamp",), "log": 11, "min": {"depth": 20, "tail": 10}})
    add("len_fib_22", _fib(22), {"labels": ("clamp",), "log": 11, "min": {"depth": 21, "tail": 11}})
    for depth, top in ((5, 60), (6, 150), (7, 300), (8, 500), (9, 1000), (10, 2000), (11, 4000)):   # as deep as allowed, no deeper
        add(f"len_chain_{depth}", _chain(depth, top), {"labels": ("no-clamp",), "log": depth})
    for m, log in ((32, 6), (64, 7), (128, 8), (200, 9)):                                            # shallower than allowed
        add(f"len_flat_{m}", [8 + (i % 3 == 0) for i in range(m)] + [4 * m], {"labels": ("no-clamp",), "log": log})
    add("len_overshoot_31", [1] * 65 + [33],
        {"labels": ("clamp", "walk-up", "rank-at-0", "overshoot-rank1", "overshoot-no-rank1"), "log": 7, "min": {"overshoot": 31, "walk-up": 5}})
    add("len_repay_37", _geo(2.05, 3, 124) + [200], {"labels": ("clamp", "high-missing", "down-to-1", "rank-continues"), "log": 8, "min": {"repay": 37, "tail": 53}})
    add("len_tail_204", [1] * 230 + [40] * 12,
        {"labels": ("clamp", "low-missing", "walk-up", "overshoot-rank1", "overshoot-no-rank1"), "log": 9, "min": {"tail": 204}})
    add("len_geo_2.05_5", _geo(2.05, 5, 200), {"labels": ("clamp", "low-missing", "step-down", "high-cheaper", "rank-exhausted"), "log": 9, "min": {"repay": 23}})
    add("len_geo_2.05_8", _geo(2.05, 8, 100), {"labels": ("clamp", "low-missing", "step-down", "down-to-1"), "log": 10, "min": {"repay": 15}})
    add("len_geo_1.5_12", _geo(1.5, 12, 200), {"labels": ("clamp", "rank-at-0", "high-missing"), "log": 10})
    add("len_geo_3.05_4", _geo(3.05, 4, 200), {"labels": ("clamp", "low-missing", "high-missing"), "log": 10})
    for p, log in ((6, 7), (8, 9), (10, 10), (12, 11)):                                              # power-of-two counts
        add(f"len_pow2_{p}", [1 << (i % p) for i in range(40)], {"labels": ("clamp", "high-cheaper"), "log": log})
    # ---- sorting
    spread = [165 + (i * 37) % 91 for i in range(250)]
    add("sort_bucket_250", spread + [9000], {"min": {"bucket": 250, "qs-depth": 5}, "log": 9})
    add("sort_bucket_210", spread[:210] + [9000], {"min": {"bucket": 210, "qs-depth": 4}})
    add("sort_bucket_210_ascending", [165 + i * 90 // 209 for i in range(210)] + [9000], {"min": {"bucket": 210, "qs-partitions": 100}})
    add("sort_bucket_210_descending", [255 - i * 90 // 209 for i in range(210)] + [9000], {"min": {"bucket": 210}})
    add("sort_bucket_210_equal", [200] * 210 + [9000], {"min": {"bucket": 210, "qs-partitions": 209}})
    eight = [170, 250, 165, 200, 255, 180, 201, 199]
    add("sort_bucket_8", eight + [3, 2, 1, 1], {"labels": ("insertion-8",), "min": {"bucket": 8}})
    add("sort_bucket_9", eight + [166, 3, 2, 1, 1], {"labels": ("insertion-9-partitioned",), "min": {"bucket": 9, "qs-depth": 2}})
    # buckets of few distinct counts: only the order of equal counts tells an insertion sort from a partition, or one side of a
    # partition from the other, and that order decides which symbols the tree makes longer
    for k, mod, mul in ((8, 3, 37), (9, 2, 1), (9, 7, 11), (10, 3, 37), (11, 7, 11), (17, 2, 1), (19, 2, 1), (25, 3, 37), (64, 7, 11), (128, 5, 37), (250, 7, 11)):
        add(f"sort_ties_{k}_of_{mod}", [165 + 11 * ((i * mul) % mod) for i in range(k)] + [9000 if k > 60 else 600, 3, 1], {"min": {"bucket": k}})
    add("sort_seam_164_165", [164, 165] * 20 + [3, 1], {"min": {"bucket-164": 20, "bucket": 20}})
    add("sort_two_symbols", [40, 24], {"log": 1, "hdr": 128})
    add("sort_two_symbols_1024", [1000, 24], {"log": 1, "lh": 4})
    add("sort_two_symbols_0_255", [50] + [0] * 254 + [30], {"log": 1, "hdr": "fse"})
    for max_sv in (1, 63, 64, 127, 128, 129, 254, 255):
        add(f"sort_maxsv_{max_sv}", _zipf(max_sv), {"maxsv": max_sv})
        if max_sv > 1:
            add(f"sort_maxsv_{max_sv}_holes", [40] + [0] * (max_sv - 2) + [9, 15], {"maxsv": max_sv, "log": 2})
    # ---- tree description
    add("desc_raw4_odd", [30, 20, 10, 4], {"hdr": 130})
    add("desc_raw4_even", [30, 20, 10, 4, 2], {"hdr": 131})
    add("desc_equal_32", [10] * 32 + [320], {"hdr": 159})
    add("desc_equal_64", [100] * 64 + [6400], {"hdr": 191})
    add("desc_equal_128", [100] * 128 + [12800], {"hdr": 255, "pair": "desc_equal_192_raw"})
    add("desc_equal_192_raw", [100] * 192 + [6400], {"raw": True, "pair": "desc_equal_128"})
    add("desc_equal_224_raw", [100] * 224 + [3200], {"raw": True, "pair": "desc_equal_128"})
    add("desc_weights_once", [128, 64, 32, 16, 8, 4, 4], {"hdr": 133, "labels": ("no-clamp",), "log": 6})
    add("desc_fse_255_weights", _geo(1.5, 12, 256), {"hdr": "fse", "maxsv": 255})
    add("desc_fse_254_weights", _geo(1.5, 12, 255), {"hdr": "fse", "maxsv": 254})
    # ---- verdicts
    add("verdict_largest_12_raw", [12] * 85 + [4], {"raw": True, "pair": "verdict_largest_13"})
    add("verdict_largest_13", [13] + [12] * 84 + [3], {"pair": "verdict_largest_12_raw", "lh": 4})
    add("verdict_largest_12_in_64k", [12] * 85 + [4], {"src": SRC, "lits": 0, "pair": "verdict_largest_13"})
    for n in (100, 5000):
        add(f"verdict_rle_{n}", [n], {"lits": 1, "pair": f"verdict_all_but_one_{n}"})
        add(f"verdict_all_but_one_{n}", [n - 1, 1], {"log": 1, "pair": f"verdict_rle_{n}"})
    n = sum(_GAIN_HIST)
    add("verdict_gain_378", _GAIN_HIST, {"src": SRC, "csize": n - min_gain(n) - 1, "pair": "verdict_gain_379"}, seed=_GAIN_SEEDS[0])
    add("verdict_gain_379", _GAIN_HIST, {"src": SRC, "lits": 0, "pair": "verdict_gain_378"}, seed=_GAIN_SEEDS[1])
    add("verdict_sample_68_raw", None, {"raw": True, "sample": 68, "pair": "verdict_sample_69"},
        lits=_sampled(40960, 34, 34))
    add("verdict_sample_69", None, {"sample": 69, "lh": 5, "pair": "verdict_sample_68_raw"}, lits=_sampled(40960, 35, 34))
    add("verdict_sample_68_at_40959", None, {"sample": 68, "lh": 5}, lits=_sampled(40959, 34, 34))
    add("verdict_size_63_raw", _decaying(63), {"raw": True, "pair": "verdict_size_64"})
    add("verdict_size_64", _decaying(64), {"streams": 1, "lh": 3, "pair": "verdict_size_63_raw"})
    for n, streams, lh in ((255, 1, 3), (256, 4, 3), (1023, 4, 3), (1024, 4, 4), (16383, 4, 4), (16384, 4, 5)):
        add(f"verdict_size_{n}", _decaying(n), {"streams": streams, "lh": lh})
    return out


REQUIRED_LABELS = ("no-clamp", "clamp", "step-down", "high-cheaper", "low-missing", "high-missing", "walk-up", "fill-lower", "rank-exhausted",
                   "rank-at-0", "overshoot-rank1", "overshoot-no-rank1", "down-to-1", "rank-continues")
REQUIRED_FIGURES = {"overshoot": 8, "repay": 30, "depth": 20, "tail": 200, "bucket": 128, "qs-depth": 4}


def find_histograms(tries, seed=3, largest=6000):
    """the search behind FOUND: random histograms of several shapes -> {label: smallest histogram found that reaches it}; the lists
    above are these, shrunk by dropping symbols and lowering counts for as long as the label stayed"""
    rng, found = random.Random(seed), {}
    for _ in range(tries):
        nsym, shape = rng.randrange(2, 257), rng.randrange(4)
        if shape == 0: hist = _geo(rng.uniform(1.2, 2.5), rng.randrange(3, 24), nsym)
        elif shape == 1: hist = [1 << rng.randrange(0, 12) for _ in range(nsym)]
        elif shape == 2: hist = _fib(min(nsym, 22)) + [rng.randrange(1, 4) for _ in range(rng.randrange(0, 6))]
        else: hist = [int(rng.paretovariate(0.8)) for _ in range(nsym)]
        if rng.random() < 0.5:
            p = rng.uniform(0, 0.6)
            hist = [0 if rng.random() < p else c for c in hist]
        rng.shuffle(hist)
        while hist and not hist[-1]: hist.pop()
        if sum(1 for c in hist if c) < 2 or not 64 <= sum(hist) <= largest: continue
        for label in lengths(hist, plan(hist)[0])[2]:
            if label not in found or sum(hist) < sum(found[label]): found[label] = hist
    return found
