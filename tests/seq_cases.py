"""Crafted seqStores for the sequence encoder (seq_enc.hip), in plain Python: no GPU, no oracle, no numpy.

Two tables:

  entropy_cases()  -> [(name, seqs, lits, srcSize, expectation)]   seqs hold repcodes already (offBase as the block codes it)
  repcode_cases()  -> [(name, raw, lits, srcSize, rep)]            raw offsets (offBase = distance + 3) and the history in front

A sequence is (offBase, litLength, mlBase).  The stores need not be replayable: the entropy stage codes what it is given.  Where a
case is about sequences it carries at most 63 literal bytes (stored raw whatever the verdict on them) and srcSize = 65536, so that
"compressed enough" never interferes.

expectation (a dict, every key optional):
  "modes": {strategy: (LL, OF, ML)}   the mode byte the oracle must write (0 predefined, 1 RLE, 2 described), per oracle strategy
  "raw": True                         the oracle answers "store raw" (such a case has "raw" in its name)
  "lits": 0 | 2                       the literals section's type (raw / Huffman-coded)
  "size": n                           the oracle's block size
  "branch": (alphabet, label)         a label label_table() must report for that alphabet's description (0 LL, 1 OF, 2 ML)

LEVELS pairs the compression levels the GPU contexts are made with and the strategy the oracle is asked for: level 9 is lazy2, whose
constants are greedy's (the clamp in the entropy hook and in the pipeline).

The rules restated here (the repcode rule, ZSTD_selectEncodingType below lazy, FSE_normalizeCount, the state chains' bit counts) label
and build the cases; they never judge the GPU: that is the oracle's part.

FSE_normalizeM2's branches: a search of 200 000 random histograms (find_m2_histograms below) reached the main loop and the second
pass.  "total is zero" is reached by construction: 22 sequences with 22 different offset codes, one of them above 28, so that the table
is described at tableLog 5 and every count of 1 first rounds up to 2.  None was found for the branches in M2_NOT_FOUND, and counting
says none exists: "every symbol distributed" and "nothing left to distribute" need more symbols that occur than two thirds of the
table's cells, which the smallest tables (32 cells for offsets, 64 for the lengths) only allow below the sequence counts at which a
table is described at all, or at counts where nothing rounds up and FSE_normalizeM2 is not called.
"""
import random

SRC = 65536
LEVELS = ((1, 1), (3, 2), (5, 3), (9, 3))          # (level of the GPU context, strategy of the oracle)
STRATEGIES = (1, 2, 3)

LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
# per alphabet (LL, OF, ML): largest code, FSELog, predefined table's log, largest code the predefined table may serve, its counts
ALPHABETS = ((35, 9, 6, 35, LL_DEFAULT), (31, 8, 5, 28, OF_DEFAULT), (52, 9, 6, 52, ML_DEFAULT))
# the smallest value of each code
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48] + [1 << k for k in range(6, 17)]
ML_BASE = list(range(32)) + [32, 34, 36, 38, 40, 44, 48, 56, 64, 80, 96] + [1 << k for k in range(7, 17)]
MAX_LL_CODE, MAX_ML_CODE = 34, 51          # what 16-bit fields reach (65535)


def highbit(v):
    return v.bit_length() - 1


def ll_code(ll):
    if ll > 63:
        return highbit(ll) + 19
    return ll if ll < 16 else (16 + (ll - 16) // 2 if ll < 24 else (20 + (ll - 24) // 4 if ll < 32 else (22 if ll < 40 else (23 if ll < 48 else 24))))


def ml_code(ml):
    if ml > 127:
        return highbit(ml) + 36
    if ml < 32:
        return ml
    if ml < 40:
        return 32 + (ml - 32) // 2
    if ml < 48:
        return 36 + (ml - 40) // 4
    return 38 if ml < 56 else (39 if ml < 64 else (40 if ml < 80 else (41 if ml < 96 else 42)))


def codes_of(seq):
    return ll_code(seq[1]), highbit(seq[0]), ml_code(seq[2])


def extra_bits(seq):
    llc, ofc, mlc = codes_of(seq)
    return LL_BITS[llc] + ML_BITS[mlc] + ofc


def seq_of_codes(llc, ofc, mlc, fill=0):
    """a sequence with these three codes; fill picks the extra bits (0: the smallest values, 1: the largest)"""
    ll = LL_BASE[llc] + (min((1 << LL_BITS[llc]) - 1, 65535 - LL_BASE[llc]) if fill else 0)
    ml = ML_BASE[mlc] + (min((1 << ML_BITS[mlc]) - 1, 65535 - ML_BASE[mlc]) if fill else 0)
    off = (1 << ofc) + (((1 << ofc) - 1) if fill else 0)
    return (off, ll, ml)


# ---------------------------------------------------------------------------------------------------------------
# the repcode rule
# ---------------------------------------------------------------------------------------------------------------
KINDS = ("rep0", "rep1", "rep2", "ll0_rep1", "ll0_rep2", "ll0_rep0m1", "ll0_full0")


def _code_for(off, ll0, hist):
    """(code, kind) of distance `off` against the history; a history entry of 0 is unknown and equals no distance"""
    if not ll0:
        if off == hist[0]: return 1, "rep0"
        if off == hist[1]: return 2, "rep1"
        if off == hist[2]: return 3, "rep2"
        return off + 3, None
    if off == hist[1]: return 1, "ll0_rep1"
    if off == hist[2]: return 2, "ll0_rep2"
    if hist[0] > 1 and off == hist[0] - 1: return 3, "ll0_rep0m1"
    return off + 3, ("ll0_full0" if off == hist[0] else None)


def history_after(code, ll0, hist):
    """the decoder's update (the rule of _replay in test_gpu_parity.py) -> (distance used, history behind the sequence)"""
    if code > 3:
        return code - 3, [code - 3, hist[0], hist[1]]
    idx = code - 1 + (1 if ll0 else 0)
    if idx == 0:
        return hist[0], list(hist)
    off = hist[0] - 1 if idx == 3 else hist[idx]
    return off, ([off, hist[0], hist[2]] if idx == 1 else [off, hist[0], hist[1]])


def resolve_reps(raw, rep):
    """raw: sequences with offBase = distance + 3 throughout -> the same with repcodes, by the serial rule"""
    return [s for s, _ in _resolve(raw, rep)]


def classify(raw, rep):
    """-> per sequence the kind of hit (one of KINDS) or None for a plain full offset"""
    return [k for _, k in _resolve(raw, rep)]


def _resolve(raw, rep):
    hist, out = list(rep), []
    for off_base, ll, mlb in raw:
        code, kind = _code_for(off_base - 3, ll == 0, hist)
        _, hist = history_after(code, ll == 0, hist)
        out.append(((code, ll, mlb), kind))
    return out


class _Store:
    """builds a raw-offset store against a running history: full() files a distance that hits nothing, hit(kind) one that hits"""

    def __init__(self, rep):
        self.rep, self.hist, self.raw, self.fresh = tuple(rep), list(rep), [], 1000

    def _file(self, off, ll):
        code, kind = _code_for(off, ll == 0, self.hist)
        _, self.hist = history_after(code, ll == 0, self.hist)
        self.raw.append((off + 3, ll, len(self.raw) % 11))
        return kind

    def full(self, off=None, ll=None):
        if off is None:
            self.fresh += 7; off = self.fresh          # 7 apart: never a history entry, never rep0 - 1
        assert self._file(off, 1 + len(self.raw) % 3 if ll is None else ll) is None
        return self

    def fulls(self, n):
        for _ in range(n): self.full()
        return self

    def hit(self, kind):
        h = self.hist
        off = {"rep0": h[0], "rep1": h[1], "rep2": h[2], "ll0_rep1": h[1], "ll0_rep2": h[2], "ll0_rep0m1": h[0] - 1, "ll0_full0": h[0]}[kind]
        assert off >= 1 and self._file(off, 0 if kind.startswith("ll0") else 2) == kind, (kind, h)
        return self

    def hits(self, kind, n):
        for _ in range(n): self.hit(kind)
        return self


def _tail(st):
    """behind the sequence under test: one use of each history entry, so that a wrong update shows in the codes, not only in a later block"""
    for kind in ("rep1", "rep2"):
        if _code_for(st.hist[int(kind[3])], False, st.hist)[1] == kind: st.hit(kind)      # (equal entries: the earlier one answers)
    return st.full().hit("rep0")


_REP_LITS = bytes(range(40))


def repcode_cases():
    cases = []

    def add(name, st):
        cases.append((name, list(st.raw), _REP_LITS, SRC, st.rep))
    # each kind of hit at the first and the last lane of a batch, around the batch edges
    for kind in KINDS:
        for at in (0, 1, 62, 63, 64, 65, 127, 128):
            add(f"{kind}@{at}", _tail(_Store((12, 40, 77)).fulls(at).hit(kind)))
    # carried history: the sequences that define rep1 / rep2 lie one and two batches back, only R1 / R2 hold them
    for n in (64, 130, 61, 125):         # 61 / 125: the swap is lane 0 of a batch (index 64 / 128)
        add(f"carried_{n}", _Store((1, 4, 8)).fulls(3).hits("rep0", n).hit("rep1").hit("rep2").hit("rep2").full().hit("rep1"))
        add(f"carried_ll0_{n}", _Store((1, 4, 8)).fulls(3).hits("rep0", n).hit("ll0_rep1").hit("ll0_rep2").hit("ll0_rep0m1").hit("rep1"))
    # rep0 - 1: rep0 = 1 gives distance 0, which no store holds, so nothing may fire on the distances around it; rep0 = 2 gives 1
    add("rep0m1_rep0_is_1", _Store((1, 4, 8)).full(20, 0).hit("rep1").full(30, 0).hit("rep1").full(2, 0).hit("rep1").full(5, 0))
    add("rep0m1_rep0_is_2", _tail(_Store((2, 40, 77)).hit("ll0_rep0m1").fulls(2).full(2).hit("ll0_rep0m1")))
    # histories with equal entries
    add("equal_after_ll0_full0", _Store((1, 4, 8)).fulls(2).hit("ll0_full0").hit("rep0").hit("ll0_rep1").hit("rep2").hit("ll0_rep1").hit("ll0_rep2").hit("rep2"))
    add("equal_555", _Store((5, 5, 5)).hit("rep0").hit("ll0_rep1").hit("ll0_rep0m1").hit("rep1").hit("ll0_rep2").full().hit("rep1"))
    # unknown history: 1, 4 and 8 are ordinary distances until the block has defined them
    st = _Store((0, 0, 0)).full(1).full(4, 0).full(8)
    add("unknown_000", st.hit("rep2").hit("ll0_rep2").hit("rep1").full(3, 0).hit("ll0_rep0m1"))
    add("unknown_000_ll0_first", _Store((0, 0, 0)).full(1, 0).hit("ll0_full0").hit("rep0").full(4).hit("rep1"))
    add("plain_148", _tail(_Store((1, 4, 8)).hit("rep1").hit("ll0_rep2").hit("rep2").full(3, 0)))
    add("dictionary_like", _tail(_Store((700, 40, 9)).hit("rep2").hit("ll0_rep0m1").hit("ll0_rep1").hit("rep0")))
    # seeded random stores: few distinct distances, so hits are the rule
    rng = random.Random(20250131)
    for i in range(200):
        rep = ((0, 0, 0), (1, 4, 8), (700, 40, 9))[rng.randrange(3)]
        pool = sorted(rng.sample(range(1, 10), rng.randrange(3, 6)))
        if rng.random() < 0.3: pool[rng.randrange(len(pool))] = rep[rng.randrange(3)] or 2
        raw = [(rng.choice(pool) + 3, 0 if rng.random() < 0.3 else rng.randrange(1, 20), rng.randrange(0, 40)) for _ in range(rng.randrange(1, 401))]
        cases.append((f"random_{i}", raw, _REP_LITS, SRC, rep))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# ZSTD_selectEncodingType below lazy, FSE_optimalTableLog, FSE_normalizeCount: restated to label cases
# ---------------------------------------------------------------------------------------------------------------
def select_mode(count, nb_seq, alphabet, strategy):
    max_code, _, default_log, default_max, _ = ALPHABETS[alphabet]
    top = max(s for s in range(max_code + 1) if count[s])
    most = max(count)
    allowed = top <= default_max
    if most == nb_seq:
        return 0 if allowed and nb_seq <= 2 else 1
    if allowed and (nb_seq < ((1 << default_log) * (10 - strategy)) >> 3 or most < nb_seq >> (default_log - 1)):
        return 0
    return 2


def optimal_table_log(max_log, n, max_sv):
    src_bits = highbit(n - 1) - 2
    t = max_log if src_bits < 0 else min(max_log, src_bits)           # (unsigned in the reference: 1 - 2 is large)
    return min(max(t, min(highbit(n) + 1, highbit(max_sv) + 2), 5), 12)


_RTB = (0, 473195, 504333, 520860, 550000, 700000, 750000, 830000)


def normalize(count, total, table_log, low_prob):
    """FSE_normalizeCount -> (normalised counts, the set of branches taken)"""
    labels, lp = set(), (-1 if low_prob else 1)
    scale = 62 - table_log
    step, vstep = (1 << 62) // total, 1 << (scale - 20)
    still, largest, largest_p, low_thr = 1 << table_log, 0, 0, total >> table_log
    norm = [0] * len(count)
    for s, c in enumerate(count):
        if c == 0: continue
        if c <= low_thr:
            norm[s] = lp; still -= 1; labels.add("low-1" if low_prob else "low+1")
            continue
        p = (c * step) >> scale
        if p < 8 and c * step - (p << scale) > vstep * _RTB[p]:
            p += 1; labels.add("rtb-up")
        if p > largest_p: largest_p, largest = p, s
        norm[s] = p; still -= p
    if -still < (norm[largest] >> 1):
        labels.add("primary-negative" if still < 0 else "primary")
        norm[largest] += still
        return norm, labels
    labels.add("M2")
    distributed, low_one = 0, (total * 3) >> (table_log + 1)
    for s, c in enumerate(count):
        if c == 0: norm[s] = 0
        elif c <= low_thr: norm[s] = lp; distributed += 1; total -= c
        elif c <= low_one: norm[s] = 1; distributed += 1; total -= c
        else: norm[s] = None
    to_dist = (1 << table_log) - distributed
    if to_dist == 0:
        labels.add("M2-nothing-left"); return norm, labels
    if total // to_dist > low_one:
        labels.add("M2-second-pass")
        low_one = (total * 3) // (to_dist * 2)
        for s, c in enumerate(count):
            if norm[s] is None and c <= low_one: norm[s] = 1; distributed += 1; total -= c
        to_dist = (1 << table_log) - distributed
    if distributed == len(count):
        labels.add("M2-all-distributed")
        norm[count.index(max(count))] += to_dist
        return norm, labels
    if total == 0:
        labels.add("M2-total-zero")
        s = 0
        while to_dist:
            if norm[s] > 0: norm[s] += 1; to_dist -= 1
            s = (s + 1) % len(count)
        return norm, labels
    labels.add("M2-main")
    vlog = 62 - table_log
    mid = (1 << (vlog - 1)) - 1
    rstep, tmp = ((to_dist << vlog) + mid) // total, mid
    for s, c in enumerate(count):
        if norm[s] is None:
            end = tmp + c * rstep
            norm[s] = (end >> vlog) - (tmp >> vlog); tmp = end
            assert norm[s] >= 1, "FSE_normalizeM2 fails on this histogram: not a case"
    return norm, labels


def plan_table(seqs, alphabet, strategy):
    """what the encoder decides for one alphabet -> (mode, tableLog, normalised counts or None for RLE, labels)"""
    max_code, fse_log, default_log, _, default_norm = ALPHABETS[alphabet]
    codes = [codes_of(s)[alphabet] for s in seqs]
    count = [0] * (max_code + 1)
    for c in codes: count[c] += 1
    mode = select_mode(count, len(seqs), alphabet, strategy)
    if mode == 1: return 1, 0, None, {"rle"}
    if mode == 0: return 0, default_log, list(default_norm), {"predefined"}
    top = max(c for c in range(max_code + 1) if count[c])
    total = len(seqs)
    table_log = optimal_table_log(fse_log, total, top)
    if count[codes[-1]] > 1: count[codes[-1]] -= 1; total -= 1      # the last sequence's code is paid by the state's start
    norm, labels = normalize(count[:top + 1], total, table_log, total >= 2048)
    return 2, table_log, norm, labels


def label_table(seqs, alphabet, strategy=1):
    return plan_table(seqs, alphabet, strategy)[3]


def modes_by_rule(seqs):
    return {st: tuple(plan_table(seqs, a, st)[0] for a in range(3)) for st in STRATEGIES}


# ---------------------------------------------------------------------------------------------------------------
# FSE_buildCTable + FSE_encodeSymbol: only how many bits each step of a state chain emits
# ---------------------------------------------------------------------------------------------------------------
def state_bits(codes, norm, table_log):
    """codes in the order they are coded (last sequence first) -> bits per step; the first step only sets the state"""
    if norm is None:
        return [0] * len(codes)
    size = 1 << table_log
    step, mask, high = (size >> 1) + (size >> 3) + 3, size - 1, size - 1
    cell = [0] * size
    for s, n in enumerate(norm):
        if n == -1: cell[high] = s; high -= 1
    pos = 0
    for s, n in enumerate(norm):
        for _ in range(max(n, 0)):
            cell[pos] = s
            pos = (pos + step) & mask
            while pos > high: pos = (pos + step) & mask
    assert pos == 0
    start, acc = [], 0
    for n in norm:
        start.append(acc); acc += abs(n)
    nxt, table = list(start), [0] * size
    for u in range(size):
        table[nxt[cell[u]]] = size + u; nxt[cell[u]] += 1
    dnb, dfs = {}, {}
    for s, n in enumerate(norm):
        if n == 0: continue
        if abs(n) == 1: dnb[s], dfs[s] = (table_log << 16) - size, start[s] - 1
        else:
            out = table_log - highbit(n - 1)
            dnb[s], dfs[s] = (out << 16) - (n << out), start[s] - n
    s = codes[0]
    nb = (dnb[s] + (1 << 15)) >> 16
    state, bits = table[(((nb << 16) - dnb[s]) >> nb) + dfs[s]], [0]
    for s in codes[1:]:
        nb = (state + dnb[s]) >> 16
        bits.append(nb)
        state = table[(state >> nb) + dfs[s]]
    return bits


def field_bits(seqs, strategy):
    """bits each sequence adds to the stream, in coding order (last sequence first): three state steps + the three extra fields"""
    order = seqs[::-1]
    total = [extra_bits(s) for s in order]
    logs = []
    for a in range(3):
        _, log, norm, _ = plan_table(seqs, a, strategy)
        logs.append(log)
        for i, b in enumerate(state_bits([codes_of(s)[a] for s in order], norm, log)): total[i] += b
    return total, logs


def bitstream_bytes(seqs, strategy):
    total, logs = field_bits(seqs, strategy)
    return (sum(total) + sum(logs) + 1 + 7) // 8


def carry_alignments(seqs, strategy):
    """the encoder packs 64 sequences per step and hands the bits of the last, partly filled word to the next step (and the last
    step's to the closing flush): -> those bit counts, 0..31 each"""
    total, _ = field_bits(seqs, strategy)
    out, acc = [], 0
    for i in range(0, len(total), 64):
        acc += sum(total[i:i + 64]); out.append(acc & 31)
    return out


def lane_alignments(seqs, strategy):
    """-> the bit position modulo 32 at which each sequence's fields start (every lane shifts its 128-bit field by it)"""
    total, _ = field_bits(seqs, strategy)
    out, acc = set(), 0
    for b in total:
        out.add(acc & 31); acc += b
    return out


# ---------------------------------------------------------------------------------------------------------------
# the entropy cases
# ---------------------------------------------------------------------------------------------------------------
def _flat(n):
    return [(4 + i % 7, i % 5, i % 9) for i in range(n)]


def _mixed(n, seed):
    """moderate widths over many codes: what the batch edges are fed"""
    rng = random.Random(seed)
    return [(rng.randrange(1, 1 << rng.randrange(1, 11)), rng.randrange(0, 1 << rng.randrange(0, 7)), rng.randrange(0, 1 << rng.randrange(0, 8)))
            for _ in range(n)]


def _skewed(n, alphabet):
    """one code of `alphabet` carries 97 % of the sequences; with fewer than 34 that leaves room for no second code, which would
    be RLE, so one sequence always differs"""
    seqs, others = [], max(1, (n * 3) // 100)
    for i, s in enumerate(_flat(n)):
        s = list(s)
        if i % (n // others) != 0 or i // (n // others) >= others:
            s[alphabet_field(alphabet)] = (5, 3, 2)[alphabet]
        else:
            s[alphabet_field(alphabet)] = (9, 1, 7)[alphabet]
        seqs.append(tuple(s))
    return seqs


def alphabet_field(alphabet):
    return (1, 0, 2)[alphabet]          # LL is litLength, OF is offBase, ML is mlBase


def _spread(n, alphabet, ncodes):
    """sequence i takes code i % ncodes of `alphabet`; the other two alphabets hold one code (RLE)"""
    out = []
    for i in range(n):
        c = [0, 2, 0]; c[alphabet] = i % ncodes
        out.append(seq_of_codes(*c))
    return out


def _from_histogram(alphabet, count, last_code):
    """a store whose `alphabet` codes have this histogram, the last sequence's code being last_code; the other alphabets are RLE"""
    codes = [c for c, k in enumerate(count) for _ in range(k)]
    random.Random(7).shuffle(codes)
    i = len(codes) - 1 - codes[::-1].index(last_code)
    codes[i], codes[-1] = codes[-1], codes[i]
    out = []
    for c in codes:
        t = [0, 2, 0]; t[alphabet] = c
        out.append(seq_of_codes(*t))
    return out


# histograms FSE_normalizeCount sends to FSE_normalizeM2, found by find_m2_histograms (alphabet, counts, code of the last sequence,
# the branch); the counts are what the store holds, the encoder takes one off the last code
M2_FOUND = [(2, [1, 4, 2, 3, 1, 4, 1, 1, 136, 19, 1, 16, 1, 54, 6, 2], 8, "M2-main"),
            (1, [1, 2, 1, 1, 8, 1, 1, 1, 1, 1, 1, 13, 1, 2, 3, 3, 1, 3, 1, 6, 1, 8, 1, 3, 1, 3, 3, 12, 317, 108, 2], 12, "M2-second-pass"),
            (1, [1] * 21 + [0] * 8 + [1], 29, "M2-total-zero")]
M2_NOT_FOUND = ("M2-all-distributed", "M2-nothing-left")


def find_m2_histograms(tries, seed=1):
    """the search behind M2_FOUND: random histograms of each alphabet -> {branch: (alphabet, counts, last code)} (first found)"""
    rng, found = random.Random(seed), {}
    for _ in range(tries):
        a = rng.randrange(3)
        ncodes = rng.randrange(2, ALPHABETS[a][0] + 2)
        shape = rng.randrange(4)
        if shape == 0: count = [rng.randrange(0, 9) for _ in range(ncodes)]
        elif shape == 1: count = [rng.randrange(1, 4) for _ in range(ncodes)]
        elif shape == 2: count = [rng.choice((0, 1, 1, 2, 60, 300)) for _ in range(ncodes)]
        else: count = [int(rng.paretovariate(0.7)) for _ in range(ncodes)]
        if sum(1 for c in count if c) < 2 or sum(count) > 16384 or not count[-1]: continue
        last = rng.choice([c for c, k in enumerate(count) if k])
        seqs = _from_histogram(a, count, last)
        if plan_table(seqs, a, 1)[0] != 2: continue
        try:
            labels = label_table(seqs, a)
        except AssertionError:
            continue
        for l in labels:
            if l.startswith("M2-"): found.setdefault(l, (a, count, last))
    return found


def _ramp_ended_literals(n):
    """skewed literals (2 bits a byte) whose first and last 4 KiB are a byte ramp: the sampling of a suspect block sees the ramps"""
    rng = random.Random(45)
    body = bytes(rng.choices((97, 98, 99, 100), (8, 4, 2, 2), k=n - 8192))
    ramp = bytes(i & 255 for i in range(4096))
    return ramp + body + ramp


def entropy_cases():
    cases = []

    def add(name, seqs, exp=None, lits=_REP_LITS, src=SRC):
        cases.append((name, seqs, lits, src, exp or {}))
    # nbSeq edges: the header's 1- / 2-byte edge, the batch edges, every residue of the chain lanes' unrolled loop
    for n in (1, 2, 3, 4, 63, 64, 65, 66, 67, 68, 127, 128, 129, 191, 192, 193, 255, 256, 257, 16383, 16384):
        add(f"nbseq_{n}", _mixed(n, n))
    # strategy thresholds: predefined below (1 << log) * (10 - strategy) / 8 sequences: 72 / 64 / 56 (LL, ML), 36 / 32 / 28 (OF)
    for n in (27, 28, 31, 32, 35, 36, 55, 56, 63, 64, 71, 72):
        modes = {st: (0 if n < (9 - st) * 8 + 8 else 2, 0 if n < (9 - st) * 4 + 4 else 2, 0 if n < (9 - st) * 8 + 8 else 2) for st in STRATEGIES}
        add(f"threshold_flat_{n}", _flat(n), {"modes": modes})
        for a in range(3):
            add(f"threshold_skew{'LL OF ML'.split()[a]}_{n}", _skewed(n, a), {"modes": modes})
    # the rule's other side: predefined because no code is frequent (mostFrequent < nbSeq >> (log - 1)), however many sequences
    for a, ncodes, n, mode in ((0, 35, 383, 2), (0, 35, 384, 0), (1, 29, 47, 2), (1, 29, 48, 0), (2, 52, 127, 2), (2, 52, 128, 0)):
        m = [1, 1, 1]; m[a] = mode
        add(f"threshold_spread{'LL OF ML'.split()[a]}_{n}", _spread(n, a, ncodes), {"modes": {st: tuple(m) for st in STRATEGIES}})
    # modes: all codes equal (predefined up to 2 sequences, RLE above), per alphabet and in all three
    for n in (1, 2, 3, 200):
        for a in range(3):
            seqs = []
            for s in _flat(n):
                s = list(s); s[alphabet_field(a)] = (5, 6, 4)[a]; seqs.append(tuple(s))
            add(f"equal{'LL OF ML'.split()[a]}_{n}", seqs)
        add(f"equal_all_{n}", [(6, 5, 4)] * n, {"modes": {st: ((0, 0, 0) if n <= 2 else (1, 1, 1)) for st in STRATEGIES}})
    # offset codes the predefined table does not hold: RLE when equal (also at 2 sequences), described otherwise (also at 3)
    for n in (2, 3, 200):
        for code in (29, 30, 31):
            add(f"of{code}_equal_{n}", [((1 << code) + 5 * i, i % 5, i % 9) for i in range(n)])
            add(f"of{code}_mixed_{n}", [((1 << code) + i if i % 2 else 4 + i % 7, i % 5, i % 9) for i in range(n)])
    for rle in range(1, 8):           # bit a: alphabet a holds one code; the others are described
        seqs = []
        for s in _mixed(200, 300 + rle):
            s = list(s)
            for a in range(3):
                if rle >> a & 1: s[alphabet_field(a)] = (5, 6, 4)[a]
            seqs.append(tuple(s))
        add(f"rle_mask_{rle}", seqs, {"modes": {st: tuple(1 if rle >> a & 1 else 2 for a in range(3)) for st in STRATEGIES}})
    # widths: the widest sequence 16-bit length fields allow, a batch of them, a batch and one, three batches and a bit
    widest = (0xFFFFFFFF, 65535, 65535)
    add("widest_64", [widest] * 64, {"size": 536})
    add("widest_65", [widest] * 65)
    add("widest_200", [widest] * 200, {"size": 1574})
    for seed in range(5):
        rng = random.Random(900 + seed)
        add(f"widths_{seed}", [seq_of_codes(rng.randrange(MAX_LL_CODE + 1), rng.randrange(32), rng.randrange(MAX_ML_CODE + 1), rng.randrange(2))
                               for _ in range(200)])
    # 200 sequences hand bits from one step to the next three times: the five stores above cannot meet 32 alignments.  80 sequences
    # (described tables at every strategy), one hand-over and the flush each, searched by seed until every count of carried bits
    # 0..31 has its store
    need, seed = set(range(32)), 0
    while need:
        rng = random.Random(5000 + seed); seed += 1
        seqs = [seq_of_codes(rng.randrange(MAX_LL_CODE + 1), rng.randrange(32), rng.randrange(MAX_ML_CODE + 1), rng.randrange(2)) for _ in range(80)]
        k = carry_alignments(seqs, 1)[0]
        if k in need:
            need.discard(k); add(f"carry_{k}", seqs, {"carry": k})
    add("widest_16384_raw", [widest] * 16384, {"raw": True})         # a stream longer than the block: the overflow path
    # table descriptions: zero runs of 24 and more, the low-probability switch, the last code's decrement
    add("ml_0_51", [seq_of_codes(i % 5, 2 + i % 3, 51 if i % 3 == 0 else 0) for i in range(100)])
    add("of_0_31", [seq_of_codes(i % 5, 31 if i % 3 == 0 else 0, i % 9) for i in range(100)])
    add("ll_0_34", [seq_of_codes(34 if i % 3 == 0 else 0, 2 + i % 3, i % 9) for i in range(100)])
    for n1 in (2047, 2048, 2049):       # the sequences the histogram counts: one more in the store, the last code occurring twice
        seqs = [seq_of_codes(0, 2, 0)] * (n1 + 1 - 40) + [seq_of_codes(1 + i % 20, 3 + i % 20, 1 + i) for i in range(40)]
        random.Random(n1).shuffle(seqs)
        seqs.append(seqs.pop(seqs.index(seq_of_codes(0, 2, 0))))
        add(f"lowprob_{n1}", seqs, {"branch": (2, "low-1" if n1 >= 2048 else "low+1"), "modes": {st: (2, 2, 2) for st in STRATEGIES}})
    base = _mixed(150, 77)
    add("last_code_once", base + [seq_of_codes(33, 27, 50)], {"modes": {st: (2, 2, 2) for st in STRATEGIES}})
    add("last_code_twice", base[:75] + [seq_of_codes(33, 27, 50)] + base[75:] + [seq_of_codes(33, 27, 50)], {"modes": {st: (2, 2, 2) for st in STRATEGIES}})
    add("m2_uniform31_129", _spread(129, 1, 31), {"branch": (1, "M2-main")})
    add("m2_uniform35_140", _spread(140, 0, 35), {"branch": (0, "M2-main")})
    for k, (a, count, last, branch) in enumerate(M2_FOUND):
        add(f"m2_{branch[3:]}_{k}", _from_histogram(a, count, last), {"branch": (a, branch)})
    # the literal verdict is coupled to the sequence count: litSize / nbSeq >= 20 makes the block "suspect", and a suspect block of
    # 40 960 literals and more is judged by its first and last 4 KiB alone
    lits = _ramp_ended_literals(45000)
    for n, lit_type in ((0, 0), (2249, 0), (2250, 0), (2251, 2), (3000, 2)):
        add(f"ramp_45000_{n}", _flat(n), {"lits": lit_type}, lits)
    for size, lit_type in ((40959, 2), (40960, 0)):
        add(f"ramp_{size}_1000", _flat(1000), {"lits": lit_type}, _ramp_ended_literals(size))
    return cases
