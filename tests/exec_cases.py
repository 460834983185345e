"""The match-execution cases: crafted dependency chains for the three executors (exec_matches_kernel, exec_matches_wide_kernel<W>,
decode_origin.hip) and the copy routines beneath them, described for tests/zstd_forge.py.

One place for the CPU test (tests/test_exec_cases_cpu.py: the table is what it says it is, and the oracle agrees with the forge's serial
executor on every frame) and the GPU test (tests/test_gpu_exec_cases.py: every executor restores that content byte for byte).  Nothing is
committed beside this file: every frame is forged, seeded, when asked for.

A case is (name, tags, build, valid); build() -> (frame_bytes, content_bytes or None, dictionary_bytes or None).  SPECS[name] keeps what
the frame was made from (the blocks, which block is under test, the batch size it was laid out for, what it claims), so that a test can
recompute every claim from the sequence list.  Offsets are always real offsets (offset_value > 3): repeat offsets never matter here.

`rounds` is the executors' dependency rule in plain Python (decode_seq.hip, "matches, in dependency rounds").
"""
import bisect
import functools
import random
import zlib

import zstd_forge as F
from forge_cases import cblock, draw_by_weight, raw, rawlit, rle, skewed_weights

KB = (64, 128, 256, 512, 1024)              # sequences per batch: exec_matches_kernel, exec_matches_wide_kernel<2 .. 16>
TAGS = ["chain", "touch", "span", "block-edge", "copy-sweep", "literals", "dict", "negative", "padded"]
PER_KB = ("chain", "touch")                 # families built once per batch size
PAD_BLOCKS = 8
PAD = PAD_BLOCKS * F.BLOCK_MAX              # 1 MiB of RLE blocks in front: the frame becomes eligible for the origin path
DICT_SIZE = 4096
FRONT = 1024                                # the raw block in front of most blocks under test: what independent matches copy from

CASES = []          # (name, tags, build, valid)
SPECS = {}          # name -> Spec


def fresh(seed, n):
    return random.Random(seed).randbytes(n)


def seed_of(name):
    return zlib.crc32(name.encode())


def dictionary(which=0):
    """raw dictionary content; `which` picks one of several of the same size (the refMultipleDDicts test loads two)"""
    d = fresh(7700 + which, DICT_SIZE)
    assert d[:4] != (0xEC30A437).to_bytes(4, "little")
    return d


# ------------------------------------------------------------------------------------------------- the rule, in plain Python
def layout(seqs):
    """per sequence (dMatch, ml, off, ll): the block-relative start of its match, its length, its distance, the literals in front"""
    out, pos = [], 0
    for ll, ov, ml in seqs:
        assert ov > 3, "real offsets only"
        out.append((pos + ll, ml, ov - 3, ll))
        pos += ll + ml
    return out


def source(seq_layout, block_start):
    """(dictN, srcLo, srcHi) of one laid-out sequence: the bytes it takes from in front of the frame, and the block-relative interval
    the rest of the match reads before it reads its own output (min(off, mlR) bytes from dMatchR - off)"""
    d, ml, off, _ = seq_layout
    back = off - (block_start + d)
    dict_n = min(back, ml) if back > 0 else 0
    dr, mlr = d + dict_n, ml - dict_n
    return dict_n, dr - off, dr - off + min(off, mlr)


def rounds(seqs, kB, block_start):
    """per batch of kB sequences the length of the longest dependency chain: a match depends on the earlier matches of its batch whose
    output [dMatch, dMatch + ml) intersects [dMatchR - off, dMatchR - off + min(off, mlR)); a sequence whose match lies wholly in front
    of the frame (mlR == 0) neither waits nor is waited for.  Outputs lie in sequence order, so the matches met form an index interval."""
    lay = layout(seqs)
    res = []
    for base in range(0, len(lay), kB):
        batch = lay[base:base + kB]
        starts, ends, depth = [], [], []
        for q in batch:
            dict_n, lo, hi = source(q, block_start)
            if q[1] - dict_n == 0:
                d = 0
            else:
                jl, jh = bisect.bisect_right(ends, lo), bisect.bisect_left(starts, hi)
                d = 1 + (max(depth[jl:jh]) if jh > jl else 0)
            depth.append(d)
            starts.append(q[0])
            ends.append(q[0] + q[1])
        res.append(max(depth))
    return res


# --------------------------------------------------------------------------------------------------------------- specs
class Spec:
    """blocks: the frame without its padding; cb: index of the block under test; kB: the batch size it was laid out for (None: any);
    dict_size: bytes of history in front of the frame; claim: what the case says of itself (read by the CPU test);
    fix: for a negative case, (sequence index, valid offset_value) - the frame states the content size it would have with that one"""

    def __init__(self, blocks, cb, kB=None, dict_size=0, padded=False, claim=None, valid=True, fix=None):
        self.blocks, self.cb, self.kB, self.dict_size, self.padded = blocks, cb, kB, dict_size, padded
        self.claim, self.valid, self.fix = claim or {}, valid, fix

    def all_blocks(self):
        pad = [rle((0x11 * (i + 1)) & 255, F.BLOCK_MAX) for i in range(PAD_BLOCKS)] if self.padded else []
        return pad + self.blocks

    def seqs(self):
        return self.blocks[self.cb]["seqs"]

    def block_start(self):
        """frame-relative start of the block under test"""
        sizes = []
        F.execute(self.blocks[:self.cb], sizes, bytes(self.dict_size))
        return (PAD if self.padded else 0) + sum(sizes)

    def stated_size(self):
        """the content size a negative case states: what it would regenerate with its one offset one byte nearer"""
        i, ov = self.fix
        fixed = [dict(b) for b in self.blocks]
        s = list(fixed[self.cb]["seqs"])
        s[i] = (s[i][0], ov, s[i][2])
        fixed[self.cb]["seqs"] = s
        return len(F.execute(fixed, None, bytes(self.dict_size))) + (PAD if self.padded else 0)

    def forge(self, history=None, did=0, did_value=0):
        """-> (frame, content or None) behind `history` (default: the raw dictionary, for a case that has one)"""
        if history is None:
            history = dictionary() if self.dict_size else b""
        assert len(history) == self.dict_size
        kw = dict(history=history, did=did, did_value=did_value, valid=self.valid)
        if not self.valid:
            kw.update(single=True, fcs_value=self.stated_size())
        return F.frame(self.all_blocks(), **kw)

    def padded_twin(self):
        assert not self.padded
        return Spec(self.blocks, self.cb, self.kB, self.dict_size, True, self.claim, self.valid, self.fix)


def add(name, tags, spec):
    tags = [tags] if isinstance(tags, str) else list(tags)
    if spec.padded and "padded" not in tags:
        tags.append("padded")
    assert all(t in TAGS for t in tags) and name not in SPECS, name
    SPECS[name] = spec

    @functools.lru_cache(maxsize=None)
    def build():
        blob, content = spec.forge()
        return blob, content, (dictionary() if spec.dict_size else None)
    CASES.append((name, tags, build, spec.valid))


def add_padded(name, tags):
    """the same block behind PAD_BLOCKS RLE blocks of 128 KiB, each of another byte"""
    add(name + "_padded", tags, SPECS[name].padded_twin())


def block(seqs, seed, trailing=0, **kw):
    """a compressed block of these sequences over fresh raw literals"""
    return cblock(rawlit(fresh(seed, sum(s[0] for s in seqs) + trailing)), seqs, **kw)


def behind_front(seqs, name, **kw):
    """[raw block of FRONT fresh bytes, the block]"""
    return [raw(fresh(seed_of(name) ^ 1, FRONT)), block(seqs, seed_of(name), **kw)]


def from_front(pos, ll, ml, t):
    """a sequence at block-relative `pos` (its literals start there) whose match copies front-block bytes [t, t + ml): depends on nothing"""
    assert t + ml <= FRONT
    return (ll, FRONT + pos + ll - t + 3, ml)


# --------------------------------------------------------------------------------------------------------------- chain
CHAIN_ML = {64: 3, 128: 4, 256: 5, 512: 7, 1024: 8}
CHAIN_VARIANTS = ("exact", "lit", "litspan", "two")


def _chain(kB, n, variant):
    ml = CHAIN_ML[kB]
    if variant == "exact":       # each match copies exactly the match in front of it
        seqs = [(ml, ml + 3, ml)] + [(0, ml + 3, ml)] * (n - 1)
    elif variant == "lit":       # one literal in between, distance ml + 1: still exactly the match in front
        seqs = [(ml + 1, ml + 1 + 3, ml)] + [(1, ml + 1 + 3, ml)] * (n - 1)
    elif variant == "litspan":   # one literal in between, distance ml: the match in front but for its first byte, and the literal
        seqs = [(ml, ml + 3, ml)] + [(1, ml + 3, ml)] * (n - 1)
    else:                        # two sequences back: two interleaved chains
        seqs = [(2 * ml, 2 * ml + 3, ml)] + [(0, 2 * ml + 3, ml)] * (n - 1)
    return seqs


for _kB in KB:
    for _n in (_kB - 1, _kB, _kB + 1, 2 * _kB + 1):
        for _v in CHAIN_VARIANTS:
            _name = f"chain_{_v}_kb{_kB}_n{_n}"
            add(_name, "chain", Spec([block(_chain(_kB, _n, _v), seed_of(_name), trailing=2)], 0, kB=_kB,
                                     claim={"depth": "half" if _v == "two" else "full"}))
            if _kB == 1024:
                add_padded(_name, "chain")


# --------------------------------------------------------------------------------------------------------------- touch
TOUCH_RELS = (("hi_eq", False), ("hi_plus1", True), ("lo_eq", False), ("lo_minus1", True))     # (name, dependency)
TOUCH_PAIR = {"hi_eq": "hi_plus1", "hi_plus1": "hi_eq", "lo_eq": "lo_minus1", "lo_minus1": "lo_eq"}


def touch_places(kB):
    """(name, producer lane, consumer lane)"""
    w = kB // 64
    places = [("adjacent", 10, 11), ("wave_ends", 0, 63)]
    if w > 1:
        places += [("wave_seam", 64 * (w - 1) - 1, 64 * (w - 1)), ("batch_ends", 0, kB - 1)]
    return places


def _touch(kB, p, c, rel, kind):
    """kB sequences, one batch: lane p a SLOW match (kind "long": 200 bytes by the whole wave; "bytewise": 61 bytes at distance 3 by
    its lane), lane c a FAST one of 5 bytes whose source touches p's output as `rel` says; every other lane copies 3 front-block bytes"""
    seqs, pos = [], 0
    for lane in range(kB):
        if lane == p:
            s = from_front(pos, 8, 200, 17) if kind == "long" else (8, 3 + 3, 61)
            start_p = pos + 8
            end_p = start_p + s[2]
        elif lane == c:
            d = pos + 6
            off = {"hi_eq": d - (start_p - 5), "hi_plus1": d - (start_p - 5) - 1, "lo_eq": d - end_p, "lo_minus1": d - end_p + 1}[rel]
            assert off >= 5
            s = (6, off + 3, 5)
        else:
            s = from_front(pos, 8, 3, lane % 500)
        seqs.append(s)
        pos += s[0] + s[2]
    return seqs


for _kB in KB:
    for _place, _p, _c in touch_places(_kB):
        for _kind in ("long", "bytewise"):
            for _rel, _dep in TOUCH_RELS:
                _name = f"touch_{_place}_{_kind}_{_rel}_kb{_kB}"
                _pair = f"touch_{_place}_{_kind}_{TOUCH_PAIR[_rel]}_kb{_kB}"
                # (both frames of a pair over the same bytes: they differ in the one offset alone)
                _seed = f"touch_{_place}_{_kind}_{_rel[:2]}_kb{_kB}"
                add(_name, "touch", Spec(behind_front(_touch(_kB, _p, _c, _rel, _kind), _seed, trailing=1), 1, kB=_kB,
                                         claim={"p": _p, "c": _c, "rel": _rel, "dep": _dep, "pair": _pair}))
    add_padded(f"touch_wave_ends_long_hi_plus1_kb{_kB}", "touch")


# ---------------------------------------------------------------------------------------------------------------- span
def _span(n, first, last, consumer):
    """n sequences; the consumer's source runs from the start of lane `first`'s match to the end of lane `last`'s: it waits for every
    match in between, a long one in lane first + 2 (by the whole wave) and a byte-wise one in lane `last` among them"""
    seqs, pos = [], 0
    for lane in range(n):
        if lane == first + 2:
            s = from_front(pos, 2, 300, 100)
        elif lane == last:
            s = (4, 3 + 3, 61)
        elif lane == consumer:
            d = pos + 2
            s = (2, d - start + 3, end - start)
        else:
            s = from_front(pos, 2, 4, lane % 700)
        if lane == first:
            start = pos + s[0]
        if lane == last:
            end = pos + s[0] + s[2]
        seqs.append(s)
        pos += s[0] + s[2]
    return seqs


def _span_lits(n, a):
    """lane a + 1 has 40 literals in front of its match; the last lane copies exactly those: between two match outputs, touching both,
    depending on neither"""
    seqs, pos = [], 0
    for lane in range(n):
        if lane == a + 1:
            lo = pos
            s = from_front(pos, 40, 4, 50)
        elif lane == n - 1:
            s = (2, pos + 2 - lo + 3, 40)
        else:
            s = from_front(pos, 2, 70 if lane == a else 4, lane % 700)
        seqs.append(s)
        pos += s[0] + s[2]
    return seqs


for _n, _first, _last, _cons in ((64, 3, 40, 45), (128, 3, 100, 110), (256, 3, 232, 242), (512, 3, 488, 498), (1024, 3, 1000, 1010)):
    _name = f"span_lanes_{_first}_{_last}_kb{_n}"
    add(_name, "span", Spec(behind_front(_span(_n, _first, _last, _cons), _name, trailing=3), 1, kB=_n,
                            claim={"c": _cons, "jl": _first, "jh": _last + 1, "rounds": [2]}))
    add_padded(_name, "span")
    _name = f"span_literals_only_kb{_n}"
    add(_name, "span", Spec(behind_front(_span_lits(_n, _n // 2 - 1), _name), 1, kB=_n,
                            claim={"c": _n - 1, "jl": _n // 2, "jh": _n // 2, "rounds": [1]}))
    add_padded(_name, "span")


# ---------------------------------------------------------------------------------------------------------- block-edge
# the block under test is the second of its frame, behind the raw front block: block-relative sources below 0 lie in that block
def _edge_lane0(off, ml):
    seqs, pos = [(4, off + 3, ml)], 4 + ml
    for lane in range(1, 70):
        seqs.append(from_front(pos, 1, 3, lane))
        pos += 4
    return seqs


add("edge_ends_at_block_start", "block-edge", Spec(behind_front(_edge_lane0(9, 5), "edge_a"), 1, claim={"seq": 0, "rel": "ends_at_start", "rounds": [1, 1]}))
add("edge_straddles_block_start", "block-edge", Spec(behind_front(_edge_lane0(6, 5), "edge_b"), 1, claim={"seq": 0, "rel": "straddles", "rounds": [1, 1]}))
add("edge_starts_at_block_start", "block-edge", Spec(behind_front(_edge_lane0(4, 5), "edge_c"), 1, claim={"seq": 0, "rel": "starts_at_start", "rounds": [1, 1]}))
# lane 0 a long match at [1, 71); lane 1 reads [-3, 5): three bytes of the front block, lane 0's literal and four bytes of its match
add("edge_straddles_block_start_into_a_match", "block-edge",
    Spec(behind_front([from_front(0, 1, 70, 200), (2, 76 + 3, 8)] + [from_front(81 + 4 * i, 1, 3, i) for i in range(70)], "edge_d"), 1,
         claim={"seq": 1, "rel": "straddles", "rounds": [2, 1]}))


def _edge_batch2_first(kB):
    """kB + 1 sequences: the last of batch 1 a long match, the first of batch 2 reads its last 6 bytes"""
    seqs, pos = [], 0
    for lane in range(kB - 1):
        seqs.append(from_front(pos, 1, 3, lane % 500))
        pos += 4
    seqs.append(from_front(pos, 2, 100, 300))
    return seqs + [(1, 7 + 3, 6)]


def _edge_straddles_batch(kB):
    """kB + 3 sequences: sequence kB + 2 reads from the start of sequence kB - 2's match to the end of sequence kB + 1's - two matches
    of the batch before (complete) and two of its own batch (a dependency)"""
    seqs, pos = [], 0
    for lane in range(kB + 2):
        s = from_front(pos, 1, 66 if lane == kB - 1 else 3, lane % 500)
        if lane == kB - 2:
            start = pos + 1
        seqs.append(s)
        pos += s[0] + s[2]
    return seqs + [(1, pos + 1 - start + 3, pos - start)]


for _kB in KB:
    add(f"edge_batch2_first_reads_batch1_last_kb{_kB}", "block-edge",
        Spec(behind_front(_edge_batch2_first(_kB), f"edge_e{_kB}"), 1, kB=_kB, claim={"seq": _kB, "rel": "inside_previous", "rounds": [1, 1]}))
    add(f"edge_source_straddles_batches_kb{_kB}", "block-edge",
        Spec(behind_front(_edge_straddles_batch(_kB), f"edge_f{_kB}"), 1, kB=_kB, claim={"seq": _kB + 2, "rel": "straddles_batches", "rounds": [1, 2]}))


# ---------------------------------------------------------------------------------------------------------- copy-sweep
SWEEP_ML = (3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 3087, 3088, 4096, 4111)
SWEEP_OFF = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def sweep_pairs():
    return [(ml, off) for ml in SWEEP_ML for off in sorted(set(SWEEP_OFF + (ml - 1, ml, ml + 1)))]


def _sweep_blocks():
    """the pairs in order, cut where a block would pass 120 KiB: each sequence `off` fresh literals, then ml bytes at distance off"""
    blocks, cur, size = [], [], 0
    for ml, off in sweep_pairs():
        if size + ml + off > 120 * 1024:
            blocks.append(cur)
            cur, size = [], 0
        cur.append((off, off + 3, ml))
        size += ml + off
    return blocks + [cur]


for _i, _seqs in enumerate(_sweep_blocks()):
    add(f"copy_sweep_{_i}", "copy-sweep", Spec([block(_seqs, 4400 + _i, trailing=5)], 0, claim={"rounds": 1}))
add_padded("copy_sweep_0", "copy-sweep")


# ------------------------------------------------------------------------------------------------------------ literals
LIT_RUNS = (0, 1, 2, 3, 4, 7, 8, 9, 16, 17, 31, 32, 33, 47, 48, 49, 255, 4096)
LIT_PIECES = (255, 256, 257, 513)
LIT_TRAILING = (0, 1, 63, 64, 65, 4111)
LIT_KINDS = ("raw", "rle", "huf", "treeless")
LIT_FRONT = 64


def _pieces_runs(total, seed):
    """64 literal runs above 32 bytes whose 16-byte pieces (the last of a run pulled back over the one before) add up to `total`"""
    base, extra = (4, total - 63 * 4) if total < 500 else (8, total - 63 * 8)
    r = random.Random(seed)
    return [r.randrange(16 * k - 15, 16 * k + 1) for k in [base] * 63 + [extra]]


def _lit_frame(lls, trailing, kind, name):
    """[raw front of LIT_FRONT bytes, (for treeless: a block that defines the Huffman table,) the block]: every match 4 front bytes"""
    seed = seed_of(name)
    blocks = [raw(fresh(seed ^ 1, LIT_FRONT))]
    w = skewed_weights(9, 30, 77)
    have = LIT_FRONT
    if kind == "treeless":
        blocks.append(cblock({"k": "huf", "data": draw_by_weight(seed ^ 2, w, 200), "w": w, "streams": 4}, [(10, 4 + 3, 5)]))
        have += 205
    seqs, pos = [], 0
    for i, ll in enumerate(lls):
        seqs.append((ll, have + pos + ll - (i % 50) + 3, 4))
        pos += ll + 4
    n = sum(lls) + trailing
    if kind == "raw":
        lit = rawlit(fresh(seed, n))
    elif kind == "rle":
        lit = {"k": "rle", "data": bytes([0xC3]) * n, "sf": None}
    elif kind == "huf":
        lit = {"k": "huf", "data": draw_by_weight(seed, w, n), "w": w, "streams": 4}
    else:
        lit = {"k": "treeless", "data": draw_by_weight(seed, w, n), "streams": 4}
    blocks.append(cblock(lit, seqs))
    return blocks


for _kind in LIT_KINDS:
    _cb = 2 if _kind == "treeless" else 1
    _name = f"lit_runs_{_kind}"
    add(_name, "literals", Spec(_lit_frame(LIT_RUNS, 7, _kind, _name), _cb, claim={"runs": LIT_RUNS, "kind": _kind}))
    for _p in LIT_PIECES:
        _name = f"lit_pieces_{_p}_{_kind}"
        add(_name, "literals", Spec(_lit_frame(_pieces_runs(_p, _p), 3, _kind, _name), _cb, claim={"pieces": _p, "kind": _kind}))
    for _t in LIT_TRAILING:
        _name = f"lit_trailing_{_t}_{_kind}"
        add(_name, "literals", Spec(_lit_frame([5, 9, 40, 2, 33, 12], _t, _kind, _name), _cb, claim={"trailing": _t, "kind": _kind}))


# ---------------------------------------------------------------------------------------------------------------- dict
# one compressed block at the frame's start, DICT_SIZE bytes of history in front of it.  Sequence 0 lays 128 literals (what the part
# of a match behind the dictionary part copies: the frame's first bytes); sequence 1 is the match under test: `back` bytes into the
# dictionary, `ml` long
def _dict_seqs(back, ml, extra=(), base=0):
    """base: what the frame holds in front of the block"""
    seqs = [(128, 100 + 3, 4), (2, base + 134 + back + 3, ml)]
    return seqs + list(extra)


DICT_BACKS = (1, 63, 64, 65, 200, DICT_SIZE)
DICT_REST = (0, 1, 30, 100)                 # bytes of the match behind its dictionary part: none, one, a lane's copy, the wave's


def _add_dict(name, back, ml, claim, extra=()):
    """the case, and the same block behind the padding: the match then reaches over 1 MiB of frame into the dictionary"""
    for tail, padded in (("", False), ("_padded", True)):
        seqs = _dict_seqs(back, ml, extra, PAD if padded else 0)
        add(name + tail, "dict", Spec([block(seqs, seed_of(name), trailing=4)], 0, dict_size=DICT_SIZE, padded=padded, claim=claim))


for _back in DICT_BACKS + (2,):
    for _rest in DICT_REST:
        # (back in {ml - 1, ml}: rest 1 and rest 0;  off == position + dictSize exactly: back == DICT_SIZE)
        if _back + _rest >= 3:
            _add_dict(f"dict_back{_back}_rest{_rest}", _back, _back + _rest, {"back": _back, "dict_n": _back, "rest": _rest})
for _back in (4, 64, 65, 66, 200, DICT_SIZE):
    # back == ml + 1: the whole match lies in the dictionary, one byte short of its end
    _add_dict(f"dict_back{_back}_inside", _back, _back - 1, {"back": _back, "dict_n": _back - 1, "rest": 0})
# a later lane of the same batch copies the dictionary part that an earlier lane just wrote: from a match wholly out of the dictionary
# (which is nobody's dependency), and from one that goes on in the frame (which is)
_add_dict("dict_part_copied_by_later_lane_whole", 300, 90, {"back": 300, "dict_n": 90, "rest": 0, "reader": 2, "rounds": [1]}, [(1, 91 + 3, 90)])
_add_dict("dict_part_copied_by_later_lane_partial", 90, 120, {"back": 90, "dict_n": 90, "rest": 30, "reader": 2, "rounds": [2]}, [(1, 121 + 3, 90)])
# the frame's FIRST match: 40 bytes out of the dictionary, then 30 more from the frame's first byte on - its own two literals and its
# own dictionary part.  Its source interval holds its own output: the one place where "earlier lanes only" (the lane mask of the
# one-wave executor, the wide one's clamp of jh to the thread) decides anything, since everywhere else a source ends where its match starts
add("dict_rest_copies_own_dict_part", "dict", Spec([block([(2, 2 + 40 + 3, 70), (1, 20 + 3, 9)], 8801, trailing=4)], 0, dict_size=DICT_SIZE,
                                                   claim={"seq": 0, "back": 40, "dict_n": 40, "rest": 30, "holds_itself": True}))


# ------------------------------------------------------------------------------------------------------------ negative
# off == position (+ dictSize) + 1: one byte in front of everything there is
def _neg_first_block(n, bad, before=0):
    """n sequences, each copying the 3 literals in front of it; sequence `bad` reaches one byte too far: `before` is everything in
    front of the block (dictionary, padding, earlier blocks)"""
    seqs = [(3, 3 + 3, 3)] * n
    seqs[bad] = (3, 6 * bad + 3 + before + 1 + 3, 3)
    return seqs


def _add_neg(name, spec):
    add(name, "negative", spec)


_add_neg("neg_lane0_first_batch", Spec([block(_neg_first_block(10, 0), 1)], 0, valid=False, fix=(0, 6)))
_add_neg("neg_lane0_first_batch_dict", Spec([block(_neg_first_block(10, 0, DICT_SIZE), 1)], 0, dict_size=DICT_SIZE, valid=False, fix=(0, 6)))
for _kB in KB:
    _add_neg(f"neg_last_lane_of_batch_kb{_kB}", Spec([block(_neg_first_block(_kB + 5, _kB - 1), 2)], 0, kB=_kB, valid=False, fix=(_kB - 1, 6)))
    if _kB > 64:
        _add_neg(f"neg_lane_in_last_wave_kb{_kB}", Spec([block(_neg_first_block(_kB, _kB - 10), 3)], 0, kB=_kB, valid=False, fix=(_kB - 10, 6)))
_add_neg("neg_last_lane_of_batch_dict", Spec([block(_neg_first_block(64, 63, DICT_SIZE), 4)], 0, kB=64, dict_size=DICT_SIZE, valid=False, fix=(63, 6)))
_add_neg("neg_first_of_second_block", Spec([raw(fresh(5, 100)), block(_neg_first_block(2, 0, 100), 5)], 1, valid=False, fix=(0, 6)))
_add_neg("neg_lane_in_last_wave_kb1024_padded", Spec([block(_neg_first_block(1024, 1014, PAD), 3)], 0, kB=1024, padded=True, valid=False, fix=(1014, 6)))
_add_neg("neg_first_of_second_block_padded", Spec([raw(fresh(5, 100)), block(_neg_first_block(2, 0, PAD + 100), 5)], 1, padded=True, valid=False, fix=(0, 6)))


# ------------------------------------------------------------------------------------------------- behind the padding
# one sequence of a whole block: a copy from 1 MiB back (the first RLE block), and the last byte 131072 times - a chain 128 Ki bytes
# deep for the origin path's jump rounds and finished regions
add("pad_copy_from_1mib_back", "padded", Spec([cblock(rawlit(b""), [(0, PAD + 3, F.BLOCK_MAX)])], 0, padded=True, claim={"rounds": [1]}))
add("pad_offset_1_whole_block", "padded", Spec([cblock(rawlit(b""), [(0, 1 + 3, F.BLOCK_MAX)])], 0, padded=True, claim={"rounds": [1]}))


def by_tag(tag, valid=True):
    return [c for c in CASES if tag in c[1] and c[3] == valid]
