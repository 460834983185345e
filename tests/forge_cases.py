"""The forged-frame cases: every corner of the decoder that no encoder here writes, described for tests/zstd_forge.py.

One place for the generator (tests/golden/make_golden_forge.py), the CPU test and the GPU test.  A case is
(name, tags, build, valid): build() -> (frame_bytes, content_bytes or None); `valid` is the FORGE's belief (the format's
words), the verdicts of libzstd and the oracle are recorded beside it in tests/golden/manifest_forge.json.

To add a corner: describe it here with add(...), rerun tests/golden/make_golden_forge.py on the authoring machine, and check
that its tag has an agreed case (the generator asserts it).
"""
import random
import zlib

import zstd_forge as F

TAGS = ["huf-log12", "huf-direct", "huf-fse-255", "huf-treeless-gap", "lit-size-formats", "fse-logs", "fse-lowprob",
        "fse-one-heavy", "fse-zero-runs", "seq-modes", "seq-zero-bits", "seq-repeat-gap", "seq-max-bits", "nbseq-3byte",
        "nbseq-2byte", "repcodes", "overlap", "header-forms", "skippable", "long-frame", "negatives"]

CASES = []          # (name, tags, build, valid)


def add(name, tags, build, valid=True):
    tags = [tags] if isinstance(tags, str) else list(tags)
    assert all(t in TAGS for t in tags) and name not in [c[0] for c in CASES]
    CASES.append((name, tags, build, valid))


# ------------------------------------------------------------------------------------------------------------- helpers
def rbytes(seed, n, alphabet=256):
    r = random.Random(seed)
    return bytes(r.randrange(alphabet) for _ in range(n))


def raw(data):
    return {"t": "raw", "data": bytes(data)}


def rle(byte, size):
    return {"t": "rle", "byte": byte, "size": size}


def cblock(lit, seqs=(), **kw):
    return dict(t="c", lit=lit, seqs=list(seqs), **kw)


def rawlit(data, sf=None):
    return {"k": "raw", "data": bytes(data), "sf": sf}


def rlelit(byte, n, sf=None):
    return {"k": "rle", "data": bytes([byte]) * n, "sf": sf}


def lits_needed(seqs, extra=0):
    return sum(s[0] for s in seqs) + extra


def fse_mode(kind, seqs, log):
    """a compressed table fitted to the codes these sequences use"""
    i = ("ll", "of", "ml").index(kind)
    codes = [F.seq_codes(s)[i][0] for s in seqs]
    counts = [0] * (max(codes) + 1)
    for c in codes:
        counts[c] += 1
    return ("fse", F.normalize(counts, log), log)


def skewed_weights(log, nsym, seed):
    """nsym Huffman weights whose longest code is `log` bits: the chain log, log-1, .., 2, 1, 1 with symbols split in two"""
    r = random.Random(seed)
    w = list(range(log, 0, -1)) + [1]
    while len(w) < nsym:
        cands = [k for k, x in enumerate(w) if x >= 2]
        if not cands:                             # 2^log symbols of weight 1: the alphabet is full
            break
        i = r.choice(cands)
        w[i] -= 1
        w.append(w[i])
    r.shuffle(w)
    if w[-1] == 0:
        w.append(0)
    return w


def draw_by_weight(seed, w, n):
    """n symbols, each symbol of weight > 0 at least once, drawn in proportion to 2^weight"""
    r = random.Random(seed)
    syms = [s for s, x in enumerate(w) if x]
    out = r.choices(syms, [1 << w[s] for s in syms], k=max(n - len(syms), 0)) + syms
    r.shuffle(out)
    return bytes(out[:n]) if n >= len(syms) else bytes(r.choices(syms, k=n))


def gen_seqs(r, n, have, ll=None, ofcode=None, ml=None, repshare=0.3, maxll=12, maxml=24):
    """n valid sequences for a block that starts with `have` bytes of the frame in front of it and the start repeat offsets
    `rep` unknown to us: repeat offsets are used only once three real offsets of this block have replaced them"""
    seqs, pos, real = [], have, 0
    rep = [1, 4, 8]
    for _ in range(n):
        l = ll if ll is not None else r.choice([0, 0, 1, 2, 3, 5, 8, maxll, r.randrange(maxll + 1)])
        if pos + l == 0:
            l = 1
        m = ml if ml is not None else r.choice([3, 3, 4, 5, 7, 8, 16, maxml, r.randrange(3, maxml + 1)])
        pos += l
        if ofcode is not None:
            lo, hi = max((1 << ofcode), 4), (2 << ofcode) - 1
            ov = r.randrange(lo, min(hi, pos + 3) + 1)
        elif real >= 3 and r.random() < repshare:
            ov = r.randrange(1, 4)
            try:
                off, _ = F.rep_step(rep, l, ov)
            except F.ForgeInvalid:
                off = pos + 1
            if off > pos:
                ov = r.randrange(1, pos + 1) + 3
        else:
            ov = r.randrange(1, min(pos, 5000) + 1) + 3
        off, rep = F.rep_step(rep, l, ov)
        assert off <= pos
        if ov > 3:
            real += 1
        seqs.append((l, ov, m))
        pos += m
    return seqs


def frame(blocks, **kw):
    return F.frame(blocks, **kw)


# sequences that name every code gen_seqs may draw: a table fitted to a block's sequences plus these can be repeated by any later block
PADS = {"ll": [(l, 9, 3) for l in range(0, 30)], "of": [(1, 1, 3), (1, 2, 3)] + [(1, 1 << c, 3) for c in range(2, 14)],
        "ml": [(1, 9, x) for x in range(3, 60)]}


# ------------------------------------------------------------------------------------------------------------ Huffman
def _huf_case(log, n, streams, enc, seed=7):
    def build():
        w = skewed_weights(log, 40, seed) if log > 1 else [1, 1]
        assert F.huf_table_log(w) == log
        data = draw_by_weight(seed + n, w, n)
        seqs = [(n // 3, 4 + 3, 9), (n // 3, 1, 5)]
        return frame([cblock({"k": "huf", "data": data, "w": w, "enc": enc, "streams": streams}, seqs)], checksum=True)
    return build


for _log in (12, 11, 10, 1):
    for _n, _streams in ((300, 1), (1023, 1), (300, 4), (5000, 4)):
        # (a single-stream section holds at most 1023 literals: the 10-bit size field is its only form)
        _enc = "fse" if (_log in (12, 10) and _streams == 4) or (_log == 11 and _streams == 1) else "direct"
        if _log == 1:
            _enc = "direct"
        add(f"huf_log{_log}_{_n}_s{_streams}", ["huf-log12"], _huf_case(_log, _n, _streams, _enc))


def _direct_case(w):
    def build():
        data = draw_by_weight(3, w, 200)
        return frame([cblock({"k": "huf", "data": data, "w": w, "enc": "direct", "streams": 1}, [(50, 5, 4)])])
    return build


add("huf_direct_2sym_odd", "huf-direct", _direct_case([1, 1]))                    # 1 stored weight
add("huf_direct_2sym_even", "huf-direct", _direct_case([1, 0, 1]))                 # 2 stored weights
add("huf_direct_3sym_even", "huf-direct", _direct_case([1, 1, 2]))                 # 2 stored
add("huf_direct_3sym_odd", "huf-direct", _direct_case([2, 0, 1, 1]))               # 3 stored
add("huf_direct_3sym_w3", "huf-direct", _direct_case([3, 0, 0, 2, 0, 1, 0, 0, 1]))   # table log 3 from 3 + 1 symbols, 8 stored
add("huf_direct_128", "huf-direct", _direct_case([1] * 128 + [8]))                # header byte 255


def _fse255():
    r = random.Random(255)
    w = [1] * 100 + [2] * 105 + [3] * 50
    r.shuffle(w)
    w.append(2)                                   # the implied 256th: 100 + 210 + 200 = 510, two short of 512
    assert F.huf_table_log(w) == 9
    data = draw_by_weight(9, w, 3000)
    return frame([cblock({"k": "huf", "data": data, "w": w, "enc": "fse", "streams": 4}, [(100, 9, 30)])], checksum=True)


add("huf_fse_255", "huf-fse-255", _fse255)


def _treeless_gap(streams, spread):
    def build():
        w = skewed_weights(9, 30, 5)
        d0, d4 = draw_by_weight(1, w, 900), draw_by_weight(2, w, 700)
        b0 = cblock({"k": "huf", "data": d0, "w": w, "enc": "fse", "streams": 4}, [(10, 6, 20), (5, 1, 8)])
        b4 = cblock({"k": "treeless", "data": d4, "streams": streams}, [(3, 1000 + 3, 40), (0, 2, 6)])
        mid = [raw(rbytes(4, 300)), cblock(rawlit(rbytes(5, 100)), [(20, 500 + 3, 10)]), rle(0x41, 5000)]
        if spread:                                # more in between: a compressed block without sequences, and RLE literals
            mid += [cblock(rlelit(0x42, 77)), cblock(rawlit(b"+")), raw(b"z")]
        return frame([b0] + mid + [b4], checksum=True)
    return build


add("huf_treeless_gap_s1", "huf-treeless-gap", _treeless_gap(1, False))
add("huf_treeless_gap_s4", "huf-treeless-gap", _treeless_gap(4, False))
add("huf_treeless_gap_far_s1", "huf-treeless-gap", _treeless_gap(1, True))
add("huf_treeless_gap_far_s4", "huf-treeless-gap", _treeless_gap(4, True))


# ------------------------------------------------------------------------------------------------ literals size formats
def _rawrle_lit(kind, n, sf):
    def build():
        lit = rawlit(rbytes(n, n), sf) if kind == "raw" else rlelit(0x5A, n, sf)
        seqs = [(n, 1 + 3, 3)] if n < 131072 - 3 else []
        return frame([cblock(lit, seqs)])
    return build


for _kind in ("raw", "rle"):
    for _n, _sf in ((31, 0), (31, 1), (31, 3), (32, 1), (4095, 1), (4095, 3), (4096, 3)):
        add(f"lit_{_kind}_{_n}_sf{_sf}", "lit-size-formats", _rawrle_lit(_kind, _n, _sf))
add("lit_rle_131072_sf3", "lit-size-formats", _rawrle_lit("rle", 131072, 3))
add("lit_rle_0_sf0", "lit-size-formats", lambda: frame([raw(b"ab"), cblock(rawlit(b"", 0), [(0, 2 + 3, 5)])]))


def _huf_lit(n, streams, sf):
    def build():
        w = skewed_weights(8, 20, 8)
        data = draw_by_weight(n, w, n)
        return frame([cblock({"k": "huf", "data": data, "w": w, "enc": "direct", "streams": streams, "sf": sf},
                             [(n - 5, 3 + 3, 7)])], checksum=True)
    return build


for _n, _streams, _sf in ((1023, 1, 0), (1023, 4, 1), (1023, 4, 2), (1024, 4, 2), (16383, 4, 2), (16383, 4, 3), (16384, 4, 3),
                          (100000, 4, 3)):
    add(f"lit_huf_{_n}_s{_streams}_sf{_sf}", "lit-size-formats", _huf_lit(_n, _streams, _sf))


# ------------------------------------------------------------------------------------------------------------ FSE tables
def _fse_log_case(kind, log, nseq=70):
    def build():
        r = random.Random(log * 10 + len(kind))
        front = raw(rbytes(6, 200))
        seqs = gen_seqs(r, nseq, 200, maxll=40 if kind == "ll" else 12, maxml=90 if kind == "ml" else 24)
        blk = cblock(rawlit(rbytes(7, lits_needed(seqs, 5))), seqs)
        blk[kind] = fse_mode(kind, seqs, log)
        return frame([front, blk])
    return build


for _kind, _mx in (("ll", 9), ("of", 8), ("ml", 9)):
    add(f"fse_{_kind}_log5", "fse-logs", _fse_log_case(_kind, 5))
    add(f"fse_{_kind}_log{_mx}", "fse-logs", _fse_log_case(_kind, _mx))


def _fse_all_logs(logs):
    def build():
        r = random.Random(sum(logs))
        seqs = gen_seqs(r, 129, 300)
        blk = cblock(rawlit(rbytes(8, lits_needed(seqs))), seqs, ll=fse_mode("ll", seqs, logs[0]),
                     of=fse_mode("of", seqs, logs[1]), ml=fse_mode("ml", seqs, logs[2]))
        return frame([raw(rbytes(9, 300)), blk])
    return build


add("fse_all_log5", "fse-logs", _fse_all_logs((5, 5, 5)))
add("fse_all_logmax", "fse-logs", _fse_all_logs((9, 8, 9)))


def _lowprob():
    # match-length table of log 9: 25 symbols "less than one", the rest shared out
    norm = [-1] * 25 + [0] * 28
    norm[30], norm[31], norm[40] = 400, 80, 7                # 25 + 487 = 512
    r = random.Random(25)
    mls = [r.choice(list(range(3, 28)) + [33, 33, 33, 34, 70]) for _ in range(100)]
    ll_norm = [-1] * 20 + [12]                               # literal-length table of log 5, 20 low-probability symbols
    seqs = [(r.randrange(20) if i % 3 else 20, 3 + 3, m) for i, m in enumerate(mls)]
    seqs[0] = (20, 4 + 3, mls[0])
    return frame([cblock(rawlit(rbytes(10, lits_needed(seqs))), seqs, ml=("fse", norm, 9), ll=("fse", ll_norm, 5))])


add("fse_lowprob", "fse-lowprob", _lowprob)


def _one_heavy(low):
    def build():
        # every table: one symbol owns all cells but one
        ll = ("fse", [511, low], 9)                          # literal lengths 0 (heavy) and 1
        of = ("fse", [0, 0, 255, low], 8)                    # offset codes 2 (heavy) and 3
        ml = ("fse", [low, 31], 5)                           # match lengths 3 and 4 (heavy)
        seqs = [(0, 5, 4)] * 30 + [(1, 9, 3)] + [(0, 6, 4)] * 30 + [(0, 12, 4), (1, 4, 4)] + [(0, 7, 4)] * 5
        return frame([raw(rbytes(11, 40)), cblock(rawlit(b"QR"), seqs, ll=ll, of=of, ml=ml)])
    return build


add("fse_one_heavy_1", "fse-one-heavy", _one_heavy(1))
add("fse_one_heavy_lowprob", "fse-one-heavy", _one_heavy(-1))


def _zero_runs():
    ml = [0] * 53
    for i, c in ((0, 20), (2, 10), (6, 10), (11, 8), (19, 8), (45, 8)):     # gaps of 1, 3, 4, 7 and 25 zeros
        ml[i] = c
    ll = [0] * 36
    for i, c in ((0, 10), (7, 10), (14, 6), (35, 6)):                       # gaps of 6, 6 and 20 zeros
        ll[i] = c
    of = [0, 0, 0, 16, 0, 0, 0, 0, 0, 0, 16]                                # leading zeros, then a gap of 6
    r = random.Random(3)
    seqs = []
    for i in range(40):
        l = r.choice([0, 7, 14])
        m = r.choice([3, 5, 9, 14, 22, 515 + r.randrange(100)])
        ov = r.choice([8, 11, 15]) if i < 12 else r.choice([8, 15, 1024, 1500])
        seqs.append((l, ov, m))
    seqs[0] = (65536, 9, 3)                                                 # the longest literal-length code, and room for offsets
    return frame([raw(rbytes(12, 20)), cblock(rlelit(0x33, lits_needed(seqs, 1)), seqs, ll=("fse", ll, 5), of=("fse", of, 5),
                                              ml=("fse", ml, 6))])


add("fse_zero_runs", "fse-zero-runs", _zero_runs)


# ------------------------------------------------------------------------------------------------------------- sequences
def _seq_modes(ml_, of_, mm_):
    def build():
        r = random.Random(zlib.crc32((ml_ + of_ + mm_).encode()))
        blocks, have = [raw(rbytes(13, 64))], 64
        for n in (1, 2, 63, 64, 65, 129):
            seqs = gen_seqs(r, n, have, ll=2 if ml_ == "rle" else None, ofcode=5 if of_ == "rle" else None,
                            ml=4 if mm_ == "rle" else None)
            kw = {}
            for kind, m in (("ll", ml_), ("of", of_), ("ml", mm_)):
                kw[kind] = "predef" if m == "predef" else ("rle",) if m == "rle" else fse_mode(kind, seqs, {"ll": 7, "of": 6, "ml": 8}[kind])
            lits = rbytes(n, lits_needed(seqs, 3))
            blocks.append(cblock(rawlit(lits), seqs, **kw))
            have += len(lits) + sum(s[2] for s in seqs)
        return frame(blocks, checksum=True)
    return build


for _a in ("predef", "rle", "fse"):
    for _b in ("predef", "rle", "fse"):
        for _c in ("predef", "rle", "fse"):
            add(f"seq_modes_{_a}_{_b}_{_c}", "seq-modes", _seq_modes(_a, _b, _c))


def _zero_bits(n):
    def build():
        seqs = [(1, 1, 3)] * n
        return frame([cblock(rawlit(rbytes(n, n)), seqs, ll=("rle",), of=("rle",), ml=("rle",))])
    return build


for _n in (1, 64, 200):
    add(f"seq_zero_bits_{_n}", "seq-zero-bits", _zero_bits(_n))


def _repeat_gap(define):
    def build():
        r = random.Random(len(define))
        fixed = dict(ll=2, ofcode=5, ml=4) if define == "rle" else {}
        have = [0]

        def blk(modes, n=20, nolits=False, **over):
            seqs = gen_seqs(r, n, have[0], **dict(fixed, **over))
            lits = rbytes(have[0], lits_needed(seqs, 2))
            have[0] += len(lits) + sum(s[2] for s in seqs)
            return cblock(rawlit(lits), seqs, **modes), seqs

        def other(n):
            have[0] += n

        def mode(kind, seqs):
            return "predef" if define == "predef" else ("rle",) if define == "rle" else fse_mode(kind, seqs + PADS[kind], 7)
        blocks = [raw(rbytes(14, 100))]; other(100)
        # one set of sequences for the whole frame's tables: a repeated table must be able to code every later block, so with
        # compressed tables the defining block's distribution is fitted to a sample drawn the same way
        sample = gen_seqs(random.Random(99), 400, 100, **fixed)
        b0, s0 = blk({}, 20)
        for kind in ("ll", "of", "ml"):
            b0[kind] = mode(kind, sample + s0) if define == "fse" else mode(kind, s0)
        rep3 = dict(ll="repeat", of="repeat", ml="repeat")
        blocks.append(b0)
        blocks.append(raw(rbytes(15, 50))); other(50)
        blocks.append(blk(rep3)[0])
        blocks.append(rle(0x77, 300)); other(300)
        blocks.append(blk(rep3)[0])
        blocks.append(cblock(rawlit(b"no sequences here")) ); other(17)
        blocks.append(blk(rep3)[0])
        # redefine ONLY the match-length table; LL and OF are repeated beside it
        b = blk(dict(ll="repeat", of="repeat"), ml=9)[0]
        b["ml"] = ("rle",)
        blocks.append(b)
        blocks.append(blk(rep3, ml=9)[0])
        # then only the literal-length table
        b = blk(dict(of="repeat", ml="repeat"), ml=9, ll=5)[0]
        b["ll"] = ("rle",)
        blocks.append(b)
        blocks.append(blk(rep3, ml=9, ll=5)[0])
        # then only the offset table
        b = blk(dict(ll="repeat", ml="repeat"), ml=9, ll=5, ofcode=4)[0]
        b["of"] = "predef"
        blocks.append(b)
        blocks.append(blk(rep3, ml=9, ll=5)[0])
        return frame(blocks, checksum=True)
    return build


for _d in ("fse", "rle", "predef"):
    add(f"seq_repeat_gap_{_d}", "seq-repeat-gap", _repeat_gap(_d))


def _max_bits(ofcode, front_blocks):
    def build():
        # the format's ceiling for a block of 130 sequences: a block regenerates at most 128 KiB, so LL code 35 and ML code 52
        # cannot meet in one sequence, let alone in 130.  One sequence takes the two 15/16-bit codes the limit allows, 130 more
        # take 8 + 9 + ofcode extra bits and full-width (9/9/8 bit) state updates: every coded symbol is "less than one".
        r = random.Random(ofcode)
        blocks = [rle(i & 255, 131072) for i in range(front_blocks)] + [raw(rbytes(16, 200))]
        lo, hi = 1 << ofcode, min((2 << ofcode) - 1, front_blocks * 131072 + 200)
        big = [(65536, r.randrange(lo, hi), 32771 + 100)]
        blocks.append(cblock(rlelit(0x10, 65536 + 1), big, ll=("fse", [-1] * 35 + [477], 9), of=("fse", [0] * ofcode + [-1, 255], 8),
                             ml=("fse", [-1] * 52 + [460], 9)))
        seqs = [(256 + r.randrange(64), r.randrange(lo, hi), 515 + r.randrange(100)) for _ in range(130)]
        ll = [0] * 36; ll[27] = -1; ll[0] = 511
        ml = [0] * 53; ml[45] = -1; ml[0] = 511
        of = [255] + [0] * (ofcode - 1) + [-1]
        blocks.append(cblock(rlelit(0x11, lits_needed(seqs, 7)), seqs, ll=("fse", ll, 9), of=("fse", of, 8), ml=("fse", ml, 9)))
        return frame(blocks, checksum=True)
    return build


add("seq_max_bits_of20", "seq-max-bits", _max_bits(20, 9))
add("seq_max_bits_of24", "seq-max-bits", _max_bits(24, 129))


def _nbseq(n, form=None):
    def build():
        # offset 61 once, then the first repeat offset: the offset table gives code 0 all cells but one
        seqs = [(1, 61 + 3, 3)] + [(1, 1, 3)] * (n - 1)
        blk = cblock(rlelit(0x78, n), seqs, ll=("rle",), ml=("rle",), of=("fse", [31, 0, 0, 0, 0, 0, 1], 5), nbseq=form)
        return frame([raw(rbytes(18, 61)), blk], checksum=True)
    return build


for _n in (32768, 0x7F00 - 1, 0x7F00, 0x7F00 + 1):
    add(f"nbseq_{_n}", "nbseq-3byte", _nbseq(_n))
for _n in (127, 128, 255):
    add(f"nbseq_{_n}", "nbseq-2byte", _nbseq(_n))
add("nbseq_127_in_2_bytes", "nbseq-2byte", _nbseq(127, 2))
add("nbseq_5_in_2_bytes", "nbseq-2byte", _nbseq(5, 2))


# -------------------------------------------------------------------------------------------------------------- repcodes
def _rep_chain(seed, gaps, first_ll0_ov3=False, start_values=False):
    def build():
        r = random.Random(seed)
        blocks, out_len = [], 0
        rep = [1, 4, 8]
        if not start_values:
            blocks.append(raw(rbytes(seed, 50))); out_len = 50
        for b in range(4):
            seqs, pos = [], out_len
            for i in range(40):
                for _try in range(50):
                    if start_values and b == 0 and i < 3:
                        l, ov = (9, 3) if i == 0 else (1, 3) if i == 1 else (2, 3)      # 8, then 4, then 1: the start values
                    elif first_ll0_ov3 and b > 0 and i == 0:
                        l, ov = 0, 3
                    else:
                        l = r.choice([0, 0, 1, 3])
                        ov = r.choice([1, 2, 3, 1, 2, 3, 1, 2, 3, r.randrange(4, 60)])
                    if pos + l == 0:
                        continue
                    try:
                        off, nrep = F.rep_step(rep, l, ov)
                    except F.ForgeInvalid:
                        if first_ll0_ov3 and b > 0 and i == 0:
                            raise
                        continue
                    if off <= pos + l:
                        break
                else:
                    raise AssertionError("no valid sequence found")
                rep = nrep
                m = r.choice([3, 4, 5, 9])
                seqs.append((l, ov, m))
                pos += l + m
            lits = rbytes(seed * 10 + b, lits_needed(seqs, 1))
            blocks.append(cblock(rawlit(lits), seqs, ll=fse_mode("ll", seqs, 5), ml=fse_mode("ml", seqs, 5)))
            out_len = pos + 1
            if b < 3:
                for g in gaps:
                    if g == "raw":
                        blocks.append(raw(rbytes(b, 33))); out_len += 33
                    elif g == "rle":
                        blocks.append(rle(0x2E, 129)); out_len += 129
                    else:
                        blocks.append(cblock(rawlit(b"gap"))); out_len += 3
        return frame(blocks, checksum=True)
    return build


add("rep_chain", "repcodes", _rep_chain(1, ()))
add("rep_chain_2", "repcodes", _rep_chain(2, ()))
add("rep_chain_block_starts_ll0_ov3", "repcodes", _rep_chain(3, (), first_ll0_ov3=True))
add("rep_chain_over_raw", "repcodes", _rep_chain(4, ("raw",)))
add("rep_chain_over_rle", "repcodes", _rep_chain(5, ("rle",)))
add("rep_chain_over_noseq", "repcodes", _rep_chain(6, ("noseq",)))
add("rep_chain_over_all_gaps", "repcodes", _rep_chain(7, ("raw", "rle", "noseq"), first_ll0_ov3=True))
add("rep_chain_start_values", "repcodes", _rep_chain(8, (), start_values=True))


def _rep_of_rep():
    # repeat offset of repeat offset of repeat offset: each sequence picks the third, which the one before just pushed down
    seqs = [(4, 10 + 3, 3), (1, 20 + 3, 3), (1, 30 + 3, 3)] + [(1, 3, 4), (1, 3, 4), (1, 3, 4), (0, 2, 3), (0, 2, 3), (0, 2, 3),
                                                              (1, 2, 3), (0, 1, 3), (1, 2, 3), (0, 1, 3), (0, 3, 3), (0, 3, 3)]
    return frame([raw(rbytes(19, 40)), cblock(rawlit(rbytes(20, lits_needed(seqs))), seqs)])


add("rep_of_rep_of_rep", "repcodes", _rep_of_rep)
# offset 1 in the first repeat offset, then "repeat offset 1 minus one" with no literals: the format calls the result (0) invalid,
# decoders of the reference's line turn it into 1.  The forge holds it invalid; the verdicts are recorded.
add("rep1_minus_one_is_zero", "repcodes",
    lambda: frame([raw(b"abcdefgh"), cblock(rawlit(b"xy"), [(1, 1 + 3, 3), (0, 3, 5), (1, 1, 3)])], valid=False), valid=False)
add("rep1_minus_one_is_one", "repcodes",
    lambda: frame([raw(b"abcdefgh"), cblock(rawlit(b"xy"), [(1, 2 + 3, 3), (0, 3, 5), (1, 1, 3)])]))


# --------------------------------------------------------------------------------------------------------------- overlap
def _overlap(off):
    def build():
        blocks = [raw(rbytes(off, 64)),
                  cblock(rawlit(b"LMNOP"), [(2, off + 3, 3), (1, off + 3, 64), (1, off + 3, 65), (1, 1, 64), (0, off + 3, 129)]),
                  cblock(rawlit(b"Z"), [(1, off + 3, 70000)]),
                  cblock(rawlit(b""), [(0, off + 3, 3), (0, 1, 70000)])]
        return frame(blocks, checksum=True)
    return build


for _off in (1, 2, 3, 7, 8, 15, 16, 63, 64):
    add(f"overlap_off{_off}", "overlap", _overlap(_off))
add("overlap_from_previous_blocks_last_byte", "overlap",
    lambda: frame([raw(rbytes(21, 10)), cblock(rawlit(b"q"), [(0, 1 + 3, 70), (1, 2 + 3, 200)]), rle(9, 7),
                   cblock(rawlit(b""), [(0, 1 + 3, 64)])]))
add("overlap_back_to_first_byte", "overlap",
    lambda: frame([raw(rbytes(22, 100)), cblock(rawlit(b"12345"), [(0, 100 + 3, 3), (5, 108 + 3, 300), (0, 408 + 3, 1000)])]))
add("overlap_first_block_first_byte", "overlap",
    lambda: frame([cblock(rawlit(b"ab"), [(1, 1 + 3, 130), (1, 132 + 3, 66)])]))


# ---------------------------------------------------------------------------------------------------------- header forms
def _plain(n, **kw):
    def build():
        seqs = [(min(n, 10), 2 + 3, n - min(n, 10) - 1)] if n >= 20 else []
        return frame([cblock(rawlit(rbytes(n, min(n, 10) + 1 if seqs else n)), seqs)], **kw)
    return build


for _n, _fcs in ((255, 1), (255, 4), (256, 2), (65791, 2), (65792, 4), (300, 8), (255, 8), (65791, 4)):
    add(f"hdr_fcs{_fcs}_{_n}", "header-forms", _plain(_n, fcs=_fcs))
add("hdr_fcs4_declares_4g_minus_1", ["header-forms", "negatives"], _plain(100, fcs=4, fcs_value=(1 << 32) - 1, valid=False), valid=False)
add("hdr_window_mantissa1", "header-forms", _plain(1100, single=False, window=(0 << 3) | 1))          # 1 KiB + 1/8
add("hdr_window_mantissa7", "header-forms", _plain(1900, single=False, window=(0 << 3) | 7, checksum=True))
add("hdr_window_mantissa7_fcs2", "header-forms", _plain(1900, single=False, window=(1 << 3) | 7, fcs=2))
add("hdr_window_1k_full_blocks", "header-forms",
    lambda: frame([raw(rbytes(23, 1024)), rle(7, 1024), cblock(rawlit(rbytes(24, 24)), [(24, 900 + 3, 1000)]), raw(b"end")],
                  single=False, window=0))
add("hdr_window_64k_full_blocks", "header-forms",
    lambda: frame([rle(1, 65536), cblock(rlelit(2, 36), [(36, 65536 + 3, 65500)]), cblock(rawlit(b"abc"), [(3, 40000 + 3, 65533)])],
                  single=False, window=6 << 3, checksum=True))
for _did in (1, 2, 4):
    add(f"hdr_dictid_{_did}_bytes_zero", "header-forms", _plain(500, did=_did))
    add(f"hdr_dictid_{_did}_bytes_zero_window", "header-forms", _plain(500, did=_did, single=False, window=8, fcs=4))
add("hdr_empty", "header-forms", lambda: frame([raw(b"")]))
add("hdr_empty_checksum", "header-forms", lambda: frame([raw(b"")], checksum=True))
add("hdr_empty_window", "header-forms", lambda: frame([raw(b"")], single=False, window=0))
add("hdr_empty_last_block", "header-forms", lambda: frame([cblock(rawlit(b"some content"), [(4, 7, 9)]), raw(b"")]))
add("hdr_empty_last_block_checksum", "header-forms", lambda: frame([rle(3, 99), raw(b"")], checksum=True, single=False, window=0))
add("hdr_empty_blocks_inside", "header-forms", lambda: frame([raw(b""), raw(b"xyz"), raw(b""), cblock(rawlit(b"-")), raw(b"!")]))
# a compressed block of two bytes (no literals, no sequences): valid by the format's words; decoders of the reference's line ask
# for three bytes.  Recorded, expected to be contested.
add("hdr_compressed_block_of_2_bytes", "header-forms", lambda: frame([raw(b"xyz"), cblock(rawlit(b"")), raw(b"!")], single=False, window=0))


# ------------------------------------------------------------------------------------------------------------- skippable
def _two():
    a = frame([cblock(rawlit(b"first frame "), [(12, 6 + 3, 30)])], checksum=True)
    b = frame([rle(0x62, 40), raw(b" second")])
    return a, b


def _skip_all16():
    (fa, ca), (fb, cb) = _two()
    out = b""
    for i in range(16):
        out += F.skippable(i, b"")
        if i == 4:
            out += fa
        if i == 9:
            out += fb
    return out, ca + cb


def _skip_lengths(where):
    def build():
        (fa, ca), (fb, cb) = _two()
        s0, s1, s2 = F.skippable(0, b""), F.skippable(7, b"\xff"), F.skippable(15, rbytes(25, 70000))
        if where == "before":
            return s0 + s1 + fa + fb, ca + cb
        if where == "between":
            return fa + s1 + s0 + fb, ca + cb
        if where == "after":
            return fa + fb + s0 + s1, ca + cb
        if where == "long":
            return s1 + fa + s2 + fb + s0, ca + cb
        return s0 + s1 + s0, b""
    return build


add("skip_all16_len0", "skippable", _skip_all16)
for _w in ("before", "between", "after", "long", "only"):
    add(f"skip_{_w}", "skippable", _skip_lengths(_w))
add("skip_only_one_empty", "skippable", lambda: (F.skippable(3, b""), b""))


# ------------------------------------------------------------------------------------------------------------ long frames
def _long_frame(nblocks, tail):
    def build():
        r = random.Random(nblocks)
        w = skewed_weights(10, 60, 31)
        blocks, have = [], 0
        B = F.BLOCK_MAX
        tables = None
        for b in range(nblocks):
            kind = b % 4
            if b == 0:
                # 2 KiB of raw content, then RLE: the seed every later match draws on
                blocks += [raw(rbytes(26, 2048)), rle(0xAB, B - 2048)]
                # (two blocks that together fill one 128 KiB step)
            elif kind == 1 or kind == 3:
                # a compressed block of exactly 128 KiB: Huffman (or treeless) literals and matches that reach 1, 2 and 8 blocks back
                seqs, left = [], B
                nlit = 1500
                for i in range(24):
                    back = (1, 2, 8)[i % 3]
                    dist = min(have, back * B + r.randrange(1000)) - r.randrange(64)
                    l, m = 50, 3500 + r.randrange(1000)
                    seqs.append((l, max(dist, 1) + 3, m))
                    left -= l + m
                # short matches and repeat offsets, then one last match that fills the block
                for i in range(40):
                    l, m = r.randrange(0, 6), r.randrange(3, 40)
                    ov = r.choice([1, 2, 3, r.randrange(5, 3000)])
                    l = max(l, 1) if ov == 3 else l                            # (never "repeat offset 1 minus one": it could reach 0)
                    seqs.append((l, ov, m))
                    left -= l + m
                used = sum(s[0] for s in seqs)
                rest = nlit - used
                seqs.append((rest - 10, 2048 + 3, left - rest))
                data = draw_by_weight(b, w, nlit)
                first = tables is None
                lit = ({"k": "huf", "data": data, "w": w, "enc": "fse", "streams": 4} if first or kind == 1 and b % 8 == 1
                       else {"k": "treeless", "data": data, "streams": 4})
                if first:
                    # the tables name every code a later block may draw, so that repeat mode can code it
                    tables = dict(ll=fse_mode("ll", seqs + [(l, 9, 3) for l in F.LL_BASE[:32]], 7),
                                  of=fse_mode("of", seqs + [(1, 1, 3), (1, 2, 3)] + [(1, 1 << c, 3) for c in range(2, 22)], 7),
                                  ml=fse_mode("ml", seqs + [(1, 9, m) for m in F.ML_BASE], 8))
                    modes = tables
                else:
                    modes = dict(ll="repeat", of="repeat", ml="repeat") if kind == 3 else dict(ll="predef", of="repeat", ml="repeat")
                blocks.append(cblock(lit, seqs, **modes))
            elif kind == 2:
                blocks += [rle(b, B - 1000), raw(rbytes(b, 1000))]
            else:
                # sequences only: two long matches from the far past
                seqs = [(0, min(have, 8 * B) + 3, B // 2), (0, 3 * 1000 + 3, B // 2 - 1)]
                blocks.append(cblock(rawlit(b"!"), seqs, ll="repeat", of="repeat", ml="repeat"))
            have += B
        if tail:
            blocks.append(raw(rbytes(27, tail)))
        return frame(blocks, checksum=True)
    return build


add("long_frame_1m_plus_5", "long-frame", _long_frame(8, 5))
add("long_frame_3m", "long-frame", _long_frame(24, 0))


# -------------------------------------------------------------------------------------------------------------- negatives
def _neg(name, build):
    add("neg_" + name, "negatives", build, valid=False)


_base_seqs = [(5, 4 + 3, 10), (0, 1, 4), (3, 2, 5)]
_base_lit = rawlit(b"negative cases!!")


def _nframe(blocks, **kw):
    return frame(blocks, valid=False, **kw)


_neg("reserved_header_bit", lambda: _nframe([cblock(_base_lit, _base_seqs)], reserved=True))
_neg("block_type_3", lambda: _nframe([raw(b"abc"), {"t": "reserved"}]))
_neg("ll_accuracy_log_10", lambda: _nframe([cblock(_base_lit, _base_seqs, ll=("fse", F.normalize([1] * 16, 9), 9, 10))]))
_neg("of_accuracy_log_9", lambda: _nframe([cblock(_base_lit, _base_seqs, of=("fse", F.normalize([1] * 8, 8), 8, 9))]))
_neg("ml_accuracy_log_10", lambda: _nframe([cblock(_base_lit, _base_seqs, ml=("fse", F.normalize([1] * 16, 9), 9, 10))]))
# a count can never exceed what remains of the table (the field's width shrinks with it), so "overshoot" is: more symbols than
# the alphabet has
_neg("of_ncount_33_symbols", lambda: _nframe([cblock(_base_lit, _base_seqs, of=("fse", [1] * 32 + [32], 6))]))
_neg("ll_ncount_37_symbols", lambda: _nframe([cblock(_base_lit, _base_seqs, ll=("fse", [1] * 36 + [28], 6))]))
_neg("huf_weights_not_a_power_of_two",
     lambda: _nframe([cblock({"k": "huf", "data": b"\x00\x01\x02" * 30, "w": [2, 1, 1], "stored": [2, 1, 1, 1], "streams": 1})]))
# with the last weight implied, the weights always sum to a power of two, so an odd number of weight-1 symbols cannot be
# written; what can is a tree with NO weight-1 symbol (one stored weight 2, the implied one 2 as well)
_neg("huf_no_weight_1_symbol",
     lambda: _nframe([cblock({"k": "huf", "data": b"\x00\x01" * 30, "w": [1, 1], "stored": [2], "streams": 1})]))
_neg("huf_weight_13",
     lambda: _nframe([cblock({"k": "huf", "data": b"\x00\x01\x02" * 30, "w": [2, 1, 1], "stored": [13, 1], "streams": 1})]))
_neg("rle_ll_code_36", lambda: _nframe([cblock(_base_lit, [(5, 7, 10)], ll=("rle", 36))]))
_neg("rle_of_code_32", lambda: _nframe([cblock(_base_lit, [(5, 7, 10)], of=("rle", 32))]))
_neg("rle_ml_code_53", lambda: _nframe([cblock(_base_lit, [(5, 7, 10)], ml=("rle", 53))]))
_neg("repeat_in_first_block", lambda: _nframe([raw(b"front"), cblock(_base_lit, _base_seqs, ll="repeat")]))
_neg("repeat_of_in_first_block", lambda: _nframe([cblock(_base_lit, _base_seqs, of="repeat")]))
_neg("treeless_in_first_block",
     lambda: _nframe([raw(b"front"), cblock({"k": "treeless", "data": b"\x00\x01\x02" * 30, "w": [2, 1, 1], "streams": 1})]))
_neg("bitstream_last_byte_0", lambda: _nframe([cblock(_base_lit, _base_seqs, append_zero=True)]))
# decoders of the reference's line update the three states once more after the last sequence, which swallows up to 9 + 9 + 8
# left-over bits: 9 bits are expected to be contested, 40 cannot be swallowed
_neg("bitstream_9_unconsumed_bits", lambda: _nframe([cblock(_base_lit, _base_seqs, junk_bits=9)]))
_neg("bitstream_40_unconsumed_bits", lambda: _nframe([cblock(_base_lit, _base_seqs, junk_bits=40)]))
_neg("sequences_take_too_many_literals", lambda: _nframe([cblock(rawlit(b"1234567"), _base_seqs)]))
_neg("offset_one_past_the_start", lambda: _nframe([raw(b"12345"), cblock(_base_lit, [(5, 11 + 3, 10)])]))
_neg("offset_one_past_the_start_repcode", lambda: _nframe([cblock(_base_lit, [(3, 3, 4)])]))
# The size limits of a block, in frames that state their content size ...
_neg("block_regenerates_128k_plus_2", lambda: _nframe([cblock(rlelit(0x61, 131071), [(131071, 4, 3)])], single=True, fcs_value=131074))
_neg("block_above_window", lambda: _nframe([raw(rbytes(28, 1025))], single=False, window=0, fcs=4))
_neg("rle_block_above_window", lambda: _nframe([rle(5, 1025)], single=False, window=0, fcs=4))
_neg("compressed_block_above_window", lambda: _nframe([cblock(rawlit(rbytes(29, 1030)))], single=False, window=0, fcs=4))
_neg("compressed_block_regenerates_above_window",
     lambda: _nframe([raw(b"ab"), cblock(rawlit(b"c"), [(1, 5, 1024)])], single=False, window=0, fcs=4))
# ... and in frames that do not: such a frame regenerates more than its own bound (blocks x block size limit, what
# ZSTD_decompressBound answers for it).  The reference's line decodes it into a destination that is larger than that.
_neg("unsized_block_above_window", lambda: _nframe([raw(rbytes(28, 1025))], single=False, window=0))
_neg("unsized_rle_block_above_window", lambda: _nframe([rle(5, 1025)], single=False, window=0))
_neg("unsized_compressed_block_regenerates_above_window",
     lambda: _nframe([cblock(rawlit(b"abc"), [(3, 1 + 3, 1024)])], single=False, window=0))
_neg("unsized_block_regenerates_128k_plus_2",
     lambda: _nframe([cblock(rlelit(0x61, 131071), [(131071, 4, 3)])], single=False, window=7 << 3))
_neg("compressed_block_above_single_segment_content", lambda: _nframe([cblock(rawlit(rbytes(30, 31)), [(31, 4, 3)])], single=True))
_neg("content_size_one_less", lambda: _nframe([cblock(_base_lit, _base_seqs)], fcs_value=34))
_neg("content_size_one_more", lambda: _nframe([cblock(_base_lit, _base_seqs)], fcs_value=36))
_neg("wrong_checksum", lambda: _nframe([cblock(_base_lit, _base_seqs)], checksum=True, bad_checksum=True))


# ---------------------------------------------------------------------------------------------------------- random frames
def random_frame(seed):
    """one frame of 1 to 4 blocks and at most 8 KiB of content: modes, table logs, weights and repcode-heavy sequences at random"""
    r = random.Random(seed)
    blocks, have = [], 0
    wide = {}                    # kind -> the frame's current table can code whatever gen_seqs draws (so a block may repeat it)
    huf_w = None
    for b in range(r.randrange(1, 5)):
        t = r.random()
        if t < 0.15:
            n = r.randrange(0, 300)
            blocks.append(raw(rbytes(seed + b, n))); have += n
            continue
        if t < 0.3:
            n = r.randrange(1, 600)
            blocks.append(rle(r.randrange(256), n)); have += n
            continue
        nseq = r.choice([0, 1, 2, 5, 20, 60, 64, 65, 130])
        fixed, modes = {}, {}
        for kind, key, val in (("ll", "ll", r.randrange(0, 18)), ("of", "ofcode", r.randrange(2, 6)), ("ml", "ml", r.randrange(3, 40))):
            m = r.choice(["predef", "rle", "fse", "fse", "repeat", "repeat"])
            if m == "repeat" and not wide.get(kind):
                m = "fse"
            if m == "rle":
                fixed[key] = val
            modes[kind] = m
        if have == 0 and fixed.get("ll") == 0:
            fixed["ll"] = 1
        if "ofcode" in fixed and have + fixed.get("ll", 1) < (2 << fixed["ofcode"]):
            del fixed["ofcode"]
            modes["of"] = "predef"
        seqs = gen_seqs(r, nseq, have, repshare=0.6, **fixed) if nseq else []
        kw = {}
        for i, kind in enumerate(("ll", "of", "ml") if nseq else ()):
            m = modes[kind]
            if m == "fse" and len(set(F.seq_codes(s)[i][0] for s in seqs)) < 2:
                m = "rle"
            if m == "fse":
                log = r.randrange(5, F.MAX_LOG[kind] + 1)
                pad = PADS[kind] if log >= 7 and r.random() < 0.6 else []
                kw[kind] = fse_mode(kind, seqs + pad, log)
                wide[kind] = bool(pad)
            elif m == "rle":
                kw[kind] = ("rle",)
                wide[kind] = False
            else:
                kw[kind] = m
                wide[kind] = True
        nlit = lits_needed(seqs, r.randrange(0, 20))
        if not seqs:
            nlit = max(nlit, 1)          # (a compressed block of 2 bytes is refused by decoders of the reference's line: its own case)
        lk = r.random()
        if nlit >= 20 and lk < 0.5:
            streams = r.choice([1, 4]) if nlit < 1024 else 4
            if huf_w is not None and lk < 0.2:
                lit = {"k": "treeless", "data": draw_by_weight(seed + b, huf_w, nlit), "streams": streams}
            else:
                huf_w = skewed_weights(r.randrange(2, 13), r.randrange(14, 60), seed + b)
                lit = {"k": "huf", "data": draw_by_weight(seed + b, huf_w, nlit), "w": huf_w, "enc": r.choice(["direct", "fse"]),
                       "streams": streams}
                if len(set(huf_w[:-1])) < 2:
                    lit["enc"] = "direct"                    # (FSE cannot describe a single value)
        elif lk < 0.75 or nlit == 0:
            lit = rawlit(rbytes(seed + b, nlit))
        else:
            lit = rlelit(r.randrange(256), nlit)
        blocks.append(cblock(lit, seqs, **kw))
        have += nlit + sum(s[2] for s in seqs)
        if have > 6000:
            break
    windowed = r.random() < 0.4
    return frame(blocks, single=False if windowed else None, window=r.randrange(4, 9) << 3 | r.randrange(8) if windowed else None,
                 checksum=r.random() < 0.5)


# ------------------------------------------------------------------------------------------- the committed fixtures
def capacity(size):
    """room to decode a case into: its content, or — for a case the forge holds invalid — more than any decoder makes of one"""
    return size if size is not None else 300000


def all_sized(blob):
    """every zstd frame of the blob states its content size (skippable frames state nothing and count for nothing)"""
    at = 0
    while at < len(blob):
        magic = int.from_bytes(blob[at:at + 4], "little")
        if magic & 0xFFFFFFF0 == F.SKIP_MAGIC:
            at += 8 + int.from_bytes(blob[at + 4:at + 8], "little")
            continue
        assert magic == F.MAGIC
        fhd = blob[at + 4]
        single, fcs = (fhd >> 5) & 1, fhd >> 6
        if not single and not fcs:
            return False
        at += 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + (single, 2, 4, 8)[fcs]
        last = 0
        while not last:
            h = int.from_bytes(blob[at:at + 3], "little")
            last = h & 1
            at += 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)
        at += 4 if fhd & 4 else 0
    return True


def load_manifest():
    """the cases of tests/golden/manifest_forge.json, each with its blob and what a decoder has to do with it:
    c["expect"] = ("bytes", size, sha256) or ("reject",)  —  an agreed case: the executor's content, or a refusal; a contested
    one: what the oracle did (DESIGN.md "Parity")"""
    import json
    import os
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    man = json.load(open(os.path.join(d, "manifest_forge.json")))
    for c in man["cases"]:
        c["blob"] = open(os.path.join(d, c["file"]), "rb").read()
        c["cap"] = capacity(c["size"])
        if c["agreed"]:
            c["expect"] = ("bytes", c["size"], c["sha256"]) if c["valid"] else ("reject",)
        elif c["oracle"] == "equal":
            c["expect"] = ("bytes", c["size"], c["sha256"])
        elif c["oracle"].startswith("different"):
            _, n, sha = c["oracle"].split(":")
            c["expect"] = ("bytes", int(n), sha)
            c["cap"] = max(c["cap"], int(n))
        else:
            c["expect"] = ("reject",)
    return man
