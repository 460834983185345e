"""A zstd frame WRITER in plain Python, written from the format specification (RFC 8878).  Test infrastructure only.

It does not compress: the caller describes a frame field by field (header form, block types and sizes, literals section form,
Huffman weights, sequence triples, the mode and distribution of each FSE table, the nbSeq form) and gets back
(frame_bytes, content_bytes).  content_bytes comes from `execute`, a plain LZ executor that follows the format's words on
repeat offsets; it shares no code with the oracle decoder or the GPU decoder and is the reference the forged-frame tests
compare against.  Fields that make a frame INVALID can be asked for too (negatives); then content_bytes is None.

Description (plain dicts / tuples, see tests/forge_cases.py for many examples):

  frame(blocks, single=None, fcs=None, fcs_value=None, window=None, did=0, checksum=False, reserved=False,
        bad_checksum=False, valid=True, history=b"", did_value=0)
      single   single-segment (the content size is the window); None = where no block is larger than the content, else a
               window descriptor that holds the content (also where an invalid description has no content size to state)
      fcs      content-size field in bytes: 0, 1, 2, 4, 8 or None = the smallest that holds the size (none under a window)
      window   the window descriptor byte (exponent << 3 | mantissa); needs single=False
      did      size of a dictionary-ID field (0, 1, 2, 4); it holds did_value (default 0)
      history  bytes in front of the frame that offsets may reach (a dictionary's content, a prefix); not part of the content

  block:   {"t": "raw", "data": b"..."}          {"t": "rle", "byte": 65, "size": 1000}        {"t": "reserved"}
           {"t": "c", "lit": LIT, "seqs": [(litLength, offset_value, matchLength), ...],
            "ll": MODE, "of": MODE, "ml": MODE, "nbseq": 1|2|3 (bytes of the count; default smallest),
            "junk_bits": n, "append_zero": bool}
           every block takes "last": bool (default: only the final one)
  LIT:     {"k": "raw"|"rle", "data": b"...", "sf": 0|1|3}
           {"k": "huf", "data": b"...", "w": weights (one per symbol 0..last, the last one included),
            "enc": "direct"|"fse", "streams": 1|4, "sf": 0..3, "stored": weights to store instead (negatives)}
           {"k": "treeless", "data": b"...", "streams": 1|4, "sf": 0..3, "w": weights to code with when no block defined any}
  MODE:    "predef" | "repeat" | ("rle",) | ("rle", code) | ("fse", norm, log) | ("fse", norm, log, declared_log)
           offset_value is the format's: 1..3 are repeat offsets, offset + 3 otherwise.
"""
import struct

MAGIC = 0xFD2FB528
SKIP_MAGIC = 0x184D2A50
BLOCK_MAX = 1 << 17

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = ([4, 3] + [2] * 11 + [1, 1, 1] + [2] * 9 + [3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_DEFAULT = ([1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7, 6)
OF_DEFAULT = ([1] * 6 + [2, 2, 2] + [1] * 15 + [-1] * 5, 5)
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}
DEFAULTS = {"ll": LL_DEFAULT, "of": OF_DEFAULT, "ml": ML_DEFAULT}


class ForgeInvalid(Exception):
    """the description does not regenerate content (a negative case)"""


# ------------------------------------------------------------------------------------------------------------ XXH64
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
_M = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, v):
    return (_rotl((acc + v * _P2) & _M, 31) * _P1) & _M


def _merge(h, v):
    return ((h ^ _round(0, v)) * _P1 + _P4) & _M


def xxh64(data, seed=0):
    n, p = len(data), 0
    if n >= 32:
        v1, v2, v3, v4 = (seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M
        for a, b, c, d in struct.iter_unpack("<QQQQ", memoryview(data)[:n - n % 32]):
            v1, v2, v3, v4 = _round(v1, a), _round(v2, b), _round(v3, c), _round(v4, d)
        p = n - n % 32
        h = (_rotl(v1, 1) + _rotl(v2, 7) + _rotl(v3, 12) + _rotl(v4, 18)) & _M
        for v in (v1, v2, v3, v4):
            h = _merge(h, v)
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[p:p + 8], "little")), 27) * _P1 + _P4) & _M
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * _P1) & _M, 23) * _P2 + _P3) & _M
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5) & _M, 11) * _P1) & _M
        p += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    h ^= h >> 32
    return h


# ------------------------------------------------------------------------------------------------------- bit writers
class Bits:
    """bits appended from bit 0 upward; as a backward stream the reader starts below the final 1 bit and reads downward, so
    what is added LAST is read FIRST, and a value added in one call is read back whole"""

    def __init__(self):
        self.chunks, self.acc, self.n, self.total = [], 0, 0, 0

    def add(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0, (value, nbits)
        self.acc |= value << self.n
        self.n += nbits
        self.total += nbits
        if self.n >= 4096:
            k = self.n // 8
            self.chunks.append((self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little"))
            self.acc >>= 8 * k
            self.n -= 8 * k

    def forward(self):
        return b"".join(self.chunks) + self.acc.to_bytes((self.n + 7) // 8, "little")

    def backward(self):
        self.add(1, 1)
        return self.forward()


def highbit(v):
    return v.bit_length() - 1


# --------------------------------------------------------------------------------------------------------------- FSE
def fse_table(norm, log):
    """the decoding table of RFC 8878 4.1.1: per state (symbol, nbBits, baseline)"""
    size = 1 << log
    assert sum(abs(c) for c in norm) == size, ("distribution does not fill the table", sum(abs(c) for c in norm), size)
    sym = [None] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nxt = [max(abs(c), 0) for c in norm]
    table = []
    for st in range(size):
        s = sym[st]
        x = nxt[s]
        nxt[s] += 1
        nb = log - highbit(x)
        table.append((s, nb, (x << nb) - size))
    return table


class FseCoder:
    """chooses, walking the symbols backward, the state that decodes to each symbol and whose bit range holds the state after it"""

    def __init__(self, norm, log):
        self.log = log
        self.by_sym = {}
        for st, (s, nb, base) in enumerate(fse_table(norm, log)):
            self.by_sym.setdefault(s, []).append((base, nb, st))

    def last_state(self, s):
        # any state of the symbol will do; take the one with the most bits (the weight coder needs nbBits > 0 at the end)
        return max(self.by_sym[s], key=lambda e: (e[1], -e[2]))[2]

    def step(self, s, next_state):
        """-> (state, bits value, nbBits) so that the decoder in `state` reads `value` and lands on next_state"""
        for base, nb, st in self.by_sym[s]:
            if base <= next_state < base + (1 << nb):
                return st, next_state - base, nb
        raise AssertionError("no state of symbol %d reaches %d" % (s, next_state))


class RleCoder:
    log = 0

    def __init__(self, s):
        self.s = s

    def last_state(self, s):
        assert s == self.s, ("RLE table of code", self.s, "cannot code", s)
        return 0

    def step(self, s, next_state):
        assert s == self.s, ("RLE table of code", self.s, "cannot code", s)
        return 0, 0, 0


def write_ncount(norm, log, declared_log=None):
    """the table description of RFC 8878 4.1.1, byte aligned"""
    norm = list(norm)
    while norm and norm[-1] == 0:
        norm.pop()
    b = Bits()
    b.add((log if declared_log is None else declared_log) - 5, 4)
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    i, prev0 = 0, False
    while remaining > 1:
        if prev0:
            start = i
            while norm[i] == 0:
                i += 1
            run = i - start
            while run >= 3:
                b.add(3, 2)
                run -= 3
            b.add(run, 2)
        c = norm[i]
        i += 1
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        v = c + 1
        if v >= threshold:
            v += mx
        b.add(v, nbits - (1 if v < mx else 0))
        prev0 = (c == 0)
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    assert remaining == 1 and i == len(norm), (remaining, i, len(norm))
    return b.forward()


def normalize(counts, log):
    """a valid distribution of total 1 << log with every counted symbol present (a helper for callers; nothing clever)"""
    total, size = sum(counts), 1 << log
    norm = [max(1, c * size // total) if c else 0 for c in counts]
    big = max(range(len(counts)), key=lambda i: norm[i])
    norm[big] += size - sum(norm)
    assert norm[big] >= 1, "too many symbols for this table size"
    return norm


# ----------------------------------------------------------------------------------------------------------- Huffman
def huf_table_log(weights):
    total = sum((1 << w) >> 1 for w in weights)
    assert total and total & (total - 1) == 0, ("weights do not complete a power of two", total)
    return highbit(total)


def huf_codes(weights):
    """{symbol: (code, nbBits)}: the canonical assignment of RFC 8878 4.2.1.3: ascending weight, then ascending symbol, from code 0"""
    log = huf_table_log(weights)
    codes, start = {}, 0
    for w in range(1, log + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (start >> (w - 1), log + 1 - w)
                start += 1 << (w - 1)
    assert start == 1 << log
    return codes


def huf_stream(data, codes):
    b = Bits()
    for s in reversed(data):
        b.add(*codes[s])
    return b.backward()


def huf_weights_header(stored, enc):
    n = len(stored)
    if enc == "direct":
        assert 1 <= n <= 128
        st = list(stored) + [0]
        return bytes([127 + n]) + bytes((st[i] << 4) | st[i + 1] for i in range(0, n, 2))
    # FSE-compressed, two interleaved states (RFC 8878 4.2.1.2), table log at most 6
    counts = [0] * 13
    for w in stored:
        counts[w] += 1
    while counts[-1] == 0:
        counts.pop()
    assert sum(1 for c in counts if c) >= 2, "FSE-compressed weights need two different values"
    log = 6 if n >= 64 else 5
    norm = normalize(counts, log)
    coder = FseCoder(norm, log)
    b = Bits()
    # the last two weights only pick the final states; every earlier weight costs one transition of its own state
    state = {(n - 1) % 2: coder.last_state(stored[n - 1]), (n - 2) % 2: coder.last_state(stored[n - 2])}
    for i in range(n - 3, -1, -1):
        st, v, nb = coder.step(stored[i], state[i % 2])
        b.add(v, nb)
        state[i % 2] = st
    b.add(state[1], log)
    b.add(state[0], log)
    body = write_ncount(norm, log) + b.backward()
    assert len(body) < 128
    return bytes([len(body)]) + body


def lit_section(lit, fs):
    """-> (section bytes, literal bytes)"""
    k, data = lit["k"], bytes(lit["data"])
    n = len(data)
    if k in ("raw", "rle"):
        sf = lit.get("sf")
        if sf is None:
            sf = 0 if n < 32 else 1 if n < 4096 else 3
        t = 0 if k == "raw" else 1
        if k == "rle":
            assert n >= 1 and data == data[:1] * n
        body = data if k == "raw" else data[:1]
        if sf == 0:
            assert n < 32
            return bytes([t | (n << 3)]) + body, data
        if sf == 1:
            assert n < 4096
            return (t | (1 << 2) | (n << 4)).to_bytes(2, "little") + body, data
        assert n < (1 << 20)
        return (t | (3 << 2) | (n << 4)).to_bytes(3, "little") + body, data
    streams = lit.get("streams", 4)
    tree = b""
    if k == "huf":
        w = list(lit["w"])
        codes = huf_codes(w)
        tree = huf_weights_header(lit.get("stored", w[:-1]), lit.get("enc", "direct"))
        fs.huf = codes
    else:
        assert k == "treeless"
        codes = fs.huf if fs.huf is not None else huf_codes(lit["w"])
    if streams == 1:
        payload = huf_stream(data, codes)
    else:
        seg = (n + 3) // 4
        parts = [huf_stream(data[i * seg:(i + 1) * seg], codes) for i in range(4)]
        assert all(len(p) < 65536 for p in parts[:3])
        payload = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
    csize = len(tree) + len(payload)
    sf = lit.get("sf")
    if sf is None:
        sf = 0 if streams == 1 else 1 if max(n, csize) < 1024 else 2 if max(n, csize) < 16384 else 3
    assert (sf == 0) == (streams == 1), "size format 0 is the single-stream form"
    bits = {0: 10, 1: 10, 2: 14, 3: 18}[sf]
    assert n < (1 << bits) and csize < (1 << bits), (n, csize, sf)
    t = 2 if k == "huf" else 3
    head = (t | (sf << 2) | (n << 4) | (csize << (4 + bits))).to_bytes({0: 3, 1: 3, 2: 4, 3: 5}[sf], "little")
    return head + tree + payload, data


# --------------------------------------------------------------------------------------------------------- sequences
def ll_code(v):
    return max(c for c in range(36) if LL_BASE[c] <= v)


def ml_code(v):
    return max(c for c in range(53) if ML_BASE[c] <= v)


def seq_codes(seq):
    ll, ov, ml = seq
    lc, mc, oc = ll_code(ll), ml_code(ml), highbit(ov)
    return (lc, ll - LL_BASE[lc], LL_BITS[lc]), (oc, ov - (1 << oc), oc), (mc, ml - ML_BASE[mc], ML_BITS[mc])


def _coder(kind, mode, codes, fs):
    """-> (table description bytes, mode number, coder)"""
    if mode == "predef":
        fs.tables[kind] = FseCoder(*DEFAULTS[kind])
        return b"", 0, fs.tables[kind]
    if mode == "repeat":
        if fs.tables.get(kind) is None:                  # negative: nothing to repeat; code as if predefined
            return b"", 3, FseCoder(*DEFAULTS[kind])
        return b"", 3, fs.tables[kind]
    if mode[0] == "rle":
        code = mode[1] if len(mode) > 1 else codes[0]
        fs.tables[kind] = RleCoder(codes[0] if code > MAX_SYM[kind] else code)
        return bytes([code]), 1, fs.tables[kind]
    assert mode[0] == "fse"
    norm, log = mode[1], mode[2]
    fs.tables[kind] = FseCoder(norm, log)
    return write_ncount(norm, log, mode[3] if len(mode) > 3 else None), 2, fs.tables[kind]


def seq_section(blk, fs):
    seqs = blk.get("seqs", [])
    n = len(seqs)
    form = blk.get("nbseq") or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert n < 128
        head = bytes([n])
    elif form == 2:
        assert n < 0x7F00
        head = bytes([0x80 + (n >> 8), n & 255])
    else:
        assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
        head = b"\xff" + (n - 0x7F00).to_bytes(2, "little")
    if n == 0:
        return head
    coded = [seq_codes(s) for s in seqs]
    desc, modes, coders = b"", [], []
    for i, kind in enumerate(("ll", "of", "ml")):
        d, m, c = _coder(kind, blk.get(kind, "predef"), [cs[i][0] for cs in coded], fs)
        desc += d
        modes.append(m)
        coders.append(c)
    cl, co, cm = coders
    b = Bits()
    b.add(0, blk.get("junk_bits", 0))                    # negative: bits the decoder never consumes
    (lc, lx, lb), (oc, ox, ob), (mc, mx, mb) = coded[-1]
    sl, so, sm = cl.last_state(lc), co.last_state(oc), cm.last_state(mc)
    b.add(lx, lb); b.add(mx, mb); b.add(ox, ob)
    for (lc, lx, lb), (oc, ox, ob), (mc, mx, mb) in reversed(coded[:-1]):
        # the decoder reads: offset, match length and literal length extra bits, then the LL, ML and OF state updates
        so, v, nb = co.step(oc, so); b.add(v, nb)
        sm, v, nb = cm.step(mc, sm); b.add(v, nb)
        sl, v, nb = cl.step(lc, sl); b.add(v, nb)
        b.add(lx, lb); b.add(mx, mb); b.add(ox, ob)
    b.add(sm, cm.log); b.add(so, co.log); b.add(sl, cl.log)
    stream = b.backward()
    if blk.get("append_zero"):                           # negative: the last byte carries no end mark
        stream += b"\x00"
    return head + bytes([(modes[0] << 6) | (modes[1] << 4) | (modes[2] << 2)]) + desc + stream


# ---------------------------------------------------------------------------------------------------------- executor
def rep_step(rep, ll, ov):
    """(offset, repeat offsets afterwards) of one sequence, RFC 8878 3.1.1.5"""
    if ov > 3:
        return ov - 3, [ov - 3, rep[0], rep[1]]
    idx = ov - 1 + (1 if ll == 0 else 0)                 # with no literals in front, the repeat offsets shift by one
    if idx == 0:
        return rep[0], rep
    off = rep[0] - 1 if idx == 3 else rep[idx]
    if off == 0:
        raise ForgeInvalid("repeat offset 1 minus one is zero")
    return off, ([off, rep[0], rep[1]] if idx >= 2 else [off, rep[0], rep[2]])


def execute(blocks, sizes=None, history=b""):
    """the content a frame of these blocks regenerates (RFC 8878 3.1.1.4 and 3.1.1.5), or ForgeInvalid; `sizes`, a list, takes
    the size each block regenerates; `history` lies in front of the frame: offsets may reach into it, the content does not hold it"""
    out = bytearray(history)
    rep = [1, 4, 8]
    for blk in blocks:
        t = blk["t"]
        start = len(out)
        if t == "raw":
            out += blk["data"]
        elif t == "rle":
            out += bytes([blk["byte"]]) * blk["size"]
        elif t == "c":
            lits, lp = bytes(blk["lit"]["data"]), 0
            for ll, ov, ml in blk.get("seqs", []):
                if lp + ll > len(lits):
                    raise ForgeInvalid("sequences take more literals than the section has")
                out += lits[lp:lp + ll]
                lp += ll
                off, rep = rep_step(rep, ll, ov)
                if off > len(out):
                    raise ForgeInvalid("offset reaches before the frame and its history")
                if off >= ml:
                    out += out[len(out) - off:len(out) - off + ml]
                else:
                    pat = bytes(out[len(out) - off:])
                    out += (pat * (ml // off + 1))[:ml]
            out += lits[lp:]
            if len(out) - start > BLOCK_MAX:
                raise ForgeInvalid("a block regenerates more than 128 KiB")
        else:
            raise ForgeInvalid("reserved block type")
        if sizes is not None:
            sizes.append(len(out) - start)
    return bytes(out[len(history):])


# ------------------------------------------------------------------------------------------------------------- frame
class _FrameState:
    def __init__(self):
        self.huf = None
        self.tables = {}


def block_bytes(blk, last, fs):
    t = blk["t"]
    last = blk.get("last", last)
    if t == "raw":
        return (last | (len(blk["data"]) << 3)).to_bytes(3, "little") + bytes(blk["data"])
    if t == "rle":
        return (last | 2 | (blk["size"] << 3)).to_bytes(3, "little") + bytes([blk["byte"]])
    if t == "reserved":
        return (last | 6 | (1 << 3)).to_bytes(3, "little") + b"\x00"
    body = lit_section(blk["lit"], fs)[0] + seq_section(blk, fs)
    assert len(body) < (1 << 21)
    return (last | 4 | (len(body) << 3)).to_bytes(3, "little") + body


def frame(blocks, single=None, fcs=None, fcs_value=None, window=None, did=0, checksum=False, reserved=False,
          bad_checksum=False, valid=True, history=b"", did_value=0):
    regen = []
    try:
        content = execute(blocks, regen, history)
    except ForgeInvalid:
        assert not valid, "the description is invalid but was declared valid"
        content = None
    fs = _FrameState()
    body = [block_bytes(blk, 1 if i == len(blocks) - 1 else 0, fs) for i, blk in enumerate(blocks)]
    n = len(content) if content is not None else 0
    size = n if fcs_value is None else fcs_value
    # the largest block, as Block_Maximum_Size = min(window, 128 KiB) bounds it: what a block regenerates, and a block's own size
    largest = max([0] + regen + [len(b) - 3 for b, blk in zip(body, blocks) if blk["t"] != "rle"])
    if single is None:
        # single-segment makes the content size the window: only where no block is larger than that
        single = window is None and (largest <= size or not valid) and (content is not None or fcs_value is not None)
        if not single and window is None:
            window = max(0, (max(largest, n, 1) - 1).bit_length() - 10) << 3
    if not single:
        assert window is not None
    wsize = size if single else ((8 + (window & 7)) << (7 + (window >> 3)))
    if valid:
        assert largest <= min(wsize, BLOCK_MAX), ("a block is larger than the frame's Block_Maximum_Size", largest, wsize)
    if fcs is None:
        fcs = 0 if not single else 1 if size < 256 else 2 if size < 65536 + 256 else 4 if size < (1 << 32) else 8
    assert (fcs == 1) <= single and (fcs == 0) <= (not single), "1-byte content size needs single-segment, none needs a window"
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs]
    out = MAGIC.to_bytes(4, "little")
    out += bytes([(flag << 6) | (single << 5) | (reserved << 3) | (checksum << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[did]])
    if not single:
        out += bytes([window])
    out += did_value.to_bytes(did, "little")
    if fcs:
        out += (size - 256 if fcs == 2 else size).to_bytes(fcs, "little")
    out += b"".join(body)
    if checksum:
        h = xxh64(content if content is not None else b"") & 0xFFFFFFFF
        out += (h ^ (1 if bad_checksum else 0)).to_bytes(4, "little")
    return out, (content if valid else None)


def skippable(nibble, payload):
    return (SKIP_MAGIC + nibble).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + bytes(payload)
