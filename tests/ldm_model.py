"""The long-distance stage (zstdsharp_amd/csrc/ldm.hip) as a serial model in plain Python; numpy only for the two hashes
and for comparing byte runs.  No GPU, no oracle.

It is written from the reference's formulation (ZSTD_ldm_generateSequences_internal, U/ZstdLdm.cs) wherever that differs from the
kernels': one serial gear hash per frame that starts from 0 at the frame's first byte, a round-robin bucket table filled in position
order (no sort), a greedy walk with an anchor per block.  tests/test_gpu_ldm_model.py compares the kernels with it for equality.

  Params(minMatch, hashLog, bucketLog, hashRateLog)     what the call resolves (ldm_resolve)
  Layout(n, base, vlo, span, chunk, maxDist)            the stage's coordinate: the pass's byte i lies at base + i, what lies in front
                                                        of it (a referenced prefix, a sliding window's content) at [vlo, base), the
                                                        end at n; span = bytes per frame (0: one frame from vlo), chunk = per block
  splits(buf, lay, p, loop=False) -> (pos, check, key), labels         buf: bytes indexed by position ([0, vlo) is never read)
  matches(buf, lay, p, S)         -> [(mStart, mLen, mOff)] per split, labels
  merge(F, L, blockLen)           -> [(start, len, distance)], literal bytes, labels
  stage(buf, lay, p)              -> splits, matches, labels of both

labels: a dict, label -> how often the branch ran.  `rules` switches single rules to a wrong form, for the tests that prove that a
case notices (tests/test_ldm_model_cpu.py); the default is the stage's rule.
"""
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "minMatch hashLog bucketLog hashRateLog")
Layout = namedtuple("Layout", "n base vlo span chunk maxDist")
M64 = (1 << 64) - 1
TILE, SEG, CAP = 16384, 64, 4

RULES = dict(cap=CAP, strict=True, nearest_first=True, anchor_fwd=True, floor=4, tie_le=True, frame_restart=True, window_in_frame=True,
             min_on_fwd=True, insert_unsearched=True, check_filter=True)


def _rules(r):
    out = dict(RULES)
    out.update(r or {})
    return out


def splitmix64(i):
    z = ((i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


GEAR = [splitmix64(i) for i in range(256)]
_GEAR_NP = np.array(GEAR, dtype=np.uint64)


def stop_mask(p):
    m = min(p.minMatch, 64)
    if 0 < p.hashRateLog <= m:
        return ((1 << p.hashRateLog) - 1) << (m - p.hashRateLog)
    return (1 << p.hashRateLog) - 1


def window_hash(window):
    """FNV-1a + fmix64 over the window's first min(minMatch, 64) bytes, one byte at a time"""
    x = 0xCBF29CE484222325 ^ len(window)
    for b in window:
        x = ((x ^ b) * 0x100000001B3) & M64
    x ^= x >> 33; x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33; x = (x * 0xC4CEB9FE1A85EC53) & M64
    return x ^ (x >> 33)


def frames_of(lay):
    """[(start, end)] of the frames the stage sees: one from vlo with something in front of the pass, else spans from 0"""
    if lay.base or not lay.span:
        return [(lay.vlo, lay.n)]
    return [(a, min(a + lay.span, lay.n)) for a in range(0, lay.n, lay.span)]


def _stops_loop(buf, a, b, mask):
    """positions p in [a, b) where the serial gear hash from h = 0 at a has no bit of the mask set"""
    out, h, gear = [], 0, GEAR
    for q in range(a, b):
        h = ((h << 1) + gear[buf[q]]) & M64
        if not h & mask:
            out.append(q)
    return out


def _stops_np(buf, a, b, mask):
    g = _GEAR_NP[np.frombuffer(buf, dtype=np.uint8, count=b - a, offset=a)]
    h = np.zeros(b - a, dtype=np.uint64)
    for j in range(min(64, b - a)):        # bit k of h depends on the last k + 1 bytes: 64 shifted adds are the whole hash
        h[j:] += g[:b - a - j] << np.uint64(j)
    return (np.flatnonzero((h & np.uint64(mask)) == 0) + a).tolist()


def _hash_np(buf, starts, mm):
    arr = np.frombuffer(buf, dtype=np.uint8)
    w = np.array(starts, dtype=np.int64)
    x = np.full(len(starts), 0xCBF29CE484222325 ^ mm, dtype=np.uint64)
    for i in range(mm):
        x = (x ^ arr[w + i].astype(np.uint64)) * np.uint64(0x100000001B3)
    for mul in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53):
        x ^= x >> np.uint64(33); x *= np.uint64(mul)
    x ^= x >> np.uint64(33)
    return [int(v) for v in x]


def splits(buf, lay, p, loop=False, rules=None):
    """the stage's splits in position order -> ([window start], [checksum], [(frame, bucket)]), labels"""
    R = _rules(rules)
    mask, mm, hb = stop_mask(p), min(p.minMatch, 64), p.hashLog - p.bucketLog
    L = {}

    def hit(k, c=1):
        L[k] = L.get(k, 0) + c
    hit("mask-high" if 0 < p.hashRateLog <= mm else "mask-low")
    pos, frame = [], []
    seg, seg_n = -1, 0
    with np.errstate(over="ignore"):
        for fi, (a, b) in enumerate(frames_of(lay)):
            if not R["frame_restart"] and fi:
                lead = max(a - 64, 0)     # (the wrong form: warmed up on the frame in front)
                stops = [q for q in (_stops_loop if loop else _stops_np)(buf, lead, b, mask) if q >= a]
            else:
                stops = (_stops_loop if loop else _stops_np)(buf, a, b, mask)
            for q in stops:
                w = q + 1 - p.minMatch
                if w < (a if R["window_in_frame"] else lay.vlo):
                    hit("window-before-frame")
                    continue
                if q // SEG != seg:
                    seg, seg_n = q // SEG, 0
                seg_n += 1
                if seg_n > R["cap"]:
                    hit("cap-drop")
                    continue
                pos.append(w); frame.append(fi)
                k = q % SEG
                if k == 0: hit("stop-k0")
                if k == 63: hit("stop-k63")
                if q % TILE < SEG: hit("tile-first-lane")
                if q - a < 63: hit("frame-head-stop" if fi or lay.base == 0 else "prefix-head-stop")
                if fi and a % TILE and q // TILE == a // TILE: hit("frame-start-inside-tile")
                if w < (q // TILE) * TILE - 64: hit("window-front-of-tile")
                if w < lay.base < q + 1: hit("window-straddles-seam")
        hs = [window_hash(buf[w:w + mm]) for w in pos] if loop else (_hash_np(buf, pos, mm) if pos else [])
    check = [h >> 32 for h in hs]
    key = [(f, h & ((1 << hb) - 1)) for f, h in zip(frame, hs)]
    return (pos, check, key), L


def _common(arr, x, y, lim):
    """bytes arr[x + i] == arr[y + i] from i = 0 on, at most lim"""
    if lim <= 0:
        return 0
    d = np.flatnonzero(arr[x:x + lim] != arr[y:y + lim])
    return int(d[0]) if d.size else lim


def _common_back(arr, x, y, lim):
    """bytes arr[x - 1 - i] == arr[y - 1 - i] from i = 0 on, at most lim"""
    if lim <= 0:
        return 0
    d = np.flatnonzero(arr[x - lim:x][::-1] != arr[y - lim:y][::-1])
    return int(d[0]) if d.size else lim


LEN_EDGES = (255, 256, 257, 258, 511, 512, 513, 514)      # around the 256-byte compare step, every residue of a lane's four bytes


def matches(buf, lay, p, S, rules=None):
    """the walk over the splits S = (pos, check, key) -> [(mStart, mLen, mOff)] per split (mLen 0: none, then all 0), labels"""
    R = _rules(rules)
    arr = np.frombuffer(buf, dtype=np.uint8)
    pos, check, key = S
    ents = 1 << p.bucketLog
    table = {}            # (frame, bucket) -> the last `ents` insertions, oldest first (a round-robin table read newest first)
    out, L = [], {}

    def hit(k, c=1):
        L[k] = L.get(k, 0) + c
    block, anchor, searching = -1, 0, 0
    fr = frames_of(lay)
    for i, w in enumerate(pos):
        slot = table.setdefault(key[i], [])
        res = (0, 0, 0)
        if w >= lay.base:
            c = (w - lay.base) // lay.chunk
            bS = lay.base + c * lay.chunk
            bE = min(bS + lay.chunk, lay.n)
            fS = fr[key[i][0]][0]
            if c != block:
                block, anchor, searching = c, bS, 0
            if w + p.minMatch > bE:
                hit("near-block-end")
                if not R["insert_unsearched"]:
                    out.append(res)
                    continue
            elif w < anchor:
                hit("before-anchor")
            else:
                searching += 1
                if searching == 65: hit("batch-over-64")
                best = None
                order = slot[::-1] if R["nearest_first"] else slot
                if len(slot) == ents: hit("bucket-full")
                for (cw, cc) in order:
                    if R["check_filter"] and cc != check[i]:
                        hit("slot-other-checksum")
                        continue
                    if lay.maxDist and w - cw > lay.maxDist:
                        hit("maxdist-skip")
                        continue
                    if lay.maxDist and w - cw == lay.maxDist: hit("maxdist-exact")
                    fwd = _common(arr, w, cw, bE - w)
                    if R["min_on_fwd"] and fwd < p.minMatch:
                        back = _common_back(arr, w, cw, min(w - anchor, cw - fS))
                        hit("fwd-short-total-long" if fwd + back >= p.minMatch else "fwd-short")
                        continue
                    back = _common_back(arr, w, cw, min(w - anchor, cw - fS))
                    if fwd + back < p.minMatch:
                        continue
                    if best is None or (fwd + back > best[0] if R["strict"] else fwd + back >= best[0]):
                        if best is not None: hit("far-longer-wins" if R["nearest_first"] else "later-wins")
                        best = (fwd + back, fwd, back, cw)
                    elif fwd + back == best[0]: hit("tie-keeps-nearest")
                if best:
                    tot, fwd, back, cw = best
                    res = (w - back, tot, w - cw)
                    hit("match")
                    if fwd == bE - w: hit("fwd-to-block-end")
                    if back == w - anchor and back: hit("back-stop-block-start" if anchor == bS else "back-stop-anchor")
                    elif back == cw - fS: hit("back-stop-frame" if not lay.base else "back-stop-prefix-start")
                    if w - cw < tot: hit("dist-lt-len")
                    if tot == lay.chunk: hit("whole-block")
                    if fwd in LEN_EDGES: hit("fwd-%d" % fwd)
                    if back in LEN_EDGES: hit("back-%d" % back)
                    if cw < lay.base:
                        hit("cand-in-prefix")
                        if cw + fwd > lay.base: hit("fwd-crosses-seam")
                        if cw + fwd == lay.base: hit("fwd-ends-at-seam")
                        if cw + fwd == lay.base - 1: hit("fwd-ends-before-seam")
                        if cw + fwd == lay.base + 1: hit("fwd-ends-behind-seam")
                    elif cw - back < lay.base:
                        hit("back-crosses-seam")
                    if searching > 64: hit("match-in-later-batch")
                    # (w + fwd IS the match's end, w - back + tot; the wrong form leaves the anchor at the split)
                    anchor = w + fwd if R["anchor_fwd"] else w
        slot.append((w, check[i]))
        if len(slot) > ents:
            del slot[0]
            hit("bucket-evict")
        out.append(res)
    return out, L


def merge(F, L, blockLen, rules=None):
    """ldm_merge_kernel's rule: finder matches F and long-distance matches L of one block, both (start, len, distance) in block
    offsets and in order -> the merged sequences, the block's literal bytes, labels"""
    R = _rules(rules)
    lab = {}

    def hit(k, c=1):
        lab[k] = lab.get(k, 0) + c
    out, fi, li, pos, lit_start, lits = [], 0, 0, 0, 0, 0
    pieces = 0            # pieces the current finder match has given so far

    def emit(s, n, d):
        nonlocal lit_start, lits
        ll = s - lit_start
        assert ll >= 0 and n >= 3 and s + n <= blockLen
        for edge in (255, 256, 257):
            if ll == edge: hit("lit-%d" % edge)
        if ll > 60000: hit("lit-over-60000")
        lits += ll; lit_start = s + n
        out.append((s, n, d))
        if len(out) in (64, 65, 129): hit("out-%d" % len(out))
    if not L: hit("no-L")
    if len(F) > 64: hit("F-over-64")
    for _ in range(4 * (len(F) + len(L)) + 8):       # (the rule always moves on; a wrong form of it may not)
        haveL, haveF = li < len(L), fi < len(F)
        Ls, Ll, Lo = L[li] if haveL else (0, 0, 0)
        Fs, Fl, Fo = F[fi] if haveF else (0, 0, 0)
        Fe = Fs + Fl
        ps = max(Fs, pos)
        if haveL and (not haveF or (Ls <= ps if R["tie_le"] else Ls < ps)):
            if haveF and Ls == ps: hit("tie-Ls==ps")
            if not haveF: hit("L-after-last-F")
            emit(Ls, Ll, Lo); pos = Ls + Ll; li += 1
            hit("L-whole")
            continue
        if not haveF:
            break
        if Fe <= ps:
            hit("F-under-L" if ps > Fs else "F-empty")
            fi += 1; pieces = 0
            continue
        pe = Ls if haveL and Ls < Fe else Fe
        if pe - ps >= R["floor"]:
            emit(ps, pe - ps, Fo)
            pieces += 1
            if ps == Fs and pe == Fe: hit("F-whole")
            elif ps == Fs: hit("F-head-piece")
            elif pe == Fe: hit("F-tail-piece")
            else: hit("F-middle-piece")
            if pieces == 2: hit("F-two-pieces")
            if pe - ps == 4: hit("piece-4-kept")
        else:
            hit("piece-%d-dropped" % (pe - ps))
        pos = pe
        if pe == Fe:
            fi += 1; pieces = 0
    else:
        raise RuntimeError("the merge does not move on")
    lits += blockLen - lit_start
    return out, lits, lab


def stage(buf, lay, p, loop=False, rules=None):
    S, la = splits(buf, lay, p, loop=loop, rules=rules)
    M, lb = matches(buf, lay, p, S, rules=rules)
    lab = dict(la)
    for k, v in lb.items():
        lab[k] = lab.get(k, 0) + v
    return S, M, lab
