"""Candidate lists the tests of the parallel cut selection share (zmi_cut_rank.h; ZSTDMI_contentCutsAsync): the crafted lists of
test_content_cuts_cpu.py's walk table, built the same way, and the expected piece ends from the numpy restatement
(content_cuts_cases.select).  A case is (n, avgLog, candidates)."""
import functools

import numpy as np

import content_cuts_cases as cc

TOP = (1 << 32) - 1


@functools.lru_cache(maxsize=None)
def crafted():
    """lists that need no source buffer: pairs at every distance around min, max, max + min and k max from a piece start, a regular
    comb, every position a candidate (the longest path: what the round count must cover), and the 2^32 - 1 tails"""
    cases = []
    for avg_log in cc.AVG_LOGS:
        mn = cc.min_of(avg_log)
        for d in (mn - 1, mn, mn + 1, cc.MAX - 1, cc.MAX, cc.MAX + 1, cc.MAX + mn - 1, cc.MAX + mn, 2 * cc.MAX, 2 * cc.MAX + 1, 3 * cc.MAX + mn - 1):
            for tail in (0, 1, mn, cc.MAX, cc.MAX + 1):
                cases.append((mn + d + tail, avg_log, [mn, mn + d]))
                cases.append((mn + d + tail, avg_log, [mn, mn + d - 1, mn + d, mn + d + 1]))
        cases.append((5 * cc.MAX, avg_log, list(range(1, 5 * cc.MAX + 1, 7))))
        cases.append((300000, avg_log, list(range(1, 300001))))
        for tail in ([TOP], [TOP - 10], [TOP - mn + 1, TOP], [TOP - mn, TOP - 1], [TOP - mn - 1], [TOP - cc.MAX - 1, TOP - cc.MAX + mn - 2], []):
            cases.append((TOP, avg_log, [mn, 2 * cc.MAX + 7] + tail))
        cases.append((TOP - 1, avg_log, [TOP - 3 * mn, TOP - 2]))
    return tuple((n, a, tuple(c for c in cands if c <= n)) for n, a, cands in cases)


@functools.lru_cache(maxsize=None)
def real():
    """the candidate lists of the shared inputs, for sizes around min, 65536 and 1 MiB"""
    cases = []
    for kind in ("rand", "text", "zipf", "flat"):
        h = cc.hashes(cc.base(kind))
        for avg_log in cc.AVG_LOGS:
            mn = cc.min_of(avg_log)
            all_c = cc.candidates(None, avg_log, h)
            for n in (0, 1, mn - 1, mn, mn + 1, 65535, 65536, 65537, 200000, 1 << 20):
                cases.append((n, avg_log, tuple(all_c[all_c <= n].tolist())))
    return tuple(cases)


def clusters(avg_log=12, first=3000, gap=cc.MAX + 100, second=20000):
    """a dense cluster (every position a candidate), a gap above max, a dense cluster of `second` entries: every node in front of the gap
    whose piece crosses it lands in the second cluster's first bad zone, and a search that went entry by entry would read min of them"""
    a = list(range(1, first + 1))
    b = list(range(first + gap, first + gap + second))
    return (b[-1] + 5000, avg_log, tuple(a + b))


@functools.lru_cache(maxsize=None)
def expected(case):
    n, avg_log, cands = case
    return cc.select(np.array(cands, dtype=np.int64), n, avg_log)


@functools.lru_cache(maxsize=None)
def planted_wide(name, avg_log):
    """content_cuts_cases.planted's `min-1`, `max+1` and `desert` by the same recipes over 2 MiB of rand: at avgLog 16 its 300 000 bytes
    hold nine candidates, too few for any of the three.  Every result is checked with the restatement to have the edge where it should
    be, and ends 200 000 bytes behind it."""
    import datagen
    buf = datagen.gen("rand", 2 << 20, 11)
    mn, flat = cc.min_of(avg_log), bytes([cc.flat_byte()])
    cs = cc.candidates(buf, avg_log)
    cset = set(cs.tolist())
    starts = [e for e in cc.select(cs, len(buf), avg_log)[4:] if e in cset]
    for c1 in starts[:12]:
        if name == "min-1":             # a candidate min - 1 bytes behind a piece start: skipped
            for c2 in cs[cs > c1 + 3 * mn][:6].tolist():
                out = (buf[:c1] + buf[c2 - (mn - 1):])[:c1 + 200000]
                ends, oc = cc.piece_ends(out, avg_log), set(cc.candidates(out, avg_log).tolist())
                if c1 in ends and c1 + mn - 1 in oc and c1 + mn - 1 not in ends:
                    return out
            continue
        gap = cc.MAX + 1 if name == "max+1" else 3 * cc.MAX + 5000      # no candidate for gap - 1 bytes behind a piece start, then one
        for c2 in cs[cs > c1 + 70000][:6].tolist():
            out = (buf[:c1] + flat * (gap - 64) + buf[c2 - 64:])[:c1 + gap + 200000]
            ends, oc = cc.piece_ends(out, avg_log), set(cc.candidates(out, avg_log).tolist())
            if c1 not in ends or c1 + gap not in oc or [x for x in oc if c1 < x < c1 + gap]:
                continue
            if name == "max+1" and c1 + cc.MAX in ends and c1 + gap not in ends:
                return out
            if name == "desert" and all(c1 + k * cc.MAX in ends for k in (1, 2, 3)) and len(ends) > ends.index(c1 + 3 * cc.MAX) + 3:
                return out
    raise AssertionError(name)
