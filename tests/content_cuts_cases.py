"""The content-defined cut rule, version 1 (include/zstd_mi355x.h "Content-defined cuts"), restated in numpy, and the inputs the cut tests
share.  Written from the rule's text, not from the kernels: the hash is 64 shifted adds over the whole buffer, the selection one
searchsorted per piece.

    gear[i] = splitmix64(i);  h(p) = sum_{k=0..min(p,63)} gear[src[p-k]] << k  (mod 2^64)
    bits = avgLog - 1, min = 1 << (avgLog - 2), max = 65536;  p + 1 is a candidate end iff the top `bits` bits of h(p) are zero
    from a piece start s the piece ends at the smallest candidate e with e - s >= min if e - s <= max, else at s + max;
    the source's end ends the last piece; an empty source has no piece;  avgLog is 12 .. 16

tests/golden/content_cuts_v1.json holds what this file gives for six small inputs (python tests/content_cuts_cases.py writes it)."""
import functools
import json
import os

import numpy as np

import datagen

RULE_VERSION = 1
AVG_LOGS = (12, 14, 16)
MAX = 65536
TILE, LIST_BLOCK = 16384, 1024        # the mark kernel's tile and the select walk's list block (zmi_cuts.h): where planted edges go
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "content_cuts_v1.json")
M64 = (1 << 64) - 1


def splitmix64(i):
    z = ((i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


GEAR = np.array([splitmix64(i) for i in range(256)], dtype=np.uint64)


def min_of(avg_log):
    return 1 << (avg_log - 2)


def as_array(data):
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, dtype=np.uint8)


def hashes(data):
    """h(p) for every p, uint64"""
    a = as_array(data)
    n = len(a)
    g = GEAR[a]
    h = np.zeros(n, dtype=np.uint64)
    for k in range(min(64, n)):
        h[k:] += g[:n - k] << np.uint64(k)
    return h


def candidates(data, avg_log, h=None):
    """the candidate ends, ascending (int64)"""
    h = hashes(data) if h is None else h
    return np.nonzero((h >> np.uint64(64 - (avg_log - 1))) == 0)[0].astype(np.int64) + 1


def select(cands, n, avg_log):
    """the piece ends for a source of n bytes with the candidate ends `cands`"""
    mn, ends, s = min_of(avg_log), [], 0
    while s < n:
        i = int(np.searchsorted(cands, s + mn, side="left"))
        e = int(cands[i]) if i < len(cands) and int(cands[i]) - s <= MAX else s + MAX
        e = min(e, n)
        ends.append(e)
        s = e
    return ends


def piece_ends(data, avg_log):
    return select(candidates(data, avg_log), len(data), avg_log)


def piece_sizes(data, avg_log):
    ends = piece_ends(data, avg_log)
    return [e - s for s, e in zip([0] + ends[:-1], ends)]


def bound(n, avg_log):
    """ZSTDMI_contentCutsBound"""
    p = n // min_of(avg_log) + 1
    return n + (n >> 8) + 64 * p + 17 + 8 * (n // 4096 + p)


def resync(a, b):
    """piece size lists of an input and of its edited version -> (leading pieces of a, of b) in front of their longest common tail"""
    t = 0
    while t < len(a) and t < len(b) and a[len(a) - 1 - t] == b[len(b) - 1 - t]:
        t += 1
    return len(a) - t, len(b) - t


# ---- inputs ----
@functools.lru_cache(maxsize=None)
def base(kind, n=1 << 20):
    """the shared inputs: datagen's rand / text / zipf / mixed with seed 7, or `flat`: the candidate-free byte"""
    if kind == "flat":
        return bytes([flat_byte()]) * n
    return datagen.gen(kind, n, 7)


@functools.lru_cache(maxsize=None)
def flat_byte():
    """the lowest byte value whose constant run has no candidate at any avgLog (h is constant from the 64th byte on, and avgLog 12 asks
    for the fewest zero bits)"""
    for b in range(256):
        if len(candidates(bytes([b]) * 256, 12)) == 0:
            return b
    raise AssertionError("no candidate-free byte")


def insert_edit(data):
    """the resync tests' edit: three bytes inserted at offset 5000"""
    return data[:5000] + b"\x01\x02\x03" + data[5000:]


GOLDEN_INPUTS = [("rand", 200000, 12), ("text", 200000, 12), ("zipf", 200000, 14), ("text", 200000, 16), ("mixed", 200000, 12), ("flat", 140000, 12)]


def golden_cases():
    return [{"kind": k, "size": n, "avgLog": a, "pieces": piece_sizes(base(k)[:n], a)} for k, n, a in GOLDEN_INPUTS]


# ---- planted edges: a candidate end moved to a place where the kernels change path.  Every builder checks with the restatement that
# the edge is where it should be in the buffer it returns. ----
@functools.lru_cache(maxsize=None)
def _rand(n):
    return datagen.gen("rand", n, 11)


def _front_cut(avg_log, modulus, want, what):
    """rand with bytes cut off the front so that a SELECTED candidate end e has (e - 1) % modulus == want"""
    buf = _rand(300000)
    for e in piece_ends(buf, avg_log)[8:]:
        k = (e - 1 - want) % modulus
        out = buf[k:]
        cs, ends = candidates(out, avg_log), piece_ends(out, avg_log)
        hit = [x for x in ends[:-1] if (x - 1) % modulus == want and x in set(cs.tolist())]
        if hit:
            return out
    raise AssertionError(what)


def _spliced(avg_log, gap, filler):
    """rand[:c1] + filler + rand[c2 - 64:], c1 a selected candidate end, c2 a later candidate: in the result c1 is a piece end and
    c1 + gap is a candidate end (its 64 bytes are c2's), gap = len(filler) + 64.  -> (buffer, c1)"""
    buf = _rand(300000)
    cs = candidates(buf, avg_log)
    cset = set(cs.tolist())
    for c1 in [e for e in piece_ends(buf, avg_log)[4:] if e in cset]:
        for c2 in cs[cs > c1 + 70000][:6].tolist():
            out = buf[:c1] + filler + buf[c2 - 64:]
            ends, oc = piece_ends(out, avg_log), set(candidates(out, avg_log).tolist())
            between = [x for x in oc if c1 < x < c1 + gap]
            if c1 in ends and c1 + gap in oc and (len(filler) < 64 or not between):
                return out, c1
    raise AssertionError("no splice")


@functools.lru_cache(maxsize=None)
def planted(name, avg_log=12):
    """-> the buffer of the planted case `name`"""
    mn, flat = min_of(avg_log), bytes([flat_byte()])
    if name.startswith("tile"):                 # tile0 / tile1 / tile16383: the candidate's byte at that offset of a mark tile
        return _front_cut(avg_log, TILE, int(name[4:]), name)
    if name.startswith("lane"):                 # lane63 / lane64: the last byte of a lane's 64 positions, the first of the next lane's
        return _front_cut(avg_log, 128, int(name[4:]), name)
    if name in ("min-1", "min"):                # a candidate min - 1 (skipped) or min (taken) bytes behind a piece start
        gap = mn - 1 if name == "min-1" else mn
        buf = _rand(300000)
        cs = candidates(buf, avg_log)
        cset = set(cs.tolist())
        for c1 in [e for e in piece_ends(buf, avg_log)[4:] if e in cset]:
            for c2 in cs[cs > c1 + 3 * mn][:6].tolist():
                out = buf[:c1] + buf[c2 - gap:]
                ends, oc = piece_ends(out, avg_log), set(candidates(out, avg_log).tolist())
                if c1 in ends and c1 + gap in oc and ((c1 + gap in ends) == (name == "min")):
                    return out
        raise AssertionError(name)
    if name in ("max", "max+1"):                # no candidate for max - 1 bytes, then one at s + max (taken) or s + max + 1 (a forced cut first)
        gap = MAX if name == "max" else MAX + 1
        out, c1 = _spliced(avg_log, gap, flat * (gap - 64))
        ends = piece_ends(out, avg_log)
        assert c1 + MAX in ends and ((c1 + gap in ends) == (name == "max")), name
        return out
    if name == "desert":                        # more than 3 x 64 KiB without a candidate between two candidate-rich stretches
        gap = 3 * MAX + 5000
        out, c1 = _spliced(avg_log, gap, flat * (gap - 64))
        ends = piece_ends(out, avg_log)
        assert all(c1 + k * MAX in ends for k in (1, 2, 3)) and len(ends) > ends.index(c1 + 3 * MAX) + 3, name
        return out
    if name in ("block-last", "block-first"):   # a selected candidate at index LIST_BLOCK - 1 / LIST_BLOCK of the candidate list
        want = LIST_BLOCK - 1 if name == "block-last" else LIST_BLOCK
        buf = _rand(3 << 20)
        cs = candidates(buf, avg_log)
        picked = set(piece_ends(buf, avg_log))
        for j in [j for j in range(want + 4, len(cs)) if int(cs[j]) in picked][:40]:
            k = int(cs[j - want - 1])           # cut behind the candidate that lies `want` + 1 in front: `want` candidates stay in front
            out = buf[k:]
            oc, ends = candidates(out, avg_log), piece_ends(out, avg_log)
            if len(oc) > want + 1 and int(oc[want]) in ends:
                return out
        raise AssertionError(name)
    raise ValueError(name)


PLANTED = ["tile0", "tile1", "tile16383", "lane63", "lane64", "min-1", "min", "max", "max+1", "block-last", "block-first", "desert"]


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump({"rule_version": RULE_VERSION, "cases": golden_cases()}, f, separators=(",", ":"))
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
