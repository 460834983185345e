"""Shared by tests/golden/make_golden_prefix.py and the refPrefix tests: the prefixes and contents of the delta cases, rebuilt from
datagen seeds on both sides, so that only the compressed frames are stored."""
import random

import datagen

MiB = 1 << 20


def edit(base: bytes, seed: int, edits: int) -> bytes:
    """`edits` seeded edits of a copy of base: a span of 1..2000 bytes is replaced by random bytes, or that many random bytes are
    inserted, or the span is deleted"""
    rng = random.Random(seed)
    out = bytearray(base)
    for _ in range(edits):
        kind = rng.choice(("replace", "insert", "delete"))
        span = rng.randint(1, 2000)
        pos = rng.randrange(0, len(out) - span)
        if kind == "replace":
            out[pos:pos + span] = rng.randbytes(span)
        elif kind == "insert":
            out[pos:pos] = rng.randbytes(span)
        else:
            del out[pos:pos + span]
    return bytes(out)


def _seam():
    r = datagen.gen("rand", 200000, 11)
    return r, r[100000:] * 2


def _small_change():
    p = datagen.gen("rand", 70001, 12)
    c = bytearray(p)
    c[35000:35003] = bytes(b ^ 0x5A for b in c[35000:35003])
    return p, bytes(c) + b"\x01\x02"


def _cut_from_the_middle():
    p = datagen.gen("rand", 3 * MiB, 13)
    return p, p[MiB + 12345:MiB + 12345 + 70003]


def _edited(kind):
    def make():
        base = datagen.gen(kind, MiB + 65536, 14)
        return base, edit(base, 5, 12)
    return make


# name -> (builder of (prefix, content), kind, level, LDM for the fixture, windowLog for the fixture)
CASES = {
    "seam": (_seam, "rand", 3, 0, 19),                      # (a) one match starts in the prefix and runs into the frame
    "small_change": (_small_change, "rand", 1, 0, 18),      # (b) 3 bytes changed in the middle, 2 appended
    "cut": (_cut_from_the_middle, "rand", 3, 1, 22),        # (c) a prefix far larger than the content
    "edited_rand": (_edited("rand"), "rand", 1, 1, 22),     # (d) content >= 1 MiB: the origin path under setLongFrames(2)
    "edited_text": (_edited("text"), "text", 3, 1, 22),
}

# the datagen / edit seeds behind each case (recorded in the manifest)
SEEDS = {"seam": dict(prefix=11), "small_change": dict(prefix=12), "cut": dict(prefix=13),
         "edited_rand": dict(base=14, edit=5, edits=12), "edited_text": dict(base=14, edit=5, edits=12)}

_built = {}


def build(name):
    """(prefix, content) of a case; built once and shared"""
    if name not in _built:
        _built[name] = CASES[name][0]()
    return _built[name]
