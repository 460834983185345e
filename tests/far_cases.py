"""Forged frames whose matches reach 2^29 bytes and further back: what zstd --long=30 / 31 or --patch-from writes for a large file,
in the smallest shape there is (an offset of 2^29 needs 512 MiB in front of it).  Built at run time with tests/zstd_forge.py; a frame
is 20 - 40 KiB, nothing large is committed.

Every frame is: 4 KiB of seeded random bytes (raw block), RLE blocks of zeros up to the far end, then one or two compressed blocks
whose far offsets land in the seed (or in the dictionary) — a decoder that loses a bit of the offset copies zeros instead.  The
offset table of such a block is FSE-coded: the predefined one ends at code 28.

build(name) -> a dict:
  blob      the frame
  valid     the forge's belief (the format's words); an invalid case has no content
  size      content bytes          cap   a destination that holds it (the frame's bound where its header has no size)
  head      content[:4096]         tail  content[tail_off:]       everything between them is zero (checked by the CPU test)
  dict      a raw-content dictionary, or None
  content   the forge's own executor's bytes — only with keep_content=True (512 MiB to 1 GiB)
  below_1g  the frame is below 1 GiB (the origin path may take it)
"""
import random

import zstd_forge as F
from forge_cases import cblock, fse_mode, raw, rawlit, rle

SEED_BYTES = 4096
BLOCK = 1 << 17
FAR = 1 << 29                   # the first offset a sequence record cannot pack


def seed_block():
    r = random.Random(0xFA12)
    return bytes(r.randrange(1, 256) for _ in range(SEED_BYTES))        # (no zero: a seed byte never looks like the fill)


def front(total):
    """raw seed + RLE zero blocks: `total` bytes in front of the first compressed block"""
    blocks, left = [raw(seed_block())], total - SEED_BYTES
    while left:
        n = min(left, BLOCK)
        blocks.append(rle(0, n))
        left -= n
    return blocks


def lits(seed, n):
    r = random.Random(seed)
    return bytes(r.randrange(1, 256) for _ in range(n))


def far_block(seqs, seed, trailing=7, **kw):
    """a compressed block over raw literals with an FSE offset table fitted to its codes"""
    return cblock(rawlit(lits(seed, sum(s[0] for s in seqs) + trailing)), seqs, of=fse_mode("of", seqs, 6), **kw)


def three(off):
    """the far offset, its repeat inside the same batch of records, and a near offset"""
    return [(5, off + 3, 200), (3, 1, 50), (0, 10, 9)]


def _edge(off):
    # the compressed block starts at 2^29 + 95: its first match stands at 2^29 + 100 and an offset of 2^29 reads seed[100:]
    return dict(blocks=front(FAR + 95) + [far_block(three(off), 1)])


def _code29():
    # 4 KiB + 4096 RLE blocks of 128 KiB; offset 536 874 913 (code 29) from 2^29 + 4101 reads seed[100:]
    return dict(blocks=front(SEED_BYTES + 4096 * BLOCK) + [far_block(three(536874913), 2)])


def _rep_next_block():
    # block A leaves the far offset as repeat offset 1 (and 7, 1 behind it); block B uses it — through the block's starting repcodes — and then
    # "repeat offset 1 minus one" with no literals in front
    off = 536874913
    a = far_block([(5, off + 3, 200), (3, 10, 9)], 3)
    b = cblock(rawlit(lits(4, 4 + 9)), [(4, 1, 100), (0, 3, 30)])
    return dict(blocks=front(SEED_BYTES + 4096 * BLOCK) + [a, b])


def _alternating():
    # 130 sequences (three batches of 64 records: 64 + 64 + 2), far and near offsets in turn; sequence 71 repeats the far offset in front
    # of it, so the first batch resolves no repcode, the second walks its slots one by one, and the last holds fewer than three records
    start = SEED_BYTES + 4096 * BLOCK
    seqs, pos = [], start
    for i in range(130):
        pos += 2
        if i == 71:
            seqs.append((2, 1, 20))                                     # repeat offset 1: the far offset of sequence 70
        elif i % 2 == 0:
            seqs.append((2, pos - (50 + 23 * i) + 3, 20))               # far: reads seed[50 + 23 i :]
        else:
            seqs.append((2, 30 + i + 3, 20))                            # near
        pos += 20
    return dict(blocks=front(start) + [far_block(seqs, 5)])


def _code30():
    # 4 KiB + 8192 RLE blocks: offset 1 073 745 735 (code 30) from 2^30 + 4101 reads seed[190:].  1 GiB and more: the ordered walk
    return dict(blocks=front(SEED_BYTES + 8192 * BLOCK) + [far_block(three(1073745735), 6)])


def _window30(sized):
    # a window descriptor for 2^30 (exponent 20, mantissa 0) over the code-29 layout, with a 4-byte content size or with none
    return dict(blocks=_code29()["blocks"], single=False, window=20 << 3, fcs=4 if sized else 0)


def _raw_dict():
    # a raw dictionary of 1000 bytes in front of the code-29 layout: the match at p reaches p + 500 back, 500 bytes inside the dictionary
    p = SEED_BYTES + 4096 * BLOCK + 5
    return dict(blocks=front(p - 5) + [far_block(three(p + 500), 7)], dict=lits(8, 1000))


def _before_frame():
    # INVALID: the far offset names the byte in front of the frame's first
    p = SEED_BYTES + 4096 * BLOCK + 5
    return dict(blocks=front(p - 5) + [far_block([(5, p + 1 + 3, 200), (3, 10, 9)], 9)], valid=False)


CASES = {
    "last_packed_offset": lambda: _edge(FAR - 1),
    "first_far_offset": lambda: _edge(FAR),
    "code29": _code29,
    "repeat_in_next_block": _rep_next_block,
    "alternating_130": _alternating,
    "code30_walk": _code30,
    "window30_sized": lambda: _window30(True),
    "window30_unsized": lambda: _window30(False),
    "raw_dict_1000": _raw_dict,
    "before_frame": _before_frame,
}
VALID = [n for n in CASES if n != "before_frame"]
INVALID = ["before_frame"]
# every valid case but this one states an offset of 2^29 or more (it is the last offset a record packs, in a frame that is far-capable)
NEEDS_FAR = [n for n in VALID if n != "last_packed_offset"]


def build(name, keep_content=False):
    d = CASES[name]()
    blocks, dic, valid = d.pop("blocks"), d.pop("dict", None), d.pop("valid", True)
    n_front = next(i for i, b in enumerate(blocks) if b["t"] == "c")
    tail_off = sum(len(b["data"]) if b["t"] == "raw" else b["size"] for b in blocks[:n_front])
    if valid and not dic:
        blob, content = F.frame(blocks, **d)            # (content: the forge's own executor's)
        stated = len(content)
    else:
        # behind a dictionary the forge's executor runs over dictionary + frame, and the frame is written as an "invalid" description
        # (its offsets leave the frame) that states its content size; an invalid case states the size it would have
        assert not d
        content = F.execute([raw(dic)] + blocks)[len(dic):] if valid else None
        stated = len(content) if valid else tail_off + sum(s[0] + s[2] for s in blocks[n_front]["seqs"]) + 7
        blob, _ = F.frame(blocks, valid=False, fcs_value=stated)
    size = len(content) if valid else 0
    sized = d.get("fcs", 4) != 0
    case = dict(name=name, blob=blob, valid=valid, size=size, dict=dic, tail_off=tail_off, below_1g=stated < (1 << 30),
                cap=stated if sized else len(blocks) * BLOCK, head=None, tail=None, content=None)
    if valid:
        case["head"], case["tail"] = content[:SEED_BYTES], content[tail_off:]
        if keep_content:
            case["content"] = content
    return case
