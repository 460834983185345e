"""A small zstd frame / block parser for the tests (the one tests/test_gpu_dict_entropy.py looks at first blocks with, in a module of
its own and without the oracle), and a STATE CHECKER on top of it: check_frame_state walks a frame's blocks the way a decoder's
entropy state evolves and asserts that nothing is used before it was defined.

What is read of a block: the literals type is the low two bits of a compressed block body's first byte (3 = treeless: the Huffman
table of an earlier block), and the byte behind the sequence count holds the three table modes, LL << 6 | OF << 4 | ML << 2
(3 = repeat: the table of the previous compressed block with sequences)."""

MAGIC = b"\x28\xB5\x2F\xFD"


def frame_header_size(frame):
    assert frame[:4] == MAGIC, frame[:4]
    fhd = frame[4]
    did, single, fcs = fhd & 3, (fhd >> 5) & 1, fhd >> 6
    return 5 + (0 if single else 1) + (4 if did == 3 else did) + ((1 if single else 0) if fcs == 0 else 1 << fcs)


def frame_size(stream, pos=0):
    """bytes of the frame (zstd or skippable) that begins at stream[pos]"""
    magic = int.from_bytes(stream[pos:pos + 4], "little")
    if magic & 0xFFFFFFF0 == 0x184D2A50:
        return 8 + int.from_bytes(stream[pos + 4:pos + 8], "little")
    frame = stream[pos:]
    at = frame_header_size(frame)
    while True:
        h = int.from_bytes(frame[at:at + 3], "little")
        assert at + 3 <= len(frame), "block header behind the stream's end"
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        at += 3 + (1 if btype == 1 else size)
        if last:
            return at + (4 if frame[4] & 4 else 0)


def frames_of(stream, skippable=False):
    """a stream -> its zstd frames in order (skippable frames — a seek table — are left out unless asked for)"""
    out, pos = [], 0
    while pos < len(stream):
        n = frame_size(stream, pos)
        assert n > 0 and pos + n <= len(stream), (pos, n, len(stream))
        if skippable or stream[pos:pos + 4] == MAGIC:
            out.append(stream[pos:pos + n])
        pos += n
    return out


def blocks_of(frame):
    """one frame -> [(block type, body)] in order (type 0 raw, 1 RLE, 2 compressed)"""
    pos = frame_header_size(frame)
    out = []
    while True:
        h = int.from_bytes(frame[pos:pos + 3], "little")
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        body = frame[pos + 3:pos + 3 + (1 if btype == 1 else size)]
        out.append((btype, body)); pos += 3 + len(body)
        if last:
            return out


def literals_of(body):
    """the literals section of a compressed block's body -> (literals type, regenerated size, bytes of the section)"""
    b0 = body[0]
    lit_type, fmt = b0 & 3, (b0 >> 2) & 3
    if lit_type < 2:
        lh = (1, 2, 1, 3)[fmt]
        size = int.from_bytes(body[:lh], "little") >> (3 if lh == 1 else 4)
        return lit_type, size, lh + (size if lit_type == 0 else 1)
    v = int.from_bytes(body[:5].ljust(5, b"\0"), "little")
    if fmt < 2:
        return lit_type, (v >> 4) & 0x3FF, 3 + ((v >> 14) & 0x3FF)
    if fmt == 2:
        return lit_type, (v >> 4) & 0x3FFF, 4 + ((v >> 18) & 0x3FFF)
    return lit_type, (v >> 4) & 0x3FFFF, 5 + ((v >> 22) & 0x3FFFF)


def parse_block(body):
    """the body of a compressed block -> (literals type, nbSeq, sequences mode byte or None when there are no sequences)"""
    lit_type, _, pos = literals_of(body)
    n = body[pos]
    if n == 0:
        return lit_type, 0, None
    if n < 128:
        return lit_type, n, body[pos + 1]
    if n < 255:
        return lit_type, ((n - 128) << 8) + body[pos + 1], body[pos + 2]
    return lit_type, body[pos + 1] + (body[pos + 2] << 8) + 0x7F00, body[pos + 3]


def modes_of(mode_byte):
    """-> (LL, OF, ML) modes: 0 predefined, 1 RLE, 2 described, 3 repeat"""
    return ((mode_byte >> 6) & 3, (mode_byte >> 4) & 3, (mode_byte >> 2) & 3)


class BlockInfo:
    """one block as the checker saw it"""
    __slots__ = ("index", "type", "lit_type", "lit_size", "nb_seq", "modes", "size")

    def __init__(self, index, btype, lit_type=None, lit_size=0, nb_seq=0, modes=None, size=0):
        self.index, self.type, self.lit_type, self.lit_size, self.nb_seq, self.modes, self.size = index, btype, lit_type, lit_size, nb_seq, modes, size

    @property
    def treeless(self):
        return self.type == 2 and self.lit_type == 3

    @property
    def repeats(self):
        """tables in repeat mode (0 .. 3)"""
        return sum(1 for m in self.modes if m == 3) if self.modes else 0

    @property
    def carried(self):
        return self.treeless or self.repeats > 0


def check_frame_state(frame, group=None, first_index=0):
    """Walk the frame's blocks as a decoder's entropy state evolves and assert that
      * a treeless literals section (type 3) has a Huffman table defined earlier in the frame (a compressed block with a
        Compressed_Literals section; raw and RLE blocks, raw and RLE literals do not touch it),
      * a table in repeat mode (3) follows a compressed block with sequences,
      * with `group` given (the carry group size): a block whose index in the frame is a multiple of it uses neither, and what a
        later block of the group uses was defined inside the group
        (first_index: the index of the frame's first block here, for a frame looked at in pieces).
    -> [BlockInfo] of the frame's blocks."""
    huf_defined = False
    seq_defined = False
    out = []
    for i, (btype, body) in enumerate(blocks_of(frame)):
        idx = first_index + i
        if group is not None and idx % group == 0:      # (the encoder's contract is narrower than the format: nothing crosses a group's start)
            huf_defined = seq_defined = False
        if btype != 2:
            out.append(BlockInfo(idx, btype, size=len(body)))
            continue
        lit_type, lit_size, _ = literals_of(body)
        _, nb_seq, mode_byte = parse_block(body)
        modes = modes_of(mode_byte) if mode_byte is not None else None
        info = BlockInfo(idx, btype, lit_type, lit_size, nb_seq, modes, len(body))
        leads = group is not None and idx % group == 0
        if lit_type == 3:
            assert not leads, f"block {idx}: treeless literals in a carry group's first block"
            assert huf_defined, f"block {idx}: treeless literals without a Huffman table defined earlier in the frame"
        if modes is not None and 3 in modes:
            assert not leads, f"block {idx}: repeat mode in a carry group's first block"
            assert seq_defined, f"block {idx}: repeat mode without an earlier compressed block with sequences"
        if lit_type == 2:
            huf_defined = True
        if nb_seq:
            seq_defined = True
        out.append(info)
    return out


def check_stream_state(stream, group=None):
    """every zstd frame of the stream through check_frame_state -> [[BlockInfo]] per frame"""
    return [check_frame_state(f, group) for f in frames_of(stream)]


def carry_groups(infos, group):
    """the carry groups of a frame of len(infos) blocks"""
    return (len(infos) + group - 1) // group
