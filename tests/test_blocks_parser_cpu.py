"""CPU tests of tests/zstd_blocks.py, the frame / block parser and state checker the entropy-carry tests look at their output with:
it accepts the golden forged frames that use treeless literals and repeat-mode tables where the format allows them, and rejects the
two that use them in a frame's first compressed block.  No kernel is launched."""
import glob
import os

import pytest

import zstd_blocks as zb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return open(os.path.join(GOLDEN, name + ".zst"), "rb").read()


def names(pattern):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, pattern + ".zst")))


TREELESS = names("forge_huf_treeless_*")
REPEAT = names("forge_seq_repeat_*")
MODES = names("forge_seq_modes_*")


def test_the_golden_sets_are_there():
    assert len(TREELESS) == 4 and len(REPEAT) == 3 and len(MODES) == 27


@pytest.mark.parametrize("name", TREELESS)
def test_accepts_treeless_frames(name):
    frames = zb.frames_of(golden(name))
    assert frames
    infos = [b for f in frames for b in zb.check_frame_state(f)]
    assert any(b.treeless for b in infos), "the frame's name says treeless"
    # the table was defined by an earlier block of the same frame, with blocks that do not touch it in between
    first = next(b for b in infos if b.treeless)
    assert first.index > 0


@pytest.mark.parametrize("name", REPEAT)
def test_accepts_repeat_frames(name):
    infos = [b for f in zb.frames_of(golden(name)) for b in zb.check_frame_state(f)]
    assert any(b.repeats for b in infos), "the frame's name says repeat"


@pytest.mark.parametrize("name", MODES)
def test_accepts_every_mode_combination(name):
    want = {"predef": 0, "rle": 1, "fse": 2}
    ll, of, ml = (want[w] for w in name.split("_")[-3:])
    infos = [b for f in zb.frames_of(golden(name)) for b in zb.check_frame_state(f)]
    assert any(b.modes == (ll, of, ml) for b in infos if b.modes is not None), [b.modes for b in infos]


@pytest.mark.parametrize("name, what", [("forge_neg_treeless_in_first_block", "treeless literals"),
                                        ("forge_neg_repeat_in_first_block", "repeat mode"),
                                        ("forge_neg_repeat_of_in_first_block", "repeat mode")])
def test_rejects_use_before_definition(name, what):
    frame = zb.frames_of(golden(name))[0]
    with pytest.raises(AssertionError, match=what):
        zb.check_frame_state(frame)


def test_group_rule_rejects_what_the_format_allows():
    """a treeless block is fine for the format wherever a table was defined before it; with the group size given, a group's first
    block may not be one, and a later block may not reach behind its group's start"""
    frame = zb.frames_of(golden("forge_huf_treeless_gap_s1"))[0]
    infos = zb.check_frame_state(frame)
    t = next(b.index for b in infos if b.treeless)
    with pytest.raises(AssertionError, match="carry group's first block"):
        zb.check_frame_state(frame, group=t)          # the treeless block leads a group
    assert zb.check_frame_state(frame, group=t + 1)   # the defining block and the treeless one share the first group
    assert zb.carry_groups(infos, 8) == (len(infos) + 7) // 8


def test_frame_sizes_add_up():
    for name in TREELESS + REPEAT + MODES[:3]:
        data = golden(name)
        assert sum(len(f) for f in zb.frames_of(data, skippable=True)) == len(data)
