"""CPU tests: the serial model of the long-distance stage (tests/ldm_model.py) and the case table (tests/ldm_cases.py) are what they
say, with no GPU: the per-byte hashes equal the vectorised ones, every modelled match is equal bytes, maximal within the limits the
model states, in order and without overlap, every case reaches the labels it names, merge() reaches every one of its labels on
synthetic lists, and single-rule flips of the model each change the result of a named case (so a kernel that is wrong in that one
way cannot equal the model there)."""
import ctypes

import pytest

import ldm_cases
import ldm_model as lm
from zstdsharp_amd import _ffi

CASES = ldm_cases.cases()
BY_NAME = {c["name"]: c for c in CASES}
_staged = {}


def staged(name):
    if name not in _staged:
        lay, p, buf = ldm_cases.framing(BY_NAME[name])
        _staged[name] = (lay, p, buf) + lm.stage(buf, lay, p)
    return _staged[name]


def test_hooks_are_declared_exported_and_typed():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    u = ctypes.POINTER(ctypes.c_uint)
    assert hasattr(raw, "ZSTDMI_debugLdmPass") and hasattr(raw, "ZSTDMI_debugLdmSkipMerge")
    assert _ffi.SIGNATURES["ZSTDMI_debugLdmPass"] == (ctypes.c_size_t, [ctypes.c_void_p, u, u, u, u, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), u, u])
    assert _ffi.SIGNATURES["ZSTDMI_debugLdmSkipMerge"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int])


def test_case_names_are_unique_and_sizes_bounded():
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        assert 64 * 1024 < len(c["data"]) <= 2 << 20, c["name"]


def test_gear_table_and_stop_mask():
    assert lm.GEAR[0] == 0xE220A8397B1DCDAF and len(set(lm.GEAR)) == 256          # splitmix64's first output for the seed 0
    assert lm.stop_mask(lm.Params(64, 0, 0, 7)) == 0x7F << 57                       # hashRateLog <= min(minMatch, 64): the window's top bits
    assert lm.stop_mask(lm.Params(1024, 0, 0, 7)) == 0x7F << 57
    assert lm.stop_mask(lm.Params(16, 0, 0, 5)) == 0x1F << 11
    assert lm.stop_mask(lm.Params(5, 0, 0, 5)) == 0x1F
    assert lm.stop_mask(lm.Params(4, 0, 0, 7)) == 0x7F                              # above it: the low bits


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_per_byte_hashes_equal_the_vectorised_ones(name):
    lay, p, buf, S = staged(name)[:4]
    assert lm.splits(buf, lay, p, loop=True)[0] == S


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_case_reaches_its_labels_and_its_matches_are_sound(name):
    c = BY_NAME[name]
    lay, p, buf, S, M, lab = staged(name)
    missing = [k for k in c["labels"] if k not in lab]
    assert not missing, (missing, sorted(lab))
    assert not [k for k in c["absent"] if k in lab]
    if "want_splits" in c:
        assert len(S[0]) == c["want_splits"]
    assert S[0] == sorted(S[0]) and len(set(S[0])) == len(S[0])
    frames = lm.frames_of(lay)
    end = lay.base
    for w, key, (s, n, off) in zip(S[0], S[2], M):
        fS, fE = frames[key[0]]
        assert fS <= w and w + p.minMatch <= fE, "a window leaves its frame"
        if not n:
            assert (s, off) == (0, 0)
            continue
        bS = lay.base + (w - lay.base) // lay.chunk * lay.chunk
        bE = min(bS + lay.chunk, lay.n)
        assert n >= p.minMatch and off >= 1 and s - off >= fS, "a match reaches in front of its frame"
        assert not lay.maxDist or off <= lay.maxDist
        assert buf[s:s + n] == buf[s - off:s - off + n], "a modelled match is not equal bytes"
        assert max(end, bS) <= s <= w and w + p.minMatch <= s + n <= bE, "matches lie in order, apart, inside their block"
        # maximal: one byte more on either side differs or crosses a limit (block end; the match in front, block and frame start)
        assert s + n == bE or buf[s + n] != buf[s + n - off]
        assert s == max(end, bS) or s - off == fS or buf[s - 1] != buf[s - 1 - off]
        end = s + n


def test_copies_across_a_frame_boundary_are_not_matched():
    lay, p, buf, S, M, _ = staged("four_frames")
    assert not any(n and 131072 <= s < 131072 + 8000 for s, n, _ in M)          # frame 1's head is frame 0's tail: out of reach
    assert any(n and 2 * 131072 + 70000 <= s < 2 * 131072 + 72500 for s, n, _ in M)
    cut = [(s, n) for s, n, _ in M if n and s + n == 3 * 131072]
    assert cut and cut[0][0] >= 3 * 131072 - 1000, "the copy that straddles into frame 3 is matched up to the frame's end"


SYNTH = [
    # (F, L, blockLen, labels that must be reached): (start, length, distance) in block offsets
    ([], [(100, 200, 5000)], 1000, ["L-whole", "L-after-last-F"]),
    ([(10, 8, 3)], [], 100, ["no-L", "F-whole"]),
    ([(120, 50, 7)], [(100, 200, 5000)], 1000, ["F-under-L"]),
    ([(90, 30, 7)], [(100, 200, 5000)], 1000, ["F-head-piece"]),
    ([(280, 40, 7)], [(100, 200, 5000)], 1000, ["F-tail-piece"]),
    ([(90, 300, 7)], [(100, 200, 5000)], 1000, ["F-head-piece", "F-tail-piece", "F-two-pieces"]),
    ([(90, 300, 7)], [(100, 50, 5000), (200, 50, 6000)], 1000, ["F-middle-piece"]),
    ([(97, 30, 7)], [(100, 200, 5000)], 1000, ["piece-3-dropped"]),
    ([(96, 30, 7)], [(100, 200, 5000)], 1000, ["piece-4-kept"]),
    ([(280, 23, 7)], [(100, 200, 5000)], 1000, ["piece-3-dropped"]),
    ([(100, 30, 7)], [(100, 200, 5000)], 1000, ["tie-Ls==ps", "F-under-L"]),
    ([(50, 100, 7)], [(100, 200, 5000)], 1000, ["F-head-piece"]),
    ([(255, 10, 3), (265 + 256, 10, 3), (531 + 257, 10, 3)], [(900, 70, 4000)], 1000, ["lit-255", "lit-256", "lit-257"]),
    ([], [(60001, 100, 70000)], 65536, ["lit-over-60000"]),
    ([(i * 10, 6, 2) for i in range(130)], [(1400, 100, 9000)], 2000, ["F-over-64", "out-64", "out-65", "out-129"]),
]


@pytest.mark.parametrize("i", range(len(SYNTH)))
def test_merge_on_synthetic_lists(i):
    F, L, n, want = SYNTH[i]
    out, lits, lab = lm.merge(F, L, n)
    assert not [k for k in want if k not in lab], (want, lab)
    # what every merge must keep: the long-distance matches whole, sequences in order and apart, every finder piece inside its match
    # with its offset, no piece under 4 bytes, literals + matches = the block
    for m in L:
        assert m in out
    pos = 0
    for s, ln, d in out:
        assert s >= pos and ln >= 4
        pos = s + ln
        assert (s, ln, d) in L or any(fs <= s and s + ln <= fs + fl and d == fo for fs, fl, fo in F)
    assert lits + sum(ln for _, ln, _ in out) == n


def test_merge_reaches_every_label_it_has():
    reached = set()
    for F, L, n, _ in SYNTH:
        reached |= set(lm.merge(F, L, n)[2])
    named = {"L-whole", "L-after-last-F", "no-L", "F-whole", "F-under-L", "F-head-piece", "F-tail-piece", "F-middle-piece", "F-two-pieces",
             "piece-4-kept", "piece-3-dropped", "tie-Ls==ps", "lit-255", "lit-256", "lit-257", "lit-over-60000", "F-over-64", "out-64",
             "out-65", "out-129"}
    assert named <= reached, named - reached


def test_merge_worked_example():
    """a finder match around a long-distance match, a 3-byte and a 4-byte piece: by hand"""
    F = [(10, 6, 2), (96, 120, 7), (217, 10, 9), (300, 8, 5)]
    L = [(100, 100, 5000), (220, 50, 6000)]
    out, lits, _ = lm.merge(F, L, 400)
    #   (96..216, off 7) gives 96..100 (4 bytes: kept) and 200..216; (217..227, off 9) gives 217..220 (3 bytes: literals)
    assert out == [(10, 6, 2), (96, 4, 7), (100, 100, 5000), (200, 16, 7), (220, 50, 6000), (300, 8, 5)]
    assert lits == 400 - (6 + 4 + 100 + 16 + 50 + 8)


# single-rule flips: (the rule's wrong form, the case whose splits or matches it must change)
STAGE_FLIPS = [
    ("strict", False, "candidate_order"),              # >= for > in the best-candidate test: the far one of two equal totals
    ("cap", 5, "rate_below_min"),                      # five splits per 64 positions
    ("nearest_first", False, "candidate_order"),       # oldest-first candidates
    ("anchor_fwd", False, "block_end_and_whole_block"),  # the anchor left at the split (w + forward is the match's end: see below)
    ("frame_restart", False, "span_120k_min4"),        # the hash of a frame's first positions warmed up on the frame in front
    ("window_in_frame", False, "span_120k_min16"),     # windows that straddle a frame start
    ("min_on_fwd", False, "forward_short_total_long"),  # minMatch asked of the total, not of the forward part
    ("insert_unsearched", False, "near_end_candidate"),  # a split too close to its block's end is not inserted
    ("check_filter", False, "key_bits_0"),             # candidates of another checksum are compared too (same result wanted: see below)
]


@pytest.mark.parametrize("rule,value,name", STAGE_FLIPS, ids=[f[0] for f in STAGE_FLIPS])
def test_single_rule_flips_change_a_named_case(rule, value, name):
    lay, p, buf, S, M, _ = staged(name)
    S2, M2, _ = lm.stage(buf, lay, p, rules={rule: value})
    if rule == "check_filter":
        # the checksum only saves compares: candidates are verified by bytes, so dropping the filter must NOT change a match
        assert (S2, M2) == (S, M)
        return
    assert (S2, M2) != (S, M), "the flipped rule gives the same result: the case does not see it"


MERGE_FLIPS = [("floor", 3, 7), ("floor", 5, 8), ("tie_le", False, 10)]


@pytest.mark.parametrize("rule,value,i", MERGE_FLIPS, ids=["floor-3", "floor-5", "tie-lt"])
def test_single_rule_flips_change_a_merge(rule, value, i):
    F, L, n, _ = SYNTH[i]
    try:
        flipped = lm.merge(F, L, n, rules={rule: value})[:2]
    except RuntimeError:
        return                  # (`<` for `<=`: a finder match that starts where a long-distance match does is never passed)
    assert flipped != lm.merge(F, L, n)[:2]
