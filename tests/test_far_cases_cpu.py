"""The far-offset frames of tests/far_cases.py on the CPU: the oracle decodes every valid one to the bytes of the forge's own executor
and refuses the invalid one — so what tests/test_gpu_far_offsets.py holds the GPU decoder to is the format's, twice over.  (A case
regenerates 512 MiB, one of them 1 GiB: each is built, checked and dropped.)"""
import pytest

import far_cases


@pytest.mark.parametrize("name", far_cases.VALID)
def test_oracle_decodes_what_the_executor_regenerates(oracle, name):
    c = far_cases.build(name, keep_content=True)
    content = c["content"]
    assert len(content) == c["size"] and c["size"] > far_cases.FAR and c["below_1g"] == (c["size"] < (1 << 30))
    got = oracle.decompress(c["blob"], c["cap"], c["dict"])
    assert not isinstance(got, int), got
    assert got == content
    del got
    # the compact form the GPU test compares on the device: seed, zeros, tail — and a tail that is not zeros (a far match that lost
    # an offset bit would copy the fill)
    assert c["head"] == far_cases.seed_block() and content[:far_cases.SEED_BYTES] == c["head"] and content[c["tail_off"]:] == c["tail"]
    assert content.count(0, far_cases.SEED_BYTES, c["tail_off"]) == c["tail_off"] - far_cases.SEED_BYTES
    assert c["tail"].count(0) * 10 < len(c["tail"]) and len(c["tail"]) >= 200       # (a near match next to the fill may copy a few zeros)


@pytest.mark.parametrize("name", far_cases.INVALID)
def test_oracle_refuses_the_invalid_case(oracle, name):
    c = far_cases.build(name)
    assert not c["valid"] and c["cap"] > far_cases.FAR
    got = oracle.decompress(c["blob"], c["cap"])
    assert got == -20, got          # corruption_detected


def test_the_cases_state_the_offsets_they_are_named_for():
    seqs = lambda d: [s for b in d["blocks"] if b["t"] == "c" for s in b["seqs"]]
    far = lambda d: [s[1] - 3 for s in seqs(d) if s[1] - 3 >= far_cases.FAR]
    assert [s[1] - 3 for s in seqs(far_cases.CASES["last_packed_offset"]())][0] == far_cases.FAR - 1 and not far(far_cases.CASES["last_packed_offset"]())
    assert far(far_cases.CASES["first_far_offset"]()) == [far_cases.FAR]
    assert far(far_cases.CASES["code29"]()) == [536874913] and (536874913 + 3).bit_length() - 1 == 29
    assert far(far_cases.CASES["code30_walk"]()) == [1073745735] and (1073745735 + 3).bit_length() - 1 == 30
    alt = seqs(far_cases.CASES["alternating_130"]())
    assert len(alt) == 130 and len(far(far_cases.CASES["alternating_130"]())) == 65 and alt[71][1] == 1
    assert all(n in far_cases.VALID for n in far_cases.NEEDS_FAR) and len(far_cases.VALID) == 9
