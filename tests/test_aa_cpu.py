"""Translated search (`bus --aa`) without a GPU: the per-item logic of kallisto_amd/csrc/kamd_aa.h compiled for the CPU (tests/emu_aa)
against a plain Python translation and against the reference's output on tests/golden/aa_bulk (tests/golden/make_aa_bulk.py)."""
import random

import numpy as np
import pytest

from tests import aa_common as A


def test_codon_table():
    """same amino acid under the standard code <=> same triplet; the three stops are masked; 20 distinct triplets"""
    t = A.emu_codon_table()
    assert len(A.CODE) == 64 and A.CODE.count("*") == 3
    for c in range(64):
        assert (t[c] == 0xFF) == (A.CODE[c] == "*"), A.codon_of(c)
        for d in range(64):
            assert (t[c] == t[d]) == (A.CODE[c] == A.CODE[d]), (A.codon_of(c), A.codon_of(d))
    assert len({int(x) for x in t if x != 0xFF}) == 20
    for c in range(64):   # (and they are the comma-free triplets of the amino acids)
        if A.CODE[c] != "*":
            assert "".join("ACGT"[(int(t[c]) >> (2 * e)) & 3] for e in range(3)) == A.CFC[A.CODE[c]]


def test_frames_match_a_plain_translation():
    reads = A.frame_test_reads(random.Random(5))
    assert {len(r) for r in reads} == set(A.FRAME_LENGTHS) and any(r.islower() for r in reads if r) and any(b"N" in r.upper() for r in reads)
    ow, ol, max_len = A.emu_frames(reads)
    got = A.unpack_frames(ow, ol, 6 * len(reads), max_len)
    for i, r in enumerate(reads):
        want = A.py_frames(r)
        assert got[6 * i:6 * i + 6] == want, r
        assert [int(x) for x in ol[6 * i:6 * i + 6]] == [3 * ((len(r) - f % 3) // 3) if len(r) >= f % 3 else 0 for f in range(6)]
    # nothing but the frame's own bits in a record: the words behind the translation are zero, the flag word says "consult the mask"
    sw = (max_len + 15) // 16 + 1
    rec = sw + (max_len + 31) // 32 + 1
    w = ow[:6 * len(reads) * rec].reshape(-1, rec)
    assert np.all(w[:, sw - 1] == 1)
    for j in range(len(w)):
        tl = int(ol[j])
        assert not np.any(w[j, (tl + 15) // 16:sw - 1]) and not np.any(w[j, sw + (tl + 31) // 32:])
        if tl % 16:
            assert int(w[j, tl // 16]) >> (2 * (tl % 16)) == 0
        if tl % 32:
            assert int(w[j, sw + tl // 32]) >> (tl % 32) == 0


def test_fixture_aims_at_the_corners():
    case = A.fixture()["case"]["variants"]
    assert case["dlist"]["emu_reads_changed_without_step1"] >= 100
    assert case["dlist"]["n_frame_clashes"] >= 100 and case["plain"]["n_frame_clashes"] >= 100
    assert case["dlist"]["emu_reads_class_list_changed_by_translated_clamp"] > 0
    assert case["dlist"]["emu_reads_early_return_before_offlist_set"] > 0


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_emulation_gives_the_reference_classes(variant):
    fx = A.fixture()
    v = fx[variant]
    e = A.emu_pseudoalign(v["index"], fx["reads"], diag=True)
    aligned = e["outcome"] >= 0
    assert e["multiset"] == v["multiset"]
    assert int(aligned.sum()) == v["run_info"]["n_pseudoaligned"]
    assert sum(n for s, n in e["multiset"].items() if len(s) == 1) == v["run_info"]["n_unique"]
    assert int(e["clashes"][aligned].sum()) == v["run_info"]["n_frame_clashes"] == v["case"]["n_frame_clashes"]
    # case.json's own numbers are this emulation's
    assert int((e["outcome"] == -1).sum()) == v["case"]["emu_rejected_offlist"]
    assert [int(x) for x in e["diag"]] == [v["case"]["emu_reads_early_return_before_offlist_set"],
                                          v["case"]["emu_reads_class_list_changed_by_translated_clamp"], v["case"]["emu_reads_changed_without_step1"]]
