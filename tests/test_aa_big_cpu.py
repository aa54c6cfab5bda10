"""The workloads of tests/aa_big.py without a GPU: the frames of reads of up to 65 535 bases against a plain Python translation, aa_big.expected_for
against the fixture's own numbers, and the conditions the workloads must meet to reach the paths tests/test_gpu_aa_big.py is about."""
import numpy as np
import pytest

from tests import aa_big as B
from tests import aa_common as A


def test_long_frames_match_a_plain_translation():
    groups = B.emulated_frames_long()
    assert [sorted({len(r) for r in reads}) for ml, reads, ow, ol in groups] == B.FRAME_LENGTHS_LONG
    for max_len, reads, ow, ol in groups:
        assert max_len == max(len(r) for r in reads) and any(r.islower() for r in reads) and any(b"N" in r.upper() for r in reads)
        got = B.unpack_frames_np(ow, ol, 6 * len(reads), max_len)
        for i, r in enumerate(reads):
            assert got[6 * i:6 * i + 6] == A.py_frames(r), (len(r), i)
            assert [int(x) for x in ol[6 * i:6 * i + 6]] == [3 * ((len(r) - f % 3) // 3) for f in range(6)]
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


def test_the_fast_unpacking_is_the_plain_one():
    reads = A.frame_test_reads(__import__("random").Random(5))
    ow, ol, max_len = A.emu_frames(reads)
    assert B.unpack_frames_np(ow, ol, 6 * len(reads), max_len) == A.unpack_frames(ow, ol, 6 * len(reads), max_len)


def _stats_of_fixture(v):
    ri = v["run_info"]
    return {"n_processed": ri["n_processed"], "n_pseudoaligned": ri["n_pseudoaligned"], "n_unique": ri["n_unique"], "n_frame_clashes": ri["n_frame_clashes"],
            "n_rejected_offlist": v["case"]["emu_rejected_offlist"]}


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_expected_for_reproduces_the_fixture(variant):
    fx = A.fixture()
    v = fx[variant]
    n = len(fx["reads"])
    e = B.emulated_fixture(variant)
    want = _stats_of_fixture(v)
    for times, order in ((1, np.arange(n)), (3, np.tile(np.arange(n), 3))):
        x = B.expected_for(e, order)
        assert x["multiset"] == {s: times * c for s, c in v["multiset"].items()}
        assert x["n_processed"] == times * want["n_processed"] == len(order)
        assert sum(x["n_winner"]) == times * want["n_pseudoaligned"] == sum(x["multiset"].values())
        assert x["n_unique"] == times * want["n_unique"]
        assert x["n_frame_clashes"] == times * want["n_frame_clashes"]
        assert x["n_rejected_offlist"] == times * want["n_rejected_offlist"]
        assert x["n_rejected_offlist"] + x["n_all_empty"] + sum(x["n_winner"]) == len(order)
    # a sub-range and a permutation of it agree; an order of one read is that read
    part = B.many_reads()[:1000]
    assert B.expected_for(e, part) == B.expected_for(e, np.sort(part))
    for i in (0, n - 1):
        x = B.expected_for(e, [i])
        assert x["multiset"] == ({e["sets"][i]: 1} if e["outcome"][i] >= 0 else {}) and x["n_processed"] == 1


def test_many_reads_go_beyond_one_chunk():
    order = B.many_reads()
    n = len(A.fixture()["reads"])
    assert len(order) > 262144 and len(order) % 8 != 0
    assert np.array_equal(np.bincount(order, minlength=n), np.full(n, B.COPIES))
    assert not np.array_equal(order, np.sort(order)) and np.array_equal(order, B.many_reads())   # shuffled, and the same every time
    # the cuts the GPU tests make fall inside groups of eight as well
    assert 100003 % 8 and 40001 % 8 and 262145 % 8


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_long_reads_meet_their_conditions(variant, capsys):
    """The largest class list of a long read, as emulated: 66 classes on either index (the fixture's own reads reach 13) -- deeper than one 64-entry row of a
    lane's slab, and that is all the 49-protein index gives a 900 nt read; the capacity handed to the kernel for these reads is 871."""
    reads = B.long_reads()
    e = B.emulated_long(variant)
    nw = B.n_whole_long_reads()
    assert nw == 196 and len(reads) == 3 * nw + B.N_FIXTURE_IN_LONG
    # (40 of the 49 proteins have 300 residues, the others 79 or 80: their reads are whole too, and shorter)
    assert max(len(r) for r in reads) == B.LONG_LEN and sum(len(r) == B.LONG_LEN for r in reads[:nw]) >= 160
    assert all(b"N" in r for r in reads[2 * nw:3 * nw]) and not any(b"N" in r for r in reads[:2 * nw])
    winners = {int(f) for f in e["outcome"][:nw]}
    assert np.all(e["outcome"][:nw] >= 0)
    assert len(winners) >= 4 and winners & {0, 1, 2} and winners & {3, 4, 5}
    deepest = int(e["list_len"][:3 * nw].max())
    with capsys.disabled():
        print("\n[%s] long reads: winners %s, clashes %d, deepest class list %d (fixture reads: %d)"
              % (variant, sorted(winners), int(e["clashes"][:nw].sum()), deepest, int(e["list_len"][3 * nw:].max())))
    assert deepest >= 64
    assert deepest == 66   # (what the docstring says)
    # any batch that holds every distinct read once has these
    x = B.expected_for(e, np.arange(len(reads)))
    assert int((e["win_sets"] > 1).sum()) >= 100 and int((e["win_sets"][:nw] > 1).sum()) >= 1   # tuple records, also at the depth of a long read
    assert x["n_rejected_offlist"] + x["n_all_empty"] >= 1
    order = B.long_batch(len(reads), 19209)
    assert len(order) == 19209 and np.all(np.bincount(order, minlength=len(reads)) >= 1)
