"""The expectations of test_gpu_fld_sample.py, held against the oracle's own walk over the reads (ko_process_reads, `tlencount < 10000`) so
that the GPU tests cannot go vacuous: expected_flens from one tile's per-pair flags is what the oracle computes on the concatenated reads,
and every named input has its 10 000th qualifying pair where the GPU tests need it."""
import numpy as np
import pytest

from tests import common
from tests import fld_sample_common as F


def _oracle_flens(inp, **opts):
    from oracle import oracle as O
    buf, off, lens = O.pack_reads(inp.reads())
    res = O.process_reads(F.oracle_index(inp.case), F.oracle_opts(**opts), buf, off, lens)
    assert res.n_processed == inp.n_items
    return res.flens


def _expected(inp, start_used=0, **opts):
    q, tls = F.pair_flags(inp.case, **opts)
    return F.expected_flens(q, tls, inp.order(), start_used)


@pytest.mark.parametrize("name,build,opts", [
    ("ref x 2, pe", lambda: F.tiled("ref_test_pe", 2), {}),
    ("ref x 4, --fr", lambda: F.tiled("ref_test_pe", 4), {"strand": 1}),
    ("ref x 4, --rf", lambda: F.tiled("ref_test_pe", 4), {"strand": 2}),
    ("ref x 4, single overhang", lambda: F.tiled("ref_test_pe", 4), {"single_overhang": 1}),
    ("cut at 16383", lambda: F.cut_at(16383), {}),
    ("dense, sparse, dense", F.dense_sparse_dense, {}),
])
def test_expected_flens_is_the_oracles_sample(name, build, opts):
    inp = build()
    flens, used = _expected(inp, **opts)
    assert used == F.WANT == flens.sum()          # each of these inputs fills the sample and goes on beyond it
    q, _ = F.pair_flags(inp.case, **opts)
    assert len(F.qualifying_positions(q, inp.order())) > F.WANT, name
    assert np.array_equal(flens, _oracle_flens(inp, **opts)), name


def test_pair_flags_are_the_fixtures_goldens():
    """one tile's flags against the reference's own sample of the fixture (expected_*.txt), for the variants the GPU tests use"""
    for case, variant, opts in [("ref_test_pe", "pe", {}), ("ref_test_pe", "pe_fr", {"strand": 1}), ("ref_test_pe", "pe_rf", {"strand": 2}),
                                ("human_pe", "pe", {}), ("dlist_pe", "pe", {}), ("dlist_pe", "pe_union", {"union": 1})]:
        q, tls = F.pair_flags(case, **opts)
        flens, used = F.expected_flens(q, tls, np.arange(len(q)))
        assert used == q.sum() < F.WANT
        assert np.array_equal(flens, common.load_expected(case, variant)["flens"]), (case, variant)
    assert F.pair_flags("ref_test_pe")[0].sum() == 6429
    assert F.pair_flags("ref_test_pe", strand=2)[0].sum() == 3296 and F.pair_flags("ref_test_pe", strand=1)[0].sum() == 3133
    assert F.pair_flags("human_pe")[0].sum() == 36 and F.pair_flags("dlist_pe")[0].sum() == 11


def test_where_the_cut_falls():
    q, _ = F.pair_flags("ref_test_pe")
    pos = F.qualifying_positions(q, F.tiled("ref_test_pe", 2).order())
    assert len(pos) == 2 * 6429 and pos[F.WANT - 1] == 15602
    for item in (16383, 16384, 16895, 16896, 16900):
        inp = F.cut_at(item)
        p = F.qualifying_positions(q, inp.order())
        assert p[F.WANT - 1] == item and len(p) == 2 * 6429 and inp.n_items == 20000 + item - 15602
        # ... and as a batch that ends with that pair
        last = inp.prefix(item + 1)
        assert last.n_items == item + 1 and np.array_equal(last.order(), inp.order()[:item + 1])
    # the junk pairs do not qualify, by the oracle itself (not only by construction)
    ix, (j1, j2) = F.oracle_index("ref_test_pe"), F.cut_at(16383).junk_read()
    u, n1, n2 = ix.pseudoalign(F.oracle_opts(), j1, j2)
    assert len(u) == 0 and n1 == 0 and n2 == 0


@pytest.mark.parametrize("nq", [9999, 10000, 10001])
def test_prefix_with_has_that_many(nq):
    q, tls = F.pair_flags("ref_test_pe")
    inp = F.prefix_with(nq)
    o = inp.order()
    pos = F.qualifying_positions(q, o)
    assert len(pos) == nq and pos[-1] == len(o) - 1       # exactly nq, and no shorter prefix has them
    flens, used = F.expected_flens(q, tls, o)
    assert used == min(nq, F.WANT) == flens.sum()
    assert np.array_equal(flens, _oracle_flens(inp))


def test_input_slicing_agrees_with_its_reads():
    """prefix / window / reads / order describe the same input"""
    inp = F.cut_at(16900)
    _, r1, r2 = F.case_reads("ref_test_pe")
    reads, o = inp.reads(), inp.order()
    assert len(reads) == 2 * inp.n_items == 2 * len(o)
    j1, j2 = inp.junk_read()
    for i in (0, F.JUNK_AT - 1, F.JUNK_AT, F.JUNK_AT + 1297, F.JUNK_AT + 1298, 11297, 11298, inp.n_items - 1):
        want = (j1, j2) if o[i] < 0 else (r1[o[i]], r2[o[i]])
        assert (reads[2 * i], reads[2 * i + 1]) == want, i
    for lo, hi in ((0, 1), (1, 5000), (5000, 5000), (5000, 16901), (16901, inp.n_items)):
        w = inp.window(lo, hi)
        assert np.array_equal(w.order(), o[lo:hi]) and w.reads() == reads[2 * lo:2 * hi]
    assert np.array_equal(inp.prefix(12345).order(), o[:12345])
    assert np.array_equal(F.tiled("human_pe", 300).prefix(F.FIRST_CHUNK).order(), F.tiled("human_pe", 300).order()[:F.FIRST_CHUNK])


def test_sample_carried_over_batches_adds_up():
    """expected_flens with start_used: the sample of ragged batches, carried, is the sample of the whole input"""
    q, tls = F.pair_flags("ref_test_pe")
    inp = F.tiled("ref_test_pe", 2)
    whole, used_whole = F.expected_flens(q, tls, inp.order())
    flens, used = np.zeros(common.MAX_FRAG_LEN, np.uint32), 0
    for lo, hi in ((0, 3), (3, 3), (3, 9000), (9000, 15602), (15602, 15603), (15603, 20000)):
        f, used = F.expected_flens(q, tls, inp.window(lo, hi).order(), used)
        flens += f
    assert used == used_whole == F.WANT and np.array_equal(flens, whole)


def test_sparse_input_needs_a_second_prefix():
    """human_pe x 300: fewer than 10 000 qualifying pairs among the first 1 048 576 items, more than 10 000 in all"""
    q, _ = F.pair_flags("human_pe")
    inp = F.tiled("human_pe", 300)
    pos = F.qualifying_positions(q, inp.order())
    assert inp.n_items == 1500000
    assert np.count_nonzero(pos < F.FIRST_CHUNK) < F.WANT < len(pos)
    assert len(F.prefixes_that_run(inp.n_items, pos)) >= 2


def test_overflow_input_is_cut_inside_a_later_prefix():
    """dlist_pe x 1000: 11 000 qualifying pairs in 4.5 M; with the first prefix the GPU test sets, the 10 000th falls in a later prefix that
    holds whole tiles (so pairs with two classes, which overflow a list of one entry) and has qualifying pairs beyond the cut"""
    q, _ = F.pair_flags("dlist_pe")
    inp = F.tiled("dlist_pe", 1000)
    pos = F.qualifying_positions(q, inp.order())
    assert len(pos) == 11000 > F.WANT
    runs = F.prefixes_that_run(inp.n_items, pos, first_chunk=65536)
    first, n = runs[-1]
    assert len(runs) >= 2 and first <= pos[F.WANT - 1] < first + n
    assert n >= 2 * len(q)                                                    # at least one whole tile inside
    assert np.count_nonzero((pos >= first) & (pos < first + n)) > F.WANT - np.count_nonzero(pos < first)   # the host loop has to stop by itself
