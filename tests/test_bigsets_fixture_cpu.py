"""The bigsets_pe fixture (tests/golden/make_bigsets.py) on the CPU: it has the sets the GPU tests of EC resolution need -- one on each side
of every size threshold of kallisto_amd/csrc/kamd_ec.hip --, the oracle gives the reference's result on it, and the host reference of
tests/test_gpu_ec_resolve.py (tests/bigsets.py: a membership matrix) is plain set intersection."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import bigsets, common


@pytest.fixture(scope="module")
def oix(tmp_path_factory):
    return O.Index(bigsets.unpack_index(tmp_path_factory.mktemp("bigsets")))


@pytest.fixture(scope="module")
def sets(oix):
    return bigsets.sets_of_oracle_index(oix)


def test_fixture_has_the_sets_the_kernels_branch_on(sets):
    sz = sets.sizes
    with open(os.path.join(common.case_dir(bigsets.NAME), "case.json")) as f:
        meta = json.load(f)
    assert meta["set_size_histogram"] == bigsets.size_histogram(sz) and meta["n_sets"] == len(sz) and meta["largest_set"] == sz.max()
    for b in bigsets.BOUNDARY_SIZES:
        assert (sz == b).any(), f"no set of exactly {b} members"
    count = lambda lo, hi: int(((sz >= lo) & (sz <= hi)).sum())
    assert count(1025, 4096) >= 5 and count(129, 1024) >= 50 and count(65, 128) >= 50 and count(17, 64) >= 200
    # two distinct sets beyond 4096 whose intersection is neither empty nor one of them
    huge = np.flatnonzero(sz > 4096)
    assert len(huge) >= 2
    assert any(0 < len(sets.intersect([a, b])) < min(sz[a], sz[b]) for i, a in enumerate(huge) for b in huge[i + 1:])
    # 129..1024: disjoint pairs, and pairs with more than 64 common members
    mid = np.flatnonzero((sz >= 129) & (sz <= 1024))
    common_members = sets.matrix[mid].astype(np.int32) @ sets.matrix[mid].astype(np.int32).T
    off_diag = ~np.eye(len(mid), dtype=bool)
    assert (common_members[off_diag] == 0).any() and (common_members[off_diag] > 64).any()
    # what the GPU tests draw from: short lists of 65..128 members that share more than 64, and a few hundred sets of more than 16
    # members with a common transcript (a non-empty intersection of more than 256 sets)
    short = np.flatnonzero((sz >= 65) & (sz <= 128))
    cs = sets.matrix[short].astype(np.int32) @ sets.matrix[short].astype(np.int32).T
    assert (cs[~np.eye(len(short), dtype=bool)] > 64).any()
    assert sets.matrix[sz > 16].sum(axis=0).max() >= 300 > bigsets.RB_MAXSETS


def test_expected_has_classes_of_large_sets(sets):
    """the reference's own result on the fixture's reads holds an EC of more than 128 transcripts and an EC that is a proper
    intersection of two or more sets of more than 128 members (not itself one of them)"""
    exp = common.load_expected(bigsets.NAME, "pe")
    assert any(len(e) > 128 for e in exp["ecs"])
    big = np.flatnonzero(sets.sizes > 128)
    as_sets = {tuple(sets.members(e).tolist()) for e in big}
    found = False
    for ec in exp["ecs"]:
        if len(ec) < 2 or ec in as_sets:
            continue
        col = np.zeros(sets.n_targets, bool)
        col[list(ec)] = True
        holders = [e for e in big if not (col & ~sets.matrix[e]).any()]   # the large sets that hold all of the EC
        if len(holders) >= 2 and np.array_equal(sets.intersect(holders), np.flatnonzero(col)):
            found = True
            break
    assert found


@pytest.mark.parametrize("variant", ["pe", "se"])
def test_oracle_matches_reference_on_large_sets(variant, oix):
    meta, r1, r2 = bigsets.load_reads()
    o = common.parse_variant(meta["variants"][variant])
    exp = common.load_expected(bigsets.NAME, variant)
    assert oix.k == meta["k"] and np.array_equal(oix.target_lens, exp["lens"])
    buf, off, lens = O.pack_reads(common.interleave(r1, r2 if o["paired"] else None))
    res = O.process_reads(oix, O.Opts(o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"]), buf, off, lens)
    assert res.n_processed == exp["nproc"]
    assert res.multiset() == exp["ecs"]
    assert np.array_equal(res.flens, exp["flens"])
    mft = O.mean_frag_lens_trunc(res.flens) if o["fld"] == 0.0 else O.trunc_gaussian_fld(o["fld"], o["sd"])
    eff, _ = O.eff_lens(oix.target_lens, mft)
    assert np.array_equal(eff, exp["eff"])
    alpha, abz, _ = O.em_run(res.ec_off, res.ec_ids, res.counts, eff, oix.num_targets)
    common.assert_abundance_close(alpha, exp["alpha"], "alpha", rel=1e-9)
    common.assert_abundance_close(abz, exp["abz"], "alpha_before_zeroes", rel=1e-9, floor=1e-12)


def test_membership_matrix_is_set_intersection(sets):
    """the host reference of the GPU tests against Python's set algebra on 200 random tuples (sizes 1 .. 40, sets of every size class)"""
    rng = np.random.default_rng(17)
    nonempty = np.flatnonzero(sets.sizes > 0)
    by_class = [nonempty[(sets.sizes[nonempty] >= lo) & (sets.sizes[nonempty] <= hi)] for lo, hi in bigsets.SIZE_CLASSES]
    n_nonempty = 0
    for i in range(200):
        m = int(rng.integers(1, 41))
        if i % 2:   # sets with a common transcript: results that are not empty
            pool = np.flatnonzero(sets.matrix[:, int(rng.integers(0, sets.n_targets))])
        else:
            pool = np.concatenate([rng.choice(c, min(len(c), m), replace=False) for c in by_class[i % 3:]])
        es = rng.choice(pool, min(m, len(pool)), replace=False)
        want = sorted(set.intersection(*[set(sets.members(e).tolist()) for e in es]))
        got = sets.intersect(es).tolist()
        assert got == want
        n_nonempty += bool(want)
        rec = [(3, list(es))]
        assert bigsets.expected_ecs(sets, rec) == ({tuple(want): 3} if want else {})
    assert 20 < n_nonempty < 200
    # merging, zero counts and dense entries of the reference itself
    a, b = by_class[5][:2]
    both = tuple(sets.intersect([a, b]).tolist())
    assert bigsets.expected_ecs(sets, [(2, [a, b]), (5, [b, a]), (0, [a])], {int(a): 0, int(b): 7}) == {both: 7, tuple(sets.members(b).tolist()): 7}
