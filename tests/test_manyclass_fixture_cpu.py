"""The manyclass_pe fixture (tests/golden/make_manyclass.py) on the CPU: it holds the items the GPU tests of kernel A's long class lists
select by count (tests/test_gpu_class_lists.py), the oracle gives the reference's result on it under every variant, and the append-only
class list of the second pass leads to the set list of the straight-line matcher -- the CPU statement of what k_classify_long must do."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import common, emu_binding as E, manyclass as M


@pytest.fixture(scope="module")
def idx_path(tmp_path_factory):
    return M.unpack_index(tmp_path_factory.mktemp("manyclass"))


@pytest.fixture(scope="module")
def emu(idx_path):
    ix = E.EmuIndex(idx_path)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def case():
    return M.load_reads()


@pytest.fixture(scope="module")
def packed(case):
    meta, r1, r2 = case
    return E.pack(common.interleave(r1, r2), meta["max_read"]), E.pack(r1, meta["max_read"])


@pytest.fixture(scope="module")
def figures(emu, case, packed):
    """D, A, S of every item under the three ways the matcher runs, recomputed"""
    meta, r1, r2 = case
    (words, l16, max_len), (w1, l1, _) = packed
    n = len(r1)
    return {"pe": M.item_figures(emu, words, l16, n, 1, max_len), "pe_nojump": M.item_figures(emu, words, l16, n, 1, max_len, no_jump=1),
            "se": M.item_figures(emu, w1, l1, n, 0, max_len)}


def test_case_json_records_the_emulations_counts(case, figures):
    meta, r1, r2 = case
    assert meta["n"] == len(r1) == len(r2) and max(map(len, r1 + r2)) <= meta["max_read"] == 400
    for v, figs in figures.items():
        rec = meta["figures"][v]
        assert rec["D"] == [it.D for it in figs] and rec["A"] == [it.A for it in figs] and rec["S"] == [it.S for it in figs], v


def test_fixture_holds_every_count(emu, case, packed, figures):
    meta, r1, r2 = case
    words, l16, max_len = packed[0]
    oc = M.filter_outcomes(emu, words, l16, len(r1), max_len, strand=common.parse_variant(meta["variants"]["pe_fr"])["strand"])
    assert oc.tolist() == meta["filter_outcome_fr"]
    grp = M.groups(figures["pe"], oc)
    assert grp == meta["groups"]
    for name, items in grp.items():
        assert len(items) >= M.SINGLE.get(name, M.MIN_ITEMS), f"{name}: {len(items)} items"
    figs = figures["pe"]
    # ranks that cross 64 and 128: per A an item whose sets are (nearly) as many as its appended classes
    for a in M.LANE_SLOT_A:
        best = max(figs[i].S for i in grp[f"A={a}"])
        assert best == meta["largest_S_at_A"][str(a)] and best >= a - 2, (a, best)
        # ... and, separately, one that is nearly all duplicates, and one with duplicates across the 64-entry slices
        assert any(figs[i].S <= 8 for i in grp[f"A={a}"]), a
        assert a < 100 or any(figs[i].cross_slice_dup for i in grp[f"A={a}"]), a      # (a list of 65 entries has one slice to speak of)
    # the mates: one without a hit, a pair of sets that do not meet, a pair without any hit
    exp = common.load_expected(M.NAME, "pe")
    assert any(it.D > 0 and not it.both_mates for it in figs) and any(it.D == 0 for it in figs)
    assert sum(exp["ecs"].values()) < sum(it.S > 0 for it in figs)      # some mapped items' sets have an empty intersection
    # the single-end and --no-jump runs reach the long lists and the re-overflow too
    for v in ("se", "pe_nojump"):
        routes = [M.route(it) for it in figures[v]]
        assert routes.count("long") >= 20 and routes.count("straight") >= 4, v
        assert any(it.A == 192 for it in figures[v]) and any(it.A == 193 for it in figures[v]), v


@pytest.mark.parametrize("variant", ["pe", "pe_union", "pe_fr", "pe_nojump", "se"])
def test_oracle_matches_reference_on_long_class_lists(variant, case, idx_path):
    meta, r1, r2 = case
    oix = O.Index(idx_path)
    o = common.parse_variant(meta["variants"][variant])
    exp = common.load_expected(M.NAME, variant)
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


@pytest.mark.parametrize("paired,no_jump", [(1, 0), (1, 1), (0, 0)])
def test_append_mode_gives_the_straight_line_set_list(paired, no_jump, emu, case, packed):
    """emu_tuples with the append bit (the second pass's list, duplicates removed by uecs_to_ecs) against match_mate, item by item"""
    meta, r1, r2 = case
    words, l16, max_len = packed[0] if paired else packed[1]
    n = len(r1)
    nj = M.FLAG_NO_JUMP if no_jump else 0
    stride = M.TUPLE_CAP_BIG + 1
    stepper, _ = E.tuples(emu, words, l16, n, paired, max_len, M.FLAGS_APPEND | nj, stride=stride)
    assert E.tuples.last_appended == sum(meta["figures"]["pe_nojump" if no_jump else "pe" if paired else "se"]["A"])
    straight, _ = E.tuples(emu, words, l16, n, paired, max_len, nj, stride=stride)
    assert np.array_equal(stepper, straight)
    first, _ = E.tuples(emu, words, l16, n, paired, max_len, M.FLAGS_FIRST | nj, stride=stride)
    assert np.array_equal(first, straight)
    assert (straight[:, 0] != 0xFFFFFFFF).sum() > 150 and straight[straight[:, 0] != 0xFFFFFFFF, 0].max() > M.LONG_CAP


def test_ec_state_opts_is_ec_state_and_marks_the_mates(emu, case, packed):
    """the GPU tests' host reference (emu_ec_state_opts: match_mate, lists of up to 1024 sets): equal to emu_ec_state where that applies,
    and under --union the same sets with the mates' flags"""
    meta, r1, r2 = case
    words, l16, max_len = packed[0]
    figs = meta["figures"]["pe"]
    small = [i for i in range(len(r1)) if figs["S"][i] <= 60]
    sub = E.pack([x for i in small for x in (r1[i], r2[i])], max_len)
    d0, s0, o0 = E.ec_state(emu, sub[0], sub[1], len(small), 1, max_len)
    d1, s1, o1 = M.ec_state_opts(emu, words, l16, len(r1), 1, max_len, item_ids=small)
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1) and np.array_equal(o0, o1)
    du, su, ou = M.ec_state_opts(emu, words, l16, len(r1), 1, max_len, union=1)
    da, sa, oa = M.ec_state_opts(emu, words, l16, len(r1), 1, max_len)
    assert np.array_equal(du, da) and np.array_equal(ou, oa)
    body = np.ones(len(sa), bool)
    body[oa.astype(np.int64)] = body[oa.astype(np.int64) + 1] = False
    assert np.array_equal(su[~body], sa[~body]) and np.array_equal(su[body] & M.ID_MASK, sa[body])
    flags = su[body] >> 30
    assert (flags != 0).all() and (flags == 3).any() and (flags == 1).any() and (flags == 2).any()
