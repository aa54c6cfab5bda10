"""No-GPU tests of the gene-level count of BUS records: the CPU build of kamd_busgenes.h (tests/emu_busgenes) against the restatement over Python
sets (tests/bus_genes_common.py), the transcripts-to-genes parser of kallisto_amd.api, and the floors of the golden cases the GPU tests lean on.
Integers only: every comparison is exact."""
import numpy as np
import pytest

from tests import bus_genes_common as G
from tests import bus_sc_common as B
from tests import common


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# gene lists
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.GRID_MAPS)
def test_gene_lists_equal_the_restatement(name):
    sets = G.grid_sets()
    assert sorted({len(s) for s in sets}) == [0] + list(G.GRID_SIZES)
    tr_gene, _ = G.grid_map(name)
    want = G.py_gene_lists(tr_gene, sets)
    off, ids = G.emu_lists(tr_gene, sets)
    assert G.lists_of_csr(off, ids) == want
    assert int(off[-1]) == len(ids) == sum(len(x) for x in want)
    # the maps do what they are there for
    big = want[len(G.GRID_SIZES) - 1]   # the class of 5000 consecutive transcripts
    if name == "zero":
        assert big == [0]
    elif name == "identity":
        assert len(big) == 5000
    elif name == "mod7":
        assert big == list(range(7))
    elif name == "none":
        assert all(x == [] for x in want)
    elif name == "mod7_holes":
        assert big == [0, 1, 2, 4, 5, 6]
    elif name == "identity_holes":
        assert len(big) == 5000 - len([t for t in sets[len(G.GRID_SIZES) - 1] if t % 7 == 3])


def test_gene_lists_of_unsorted_sets_with_repeats():
    """the CSR need not be sorted or distinct for the lists to be"""
    tr_gene = np.array([5, 1, -1, 1, 0, 5, 3], np.int32)
    sets = [[6, 0, 5, 0], [2], [3, 1, 4, 2], []]
    off, ids = G.emu_lists(tr_gene, sets)
    assert G.lists_of_csr(off, ids) == [[3, 5], [], [0, 1], []] == G.py_gene_lists(tr_gene, sets)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the rule of a group
# ---------------------------------------------------------------------------------------------------------------------------------------------------
LISTS = [[3], [], [3, 4], [4, 9], [1, 3, 4, 9], [7]]   # class -> gene list


@pytest.mark.parametrize("classes,want", [
    ([0], 3), ([1], G.NONE), ([2], G.MULTI),                                  # one class: one gene, none, several
    ([2, 3], 4), ([0, 5], G.NONE), ([2, 4], G.MULTI),                         # several classes: one gene left, none, several
    ([0, 1], G.NONE), ([4, 3, 2], 4), ([4, 4], G.MULTI), ([0, 0, 0], 3),      # an empty list among them; three classes; a class named twice
    ([3, 4, 3, 4], G.MULTI), ([2, 3, 2, 3, 2], 4),
])
def test_group_rule(classes, want):
    assert G.py_group_gene(LISTS, classes) == want
    assert G.emu_group(LISTS, classes) == want


def _hand_records():
    """barcode 10: six groups, one of each outcome; barcode 20: an uncollapsed group with duplicate classes and flags, a counted group for gene 4
    again; barcode 30: nothing counted"""
    rows = [(10, 1, 0), (10, 2, 1), (10, 3, 2), (10, 4, 2), (10, 4, 3), (10, 5, 0), (10, 5, 5), (10, 6, 2), (10, 6, 4),
            (20, 1, 2), (20, 1, 2), (20, 1, 3), (20, 1, 3), (20, 2, 3), (20, 2, 2), (20, 9, 0),
            (30, 1, 1), (30, 2, 4)]
    b, u, e = zip(*rows)
    rec = G.make_records(b, u, e, flags=np.arange(len(rows)) % 3, count=np.arange(len(rows)) + 1)
    return G.np_sort(rec)


def test_count_on_hand_built_groups():
    rec = _hand_records()
    rc, bc, en, st = G.emu_count(LISTS, rec, G.UMIS)
    assert rc == 0
    want = G.assert_gene_count_is_the_restatement(rec, G.UMIS, LISTS, bc, en, st)
    assert want["barcodes"] == [10, 20, 30]
    assert want["entries"] == {(0, 3): 1, (0, 4): 1, (1, 4): 2, (1, 3): 1}
    assert (st["n_umis"], st["n_counted"], st["n_no_gene"], st["n_multi_gene"]) == (11, 5, 3, 3)
    assert G.py_outcomes(G.rec_tuples(rec), LISTS) == dict(single_one=2, single_none=2, single_multi=2, multi_one=3, multi_none=1, multi_multi=1)


def test_count_reads_mode():
    rec = _hand_records()
    rc, bc, en, st = G.emu_count(LISTS, rec, G.READS)
    assert rc == 0
    want = G.assert_gene_count_is_the_restatement(rec, G.READS, LISTS, bc, en, st)
    assert st["n_umis"] == len(rec) and st["n_wave_groups"] == 0
    by_class = {e: int(rec["count"][rec["ec"] == e].sum()) for e in (0, 5)}   # the classes with one gene: 0 -> gene 3, 5 -> gene 7
    assert sum(v for (r, g), v in want["entries"].items() if g == 3) == by_class[0] and sum(v for (r, g), v in want["entries"].items() if g == 7) == by_class[5]
    assert st["n_counted"] == int(np.isin(rec["ec"], (0, 5)).sum()) and st["n_no_gene"] == int((rec["ec"] == 1).sum())


def test_count_errors():
    rec = _hand_records()
    bad = rec.copy()
    bad["ec"][7] = len(LISTS)
    assert G.emu_count(LISTS, G.np_sort(bad), G.UMIS)[0] == 1
    bad["ec"][7] = -1
    assert G.emu_count(LISTS, G.np_sort(bad), G.READS)[0] == 1
    swapped = rec.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert G.emu_count(LISTS, swapped, G.UMIS)[0] == 2
    big = G.make_records([1, 1, 1], [1, 2, 3], [0, 0, 0], count=[0xFFFFFFFF, 1, 5])
    assert G.emu_count(LISTS, big, G.READS)[0] == 3
    assert G.emu_count(LISTS, big, G.UMIS)[0] == 0   # (UMIS counts groups, not reads)
    rc, bc, en, st = G.emu_count(LISTS, rec[:0], G.UMIS)
    assert rc == 0 and len(bc) == 0 and len(en) == 0 and st["n_umis"] == 0


def test_thresholds_decide_the_wave_groups():
    mr, ml = G.thresholds()
    assert mr >= 2 and ml >= 1
    lists = [list(range(k)) for k in range(ml + 3)]   # class k: a list of k genes
    groups = [[ml, ml], [ml + 1, ml + 1], [ml + 1, ml + 2], [ml + 1] * mr, [1] * mr, [1] * (mr + 1), [ml + 2], [0, ml + 2]]
    b = [1] * sum(len(g) for g in groups)
    u = [i for i, g in enumerate(groups) for _ in g]
    rec = G.np_sort(G.make_records(b, u, [c for g in groups for c in g], flags=np.arange(len(b))))
    rc, bc, en, st = G.emu_count(lists, rec, G.UMIS)
    assert rc == 0
    G.assert_gene_count_is_the_restatement(rec, G.UMIS, lists, bc, en, st)
    assert st["n_wave_groups"] == G.py_wave_groups(G.rec_tuples(rec), lists, mr, ml) == 4


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the parser
# ---------------------------------------------------------------------------------------------------------------------------------------------------
NAMES = ["tA", "tB", "tC", "tB", "tD"]   # (tB twice: the first wins)


def _map(tmp_path, text):
    p = tmp_path / "t2g.txt"
    p.write_text(text)
    return str(p)


def test_genemap_good_files(tmp_path):
    from kallisto_amd import api as A
    tr, names, common_names = A.genemap_read(_map(tmp_path, "tC gX  GeneX\ntA\tgY\n\ntB gX ignored extra\n"), NAMES)
    assert tr.dtype == np.int32 and tr.tolist() == [1, 0, 0, -1, -1]
    assert names == ["gX", "gY"] and common_names == ["GeneX", ""]       # numbered by first appearance; the common name of the first line
    tr, names, _ = A.genemap_read(_map(tmp_path, "tA g1\ntA g2\ntD g1\n"), NAMES)   # a transcript named twice: the last line wins
    assert tr.tolist() == [1, -1, -1, -1, 0] and names == ["g1", "g2"]
    tr, names, _ = A.genemap_read(_map(tmp_path, ""), NAMES)
    assert tr.tolist() == [-1] * 5 and names == []


def test_genemap_errors(tmp_path):
    from kallisto_amd import api as A
    p = _map(tmp_path, "tA g1\ntB\n")
    with pytest.raises(A.KallistoAmdError) as e:
        A.genemap_read(p, NAMES)
    assert str(e.value) == "Error: No gene associated with transcript tB in " + p
    p = _map(tmp_path, "tA g1\ntZ g2\n")
    with pytest.raises(A.KallistoAmdError) as e:
        A.genemap_read(p, NAMES)
    assert str(e.value) == "Error: Invalid transcript: tZ in " + p
    with pytest.raises(A.KallistoAmdError, match="could not open file"):
        A.genemap_read(str(tmp_path / "missing.txt"), NAMES)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the golden cases hold every outcome
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def golden_records(name):
    """the reference's records of a case -> (sets: the distinct transcript sets in sorted order, recs: (barcode, umi, class, 1) per line, n_targets)"""
    from kallisto_amd import api as A
    _, lines = B.load_golden(name)
    _, idx, _, _ = common.load_case(B.CASES[name]["fixture"])
    n_targets = int(A.Index(idx).num_targets)
    sets = sorted({l[3] for l in lines})
    cid = {s: i for i, s in enumerate(sets)}
    return sets, [(bc, umi, cid[s], 1) for _, bc, umi, s in lines], n_targets


def test_goldens_hold_every_outcome():
    seen = dict.fromkeys(G.OUTCOMES, 0)
    per = {}
    for name in B.golden_cases():
        sets, recs, n_targets = golden_records(name)
        for holes in (False, True):
            tr_gene, _ = G.golden_map(n_targets, holes)
            out = per[(name, holes)] = G.py_outcomes(recs, G.py_gene_lists(tr_gene, sets))
            for k, v in out.items():
                seen[k] += v
        assert per[(name, True)]["single_none"] > 0, name                 # with holes every case has single-class groups without a gene
        has_umi = B.parse(B.CASES[name]["tech"])[0].parts("umi")[0][0] >= 0
        if has_umi:
            assert sum(1 for v in per[(name, True)].values() if v) >= 4, (name, per[(name, True)])
    assert all(v > 0 for v in seen.values()), seen
    t = per[("10xv3", False)]
    assert (t["single_one"], t["single_none"], t["single_multi"]) == (1623, 0, 178) and (t["multi_one"], t["multi_none"], t["multi_multi"]) == (30, 129, 0)
    assert per[("indropsv2", False)]["multi_multi"] == 44
