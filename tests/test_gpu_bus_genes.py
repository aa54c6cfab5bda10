"""BUS records to a cells x genes matrix on the GPU (kamd_bus_genes_create, kamd_bus_count_genes, `bus_sc --genecounts -g`).  The yardsticks are the
restatement over Python sets and dicts (tests/bus_genes_common.py: py_gene_lists, py_gene_count) and the reference's own records
(tests/golden/bus_sc); never the code under test.  Integers only: every comparison is exact."""
import collections
import json
import os

import numpy as np
import pytest

from tests import bus_genes_common as G
from tests import bus_sc_common as B
from tests import common

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    kallisto_amd.load_library()
    return kallisto_amd


@pytest.fixture(scope="module")
def world(ka):
    ctxs = {}

    def ctx_of(fixture):
        if fixture not in ctxs:
            _, idx, _, _ = common.load_case(fixture)
            ctx = ka.Context(0)
            ctx.upload(ka.Index(idx))
            ctxs[fixture] = ctx
        return ctxs[fixture]
    yield ctx_of
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope="module")
def ctx(world):
    return world("ref_test_pe")


def _dev(rec):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rec, G.REC).view(np.int64).reshape(-1, 4).copy()).to("cuda:0")


def _entries(t):
    return np.ascontiguousarray(t.cpu().numpy()).reshape(-1).view(G.ENTRY)


def _count(ctx, table, rec_sorted, mode):
    c = ctx.bus_count_genes(table, _dev(rec_sorted), mode)
    return c["barcodes"].cpu().numpy().view(np.uint64), _entries(c["entries"]), c["stats"]


def _table_of_lists(ctx, lists, n_genes):
    """a table whose gene lists are `lists`: the identity map, the lists as the classes' transcript sets"""
    return ctx.bus_genes(np.arange(n_genes, dtype=np.int32), n_genes, lists)


def _check(ctx, table, lists, rec_sorted, mode):
    """count on the device, twice: the restatement's rows, entries, order and counters; the thresholds' number of wave groups; the same bytes"""
    bc, en, st = _count(ctx, table, rec_sorted, mode)
    want = G.assert_gene_count_is_the_restatement(rec_sorted, mode, lists, bc, en, st)
    mr, ml = G.thresholds()
    assert st["n_wave_groups"] == (G.py_wave_groups(G.rec_tuples(rec_sorted), lists, mr, ml) if mode == G.UMIS else 0)
    bc2, en2, st2 = _count(ctx, table, rec_sorted, mode)
    assert bc.tobytes() == bc2.tobytes() and en.tobytes() == en2.tobytes()
    assert {k: v for k, v in st.items() if not k.endswith("ms")} == {k: v for k, v in st2.items() if not k.endswith("ms")}
    return want, st


class Groups:
    """records by group: add(barcode, classes) gives the group the next UMI of its barcode; flags differ from record to record, so a class named
    twice stays two records"""

    def __init__(self):
        self.b, self.u, self.e, self.next_umi = [], [], [], collections.Counter()

    def add(self, barcode, classes):
        u = self.next_umi[barcode]
        self.next_umi[barcode] += 1
        for c in classes:
            self.b.append(barcode); self.u.append(u); self.e.append(c)

    def records(self):
        n = len(self.b)
        return G.np_sort(G.make_records(self.b, self.u, self.e, flags=np.arange(n) % 5, count=1 + np.arange(n) % 3))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Context.bus_genes
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.GRID_MAPS)
def test_gene_lists_equal_the_restatement(ctx, name):
    sets = G.grid_sets()
    tr_gene, n_genes = G.grid_map(name)
    want = G.py_gene_lists(tr_gene, sets)
    t = ctx.bus_genes(tr_gene, n_genes, sets)
    off, ids = t.lists()
    assert G.lists_of_csr(off, ids) == want
    st = t.stats
    assert st["n_classes"] == len(sets) and st["n_entries_in"] == sum(len(s) for s in sets) and st["n_pairs"] == sum(len(x) for x in want) == len(ids)
    assert st["n_empty"] == sum(1 for x in want if not x) and st["max_list"] == max(len(x) for x in want) and st["n_genes"] == n_genes
    # ... and a CSR with the same content gives the same table; the statuses the lists yield in a count are the restatement's
    t2 = ctx.bus_genes(tr_gene, n_genes, G.csr_of(sets))
    off2, ids2 = t2.lists()
    assert np.array_equal(off, off2) and np.array_equal(ids, ids2)
    rec = G.np_sort(G.make_records(np.arange(len(sets)) % 3, np.arange(len(sets)), np.arange(len(sets))))
    _check(ctx, t2, want, rec, G.UMIS)
    t.free(); t2.free()
    with pytest.raises(Exception):
        t.lists()


def test_gene_table_refusals_and_edges(ctx, ka):
    tr = np.array([0, 1, -1, 2], np.int32)
    for bad_tr, n_genes, sets, why in ((np.array([0, 3], np.int32), 3, [[0]], "gene 3"), (np.array([0, -2], np.int32), 3, [[0]], "gene -2"), (tr, 3, [[0, 4]], "names transcript 4")):
        with pytest.raises(ka.KallistoAmdError, match=why):
            ctx.bus_genes(bad_tr, n_genes, sets)
    with pytest.raises(ka.KallistoAmdError, match="decrease"):
        ctx.bus_genes(tr, 3, (np.array([0, 2, 1], np.uint64), np.array([0, 1], np.uint32)))
    t = ctx.bus_genes(tr, 3, [])                       # no classes at all
    assert t.stats["n_classes"] == 0 and t.stats["n_pairs"] == 0 and t.lists()[0].tolist() == [0]
    with pytest.raises(ka.KallistoAmdError, match="outside the table"):
        ctx.bus_count_genes(t, _dev(G.make_records([1], [1], [0])), G.UMIS)
    t = ctx.bus_genes(tr, 3, [[2], [], [2, 2]])        # no entry has a gene
    assert t.stats["n_pairs"] == 0 and t.stats["n_empty"] == 3 and t.stats["max_list"] == 0 and t.lists()[0].tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Context.bus_count_genes against py_gene_count
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _two_lists(s, o, k, where, base):
    """list A of s genes and list B of o genes that share exactly k genes, at the `where` (first / middle / last) of A; None where o < k or s < k"""
    a = [base + 3 * j for j in range(s)]
    if k > s or k > o or (k == 2 and s < 2):
        return None
    pos = {"first": [0, 1], "middle": [s // 2, s // 2 - 1 if s // 2 else 1], "last": [s - 1, s - 2]}[where][:k]
    if len(set(pos)) < k or any(p < 0 or p >= s for p in pos):
        return None
    shared = [a[p] for p in pos]
    filler = [base + 3 * j + 1 for j in range(o - k)]   # (no member of A)
    return a, sorted(shared + filler)


SMALLEST = lambda ml: (1, ml, ml + 1, 63, 64, 65, 129, 1000)
OTHERS = (1, 2, 3, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def shapes(ctx):
    """every smallest-list size x every other-list size x 0 / 1 / 2 survivors x the survivor first / middle / last in its list: groups of two and of
    three records, one table"""
    mr, ml = G.thresholds()
    lists, gr, kinds = [], Groups(), collections.Counter()
    for s in SMALLEST(ml):
        for o in OTHERS:
            for k in (0, 1, 2):
                for where in (("first",) if k == 0 else ("first", "middle", "last")):
                    ab = _two_lists(s, o, k, where, 0)
                    if ab is None:
                        continue
                    ia = len(lists)
                    lists += [ab[0], ab[1], sorted(set(ab[1]) | {5000, 5001})]
                    gr.add(len(lists) % 7, [ia, ia + 1])
                    gr.add(len(lists) % 5, [ia + 1, ia + 2, ia] if len(lists) % 2 else [ia + 2, ia, ia + 1])
                    kinds[(min(s, o) > ml, k)] += 1
    rec = gr.records()
    return ctx, _table_of_lists(ctx, lists, 6000), lists, rec, kinds


def test_list_sizes_and_survivors(shapes):
    ctx, table, lists, rec, kinds = shapes
    assert all(kinds[(wave, k)] > 0 for wave in (False, True) for k in (0, 1, 2))   # both kernels see zero, one and two survivors
    want, st = _check(ctx, table, lists, rec, G.UMIS)
    assert 0 < st["n_wave_groups"] < st["n_umis"] and st["n_counted"] and st["n_no_gene"] and st["n_multi_gene"]
    _check(ctx, table, lists, rec, G.READS)


def _sized_groups():
    """groups of 1, 2, MAX_RECORDS, MAX_RECORDS + 1, 64 and 65 records of distinct classes: counted (one shared gene), none (one record lacks it),
    multi (two shared genes), and the same with every class named twice"""
    mr, _ = G.thresholds()
    lists, gr = [], Groups()
    for m in (1, 2, mr, mr + 1, 64, 65):
        for kind in ("one", "none", "multi"):
            for twice in (False, True):
                ids = []
                for k in range(m):
                    x = [7] + ([100 + len(lists)] if m > 1 else []) + ([8] if kind == "multi" else [])   # (a gene of its own: the classes differ)
                    if kind == "none" and k == m - 1:
                        x = [100 + len(lists)] if m > 1 else []
                    ids.append(len(lists))
                    lists.append(sorted(x))
                gr.add(m % 3, ids * 2 if twice else ids)
    return lists, gr.records()


def test_group_sizes(ctx):
    lists, rec = _sized_groups()
    table = _table_of_lists(ctx, lists, 100 + len(lists))
    want, st = _check(ctx, table, lists, rec, G.UMIS)
    assert st["n_counted"] == st["n_no_gene"] == st["n_multi_gene"] == 12
    _check(ctx, table, lists, rec, G.READS)


def test_a_group_of_70000_classes_that_share_one_gene(ctx):
    m = 70000
    tr_gene = np.concatenate([1 + np.arange(m) % 50, [0]]).astype(np.int32)
    sets = [[k, m] for k in range(m)] + [[m], [3]]
    lists = G.py_gene_lists(tr_gene, sets)
    table = ctx.bus_genes(tr_gene, 51, sets)
    assert table.stats["n_pairs"] == 2 * m + 2 and table.stats["max_list"] == 2
    gr = Groups()
    gr.add(1, [m])                       # gene 0, counted by a thread
    gr.add(2, list(range(m)))            # the big group: gene 0
    gr.add(2, list(range(0, m, 2)) + [m + 1])   # ... and one that ends in a class without it: no gene
    gr.add(3, [m + 1, 2])                # gene 4 (class 2: genes 0, 3; class m + 1: gene 4) -> none
    rec = gr.records()
    want, st = _check(ctx, table, lists, rec, G.UMIS)
    assert want["entries"] == {(0, 0): 1, (1, 0): 1} and st["n_wave_groups"] == 2 and st["n_no_gene"] == 2


def _random_case(n, seed):
    rnd = np.random.RandomState(seed)
    n_genes, n_classes = 500, 3000
    lens = rnd.choice([0, 1, 1, 1, 2, 2, 3, 5, 9, 12, 40, 130], n_classes)
    lists = [sorted(rnd.choice(n_genes, l, replace=False).tolist()) for l in lens]
    # classes that share genes: neighbours in id get the genes of their predecessor too, now and then
    for c in range(1, n_classes, 3):
        lists[c] = sorted(set(lists[c]) | set(lists[c - 1][:2]))
    b = rnd.randint(0, 2000, n).astype(np.uint64) * np.uint64(0x100000001)
    u = rnd.randint(0, 40, n)
    e = (rnd.randint(0, 30, n) + 29 * (b % np.uint64(97)).astype(np.int64) + u) % n_classes   # a group's classes lie close together
    rec = G.make_records(b, u, e, flags=rnd.randint(0, 3, n), count=rnd.randint(1, 4, n))
    return lists, n_genes, G.np_sort(rec)


@pytest.fixture(scope="module")
def boundary_case(ctx):
    """records 0 .. 262: single-record groups, but for one group of 13 records that lies on records 250 .. 262"""
    mr, ml = G.thresholds()
    lists = [[1], [2], [1, 2], []] + [[9, 20 + k] for k in range(13)]
    gr = Groups()
    for i in range(250):
        gr.add(i // 50, [i % 4])
    gr.add(9, list(range(4, 17)))
    rec = gr.records()
    assert len(rec) == 263 and len(set(rec["umi"][250:].tolist())) == 1 and rec["barcode"][249] != rec["barcode"][250]
    return _table_of_lists(ctx, lists, 40), lists, rec


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 263])
def test_small_inputs_and_a_group_across_a_block_boundary(ctx, boundary_case, n):
    table, lists, rec = boundary_case
    want, st = _check(ctx, table, lists, rec[:n], G.UMIS)
    if n > 251:
        assert st["n_wave_groups"] == 1 and (5, 9) in want["entries"]
    _check(ctx, table, lists, rec[:n], G.READS)


def test_263378_records(ctx):
    lists, n_genes, rec = _random_case(263378, 5)
    table = _table_of_lists(ctx, lists, n_genes)
    want, st = _check(ctx, table, lists, rec, G.UMIS)
    assert st["n_wave_groups"] > 100 and min(st["n_counted"], st["n_no_gene"], st["n_multi_gene"]) > 100
    _check(ctx, table, lists, rec, G.READS)


@pytest.mark.parametrize("what", ["all", "none", "first", "last"])
def test_mixtures(ctx, what):
    lists = [[4], [], [4, 5], [5]]
    table = _table_of_lists(ctx, lists, 6)
    n = 700
    gr = Groups()
    for i in range(n):
        good = what == "all" or (what == "first" and i == 0) or (what == "last" and i == n - 1)
        gr.add(i // 100, ([0], [0, 2], [2, 3])[i % 3] if good else ([1], [0, 3], [2], [2, 2])[i % 4])
    rec = gr.records()
    want, st = _check(ctx, table, lists, rec, G.UMIS)
    assert st["n_counted"] == {"all": n, "none": 0, "first": 1, "last": 1}[what]
    assert st["n_entries"] == len(want["entries"]) and (what != "none" or st["n_entries"] == 0)
    if what in ("first", "last"):
        assert list(want["entries"]) == [(0 if what == "first" else 6, 4)]


def _raw(ka, ctx, table_handle, rec, mode):
    """the C call on outputs filled with -1 -> (rc, error text, outputs untouched)"""
    import torch
    C = ka.api.C
    d = _dev(rec)
    bc = torch.full((len(rec),), -1, dtype=torch.int64, device="cuda:0")
    en = torch.full((len(rec), 3), -1, dtype=torch.int32, device="cuda:0")
    rc = ka.load_library().kamd_bus_count_genes(ctx._h, table_handle, d.data_ptr(), len(rec), mode, bc.data_ptr(), en.data_ptr(), None)
    return rc, ka.load_library().kamd_last_error().decode(), bool((bc == -1).all()) and bool((en == -1).all())


def test_errors(ka, ctx):
    mr, ml = G.thresholds()
    lists = [[1], [1, 2], [2]]
    table = _table_of_lists(ctx, lists, 3)
    gr = Groups()
    for i in range(600):
        gr.add(i // 64, [i % 3])
    gr.add(99, [0, 1] * (mr + 3))   # a group a wavefront settles
    rec = gr.records()
    _check(ctx, table, lists, rec, G.UMIS)
    big = len(rec) - 2
    for mode in (G.UMIS, G.READS):
        for at, cls in ((300, 3), (300, -1), (0, 1 << 30), (big, 3), (big, -7)):   # single-record groups, and inside the wavefront's group
            bad = rec.copy()
            bad["ec"][at] = cls
            bad = G.np_sort(bad)
            rc, text, untouched = _raw(ka, ctx, table._h, bad, mode)
            assert rc == -4 and "outside the table's [0, 3)" in text and untouched, (mode, at, cls)
        swapped = rec.copy()
        swapped[[10, 400]] = swapped[[400, 10]]
        rc, text, untouched = _raw(ka, ctx, table._h, swapped, mode)
        assert rc == -4 and "lie before their predecessor in key order: the input is not sorted; nothing counted" in text and untouched
    with pytest.raises(ka.KallistoAmdError, match="not sorted"):
        ctx.bus_count_genes(table, _dev(swapped), G.UMIS)
    # a value above 32 bits: READS mode only (UMIS counts groups)
    over = G.make_records([1, 1, 2], [1, 2, 1], [0, 0, 2], count=[0xFFFFFFFF, 1, 5])
    rc, text, untouched = _raw(ka, ctx, table._h, over, G.READS)
    assert rc == -4 and "0xFFFFFFFF" in text and untouched
    assert _raw(ka, ctx, table._h, over, G.UMIS)[0] == 0
    # a foreign table, a freed table
    other = ka.Context(0)
    try:
        foreign = other.bus_genes(np.arange(3, dtype=np.int32), 3, lists)
        with pytest.raises(ka.KallistoAmdError, match="not a .* gene table of this context"):
            ctx.bus_count_genes(foreign, _dev(rec), G.UMIS)
        rc, text, untouched = _raw(ka, ctx, foreign._h, rec, G.UMIS)
        assert rc == -1 and "not a gene table of this context" in text and untouched
    finally:
        other.close()
    table.free()
    with pytest.raises(ka.KallistoAmdError, match="not a .* gene table of this context"):
        ctx.bus_count_genes(table, _dev(rec), G.UMIS)
    with pytest.raises(ka.KallistoAmdError, match="mode must be"):
        ctx.bus_count_genes(_table_of_lists(ctx, lists, 3), _dev(rec), 2)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the EC state, the golden cases, the driver
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_gene_calls_leave_the_ec_state_alone(ka, world):
    from tests.test_gpu_bus_sort import _batch, _host, _same_ecs
    ctx = world("ref_test_pe")
    lists, rec = _sized_groups()

    def both():
        t = _table_of_lists(ctx, lists, 100 + len(lists))
        _count(ctx, t, rec, G.UMIS)
        _count(ctx, t, rec, G.READS)
        t.free()
    _, _, plain, _ = _batch(ka, ctx, "10xv3")
    d_rec, sets, ecs, _ = _batch(ka, ctx, "10xv3", between=both, behind=both)   # between the batch and its finalize, and behind it
    assert ecs.multiset() == plain.multiset()
    assert _same_ecs(ctx.download_ecs(), ecs)
    assert np.array_equal(np.bincount(_host(d_rec)["ec"], minlength=len(sets)), ecs.counts)


def _reference_records(lines, mode):
    """the reference's lines -> (sets, (barcode, umi, class, count) records: one per line, in READS mode one per distinct line with its multiplicity,
    as a collapsed BUS file holds them)"""
    sets = sorted({l[3] for l in lines})
    cid = {s: i for i, s in enumerate(sets)}
    if mode == G.UMIS:
        return sets, [(bc, umi, cid[s], 1) for _, bc, umi, s in lines]
    return sets, [(bc, umi, cid[s], n) for (_, bc, umi, s), n in collections.Counter(lines).items()]


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("name", sorted(B.golden_cases()))
def test_chain_on_the_references_records(ka, world, name, holes):
    """split, pseudoalign, finalize, read_ecs, bus_records, bus_sort, then the table of the batch's classes and the gene count: the matrix and the
    counters are the restated gene count of the reference's own lines, barcodes matched by value"""
    from kallisto_amd import bus_sc
    from tests.test_gpu_bus_sort import _batch
    ctx = world(B.CASES[name]["fixture"])
    _, lines = B.load_golden(name)
    d_rec, sets, _, L = _batch(ka, ctx, name)
    mode = bus_sc.count_mode(L)
    tr_gene, n_genes = G.golden_map(int(ctx_targets(ka, name)), holes)
    table = ctx.bus_genes(tr_gene, n_genes, sets)
    srt, _ = ctx.bus_sort(d_rec, None, True)
    c = ctx.bus_count_genes(table, srt, mode)
    table.free()
    ref_sets, ref_recs = _reference_records(lines, mode)
    want = G.py_gene_count(ref_recs, mode, G.py_gene_lists(tr_gene, ref_sets))
    barcodes = c["barcodes"].cpu().numpy().view(np.uint64).tolist()
    en = _entries(c["entries"])
    assert barcodes == want["barcodes"]
    assert dict(zip(zip(en["row"].tolist(), en["ec"].tolist()), en["value"].tolist())) == want["entries"]
    for k in ("n_umis", "n_counted", "n_no_gene", "n_multi_gene"):
        assert c["stats"][k] == want[k], k
    assert c["stats"]["n_barcodes"] == len(barcodes) and c["stats"]["n_entries"] == len(en)


def ctx_targets(ka, name):
    _, idx, _, _ = common.load_case(B.CASES[name]["fixture"])
    return ka.Index(idx).num_targets


def _write_t2g(path, names, tr_gene):
    """gene g as "G<g>" with a common name, in an order in which the genes first appear as 0, 1, 2, ...; transcripts without a gene are left out"""
    with open(path, "w") as f:
        for t, g in enumerate(tr_gene.tolist()):
            if g >= 0:
                f.write("%s\tG%d\tname%d\n" % (names[t], g, g))


def _read_gene_dir(d):
    lines = open(os.path.join(d, "output.mtx")).read().split("\n")[:-1]
    assert lines[0] == "%%MatrixMarket matrix coordinate integer general"
    shape = [int(x) for x in lines[1].split()]
    trip = [tuple(int(x) for x in l.split()) for l in lines[2:]]
    assert shape[2] == len(trip) and trip == sorted(trip) and len({t[:2] for t in trip}) == len(trip)
    from tests import bus_correct_common as K
    barcodes = [K.encode(s) for s in open(os.path.join(d, "output.barcodes.txt")).read().split("\n")[:-1]]
    genes = open(os.path.join(d, "output.genes.txt")).read().split("\n")[:-1]
    assert shape[:2] == [len(barcodes), len(genes)]
    return barcodes, genes, {(barcodes[r - 1], genes[g - 1]): v for r, g, v in trip}, json.load(open(os.path.join(d, "count.json")))


@pytest.mark.parametrize("name", B.DRIVER_CASES)
def test_driver_genecounts(ka, name, tmp_path):
    """bus_sc --genecounts -g with and without --count, and a run without the flag: the three files and count.json are the restated gene count of
    the reference's lines; counts/ and the run's own files are what they are without the flag"""
    from kallisto_amd import bus_sc
    from tests.test_gpu_bus_correct import _bus_file, _case_files, _ec_file
    c, idx, files = _case_files(name, tmp_path)
    _, lines = B.load_golden(name)
    names = ka.Index(idx).target_names()
    tr_gene, n_genes = G.golden_map(len(names), True)
    t2g = str(tmp_path / "t2g.txt")
    _write_t2g(t2g, names, tr_gene)
    plain, counted, genes, both = (str(tmp_path / x) for x in ("plain", "counted", "genes", "both"))
    assert bus_sc.main(["-x", c["tech"], "-i", idx, "-o", plain, "--unit-records", "1000", *c["flags"], *files]) == 0   # (units of 1000: classes merged batch by batch)
    assert bus_sc.main(["-x", c["tech"], "-i", idx, "-o", counted, "--count", *c["flags"], *files]) == 0
    assert bus_sc.main(["-x", c["tech"], "-i", idx, "-o", genes, "--genecounts", "-g", t2g, "--unit-records", "1000", *c["flags"], *files]) == 0
    info = bus_sc.run(c["tech"], idx, both, files, count=True, genecounts=True, genemap=t2g)
    # without the flag: the records are the reference's, and nothing of the flag's is written
    hdr, rec = _bus_file(os.path.join(plain, "output.bus"))
    ecs = _ec_file(os.path.join(plain, "matrix.ec"))
    assert sorted((int(r["flags"]), int(r["barcode"]), int(r["umi"]), ecs[int(r["ec"])]) for r in rec for _ in range(int(r["count"]))) == lines
    assert not os.path.exists(os.path.join(plain, "genes")) and not os.path.exists(os.path.join(counted, "genes"))
    for f in ("output.bus", "matrix.ec", "transcripts.txt"):
        assert open(os.path.join(genes, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
        assert open(os.path.join(both, f), "rb").read() == open(os.path.join(counted, f), "rb").read(), f
    for f in ("output.mtx", "output.barcodes.txt", "output.ec.txt"):   # counts/ is what it was
        assert open(os.path.join(both, "counts", f), "rb").read() == open(os.path.join(counted, "counts", f), "rb").read(), f
    assert not os.path.exists(os.path.join(genes, "counts"))
    assert set(json.load(open(os.path.join(genes, "run_info.json")))) == set(json.load(open(os.path.join(plain, "run_info.json"))))
    # the gene matrix: the restatement on the reference's lines
    mode = bus_sc.count_mode(ka.BusLayout.parse(c["tech"])[0])
    ref_sets, ref_recs = _reference_records(lines, mode)
    want = G.py_gene_count(ref_recs, mode, G.py_gene_lists(tr_gene, ref_sets))
    gene_names = ["G%d" % g for g in sorted({g for g in tr_gene.tolist() if g >= 0})]
    for out in (genes, both):
        barcodes, gnames, matrix, counters = _read_gene_dir(os.path.join(out, "genes"))
        assert barcodes == want["barcodes"] and gnames == gene_names
        assert matrix == {(want["barcodes"][r], "G%d" % g): v for (r, g), v in want["entries"].items()}
        assert counters == {"n_barcodes": len(barcodes), **{k: want[k] for k in ("n_umis", "n_counted", "n_no_gene", "n_multi_gene")}}
    assert {k: info["genes_" + k] for k in counters} == counters and info["n_barcodes"] == len(barcodes)


def test_driver_genecounts_with_a_whitelist(ka, tmp_path):
    from kallisto_amd import bus_sc
    from tests import bus_correct_common as K
    from tests.test_gpu_bus_correct import _case_files, _expected_lines
    name = "10xv3"
    c, idx, files = _case_files(name, tmp_path)
    W, L, want_lines, _ = _expected_lines(name)
    wpath, t2g, out = str(tmp_path / "whitelist.txt"), str(tmp_path / "t2g.txt"), str(tmp_path / "out")
    open(wpath, "wb").write(K.whitelist_text(W, L))
    names = ka.Index(idx).target_names()
    tr_gene, _ = G.golden_map(len(names), False)
    _write_t2g(t2g, names, tr_gene)
    assert bus_sc.main(["-x", c["tech"], "-i", idx, "-o", out, "-w", wpath, "--genecounts", "-g", t2g, *c["flags"], *files]) == 0
    ref_sets, ref_recs = _reference_records(want_lines, G.UMIS)
    want = G.py_gene_count(ref_recs, G.UMIS, G.py_gene_lists(tr_gene, ref_sets))
    barcodes, gnames, matrix, counters = _read_gene_dir(os.path.join(out, "genes"))
    assert set(barcodes) <= set(W) and barcodes == want["barcodes"]                 # only listed barcodes are rows
    assert matrix == {(want["barcodes"][r], "G%d" % g): v for (r, g), v in want["entries"].items()}
    assert counters["n_counted"] == want["n_counted"] and counters["n_umis"] == want["n_umis"]


def test_driver_refusals(ka, tmp_path, capsys):
    from kallisto_amd import bus_sc
    _, idx, _, _ = common.load_case("ref_test_pe")
    t2g, never = str(tmp_path / "t2g.txt"), str(tmp_path / "never")
    open(t2g, "w").write("no_such_transcript g1\n")
    with pytest.raises(ka.KallistoAmdError, match="--genecounts needs a transcripts-to-genes file"):
        bus_sc.run("10XV3", idx, never, ["a.fq", "b.fq"], genecounts=True)
    with pytest.raises(ka.KallistoAmdError, match="only used with --genecounts"):
        bus_sc.run("10XV3", idx, never, ["a.fq", "b.fq"], genemap=t2g)
    with pytest.raises(ka.KallistoAmdError, match="Error: Invalid transcript: no_such_transcript in " + t2g):
        bus_sc.run("10XV3", idx, never, ["a.fq", "b.fq"], genecounts=True, genemap=t2g)
    assert bus_sc.main(["-x", "10XV3", "-i", idx, "-o", never, "--genecounts", "a.fq", "b.fq"]) == 1
    assert "--genecounts needs" in capsys.readouterr().err
    assert bus_sc.main(["-x", "10XV3", "-i", idx, "-o", never, "-g", t2g, "a.fq", "b.fq"]) == 1
    assert "only used with --genecounts" in capsys.readouterr().err
    assert not os.path.exists(never)
