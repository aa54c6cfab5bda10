"""BUS records to a cells x classes matrix on the GPU (kamd_bus_sort, kamd_bus_count, `bus_sc --count`).  The yardsticks are numpy (lexsort, run-length
sums), the CPU build of the rules (tests/emu_bussort), a dict restatement of `bustools count` (tests/bus_sort_common.py) and the reference's own
output (tests/golden/bus_sc, tests/golden/bus_tcc); never the code under test.  Integers only: every comparison is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import bus_sc_common as B
from tests import bus_sort_common as S
from tests import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4 * 65536 + 1234]
KINDS = ["random", "tenx", "equal", "barcode_top_bit", "flags_bit0", "negative_ec", "sorted", "reversed"]
NO_UMI = 2 ** 64 - 1


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
    return torch.from_numpy(np.ascontiguousarray(rec, S.REC).view(np.int64).reshape(-1, 4).copy()).to("cuda:0")


def _host(t):
    return np.ascontiguousarray(t.cpu().numpy()).reshape(-1).view(S.REC)


def _sort(ctx, rec, ec_map=None, collapse=True):
    out, st = ctx.bus_sort(_dev(rec), ec_map, collapse)
    return _host(out), st


def _keys(kind, n, seed):
    rng = np.random.default_rng(seed)
    u64 = lambda hi: rng.integers(0, hi, n, dtype=np.uint64)
    if kind == "random":
        r = S.make_records(u64(2 ** 64), u64(2 ** 64), rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), u64(2 ** 32).astype(np.uint32))
    elif kind in ("tenx", "sorted", "reversed"):
        pool = rng.integers(0, 2 ** 32, 50, dtype=np.uint64)
        r = S.make_records(pool[rng.integers(0, 50, n)], u64(2 ** 24), rng.integers(0, 1000, n).astype(np.int32), np.array([0, 1, 5], np.uint32)[rng.integers(0, 3, n)])
        if kind != "tenx":
            r = S.np_sort(r)
            r = r[::-1].copy() if kind == "reversed" else r
    elif kind == "equal":
        r = S.make_records(np.full(n, 0x1234567890, np.uint64), 77, 5, 1)
    elif kind == "barcode_top_bit":
        r = S.make_records(np.uint64(0x1234) | (u64(2) << np.uint64(63)), 77, 5, 1)
    elif kind == "flags_bit0":
        r = S.make_records(np.full(n, 0x1234, np.uint64), 77, 5, u64(2).astype(np.uint32) | np.uint32(4))
    elif kind == "negative_ec":
        ec = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
        ec[:min(n, 4)] = np.array([-1, -2 ** 31, 0, 2 ** 31 - 1], np.int32)[:min(n, 4)]
        r = S.make_records(u64(3), u64(2), ec, 0)
    r["count"] = rng.integers(1, 6, n)
    r["pad"] = np.arange(n)   # the input index: stability
    return r


@pytest.mark.parametrize("kind", KINDS)
def test_sort_and_collapse_equal_numpy(ctx, kind):
    for n in SIZES:
        rec = _keys(kind, n, 100 + n)
        want = S.np_sort(rec)
        passes = bin(S.emu_plan(rec)).count("1")
        assert S.emu_plan(rec) == S.np_plan(rec)
        got, st = _sort(ctx, rec, collapse=False)
        assert got.tobytes() == want.tobytes(), (kind, n)                      # every field, pad included: the sort is stable
        assert (st["n_in"], st["n_out"], st["passes"]) == (n, n, passes), (kind, n)
        col, sums = S.np_collapse(want)
        got, st = _sort(ctx, rec, collapse=True)
        assert got.tobytes() == col.tobytes(), (kind, n)                       # sums of the runs, pad of each run's first record
        assert (st["n_in"], st["n_out"], st["passes"]) == (n, len(col), passes), (kind, n)
    assert passes == {"random": 24, "equal": 0, "barcode_top_bit": 1, "flags_bit0": 1}.get(kind, passes)


def test_sort_is_reproducible(ctx):
    for kind in ("random", "tenx"):
        rec = _keys(kind, SIZES[-1], 7)
        for collapse in (False, True):
            a, _ = _sort(ctx, rec, collapse=collapse)
            b, _ = _sort(ctx, rec, collapse=collapse)
            assert a.tobytes() == b.tobytes()


def test_ec_map(ctx, ka):
    import torch
    rec = _keys("tenx", 70001, 8)
    perm = np.random.default_rng(9).permutation(1000).astype(np.int32)
    d_map = torch.from_numpy(perm).to("cuda:0")
    mapped = rec.copy()
    mapped["ec"] = perm[rec["ec"]]
    got, _ = _sort(ctx, rec, d_map, collapse=False)
    assert got.tobytes() == S.np_sort(mapped).tobytes()
    got, _ = _sort(ctx, rec, d_map, collapse=True)
    assert got.tobytes() == S.np_collapse(S.np_sort(mapped))[0].tobytes()
    for bad in (1000, -1):   # a row equal to n_map, a negative row: an error, and the buffer is as it was
        r2 = rec.copy()
        r2["ec"][12345] = bad
        d = _dev(r2)
        with pytest.raises(ka.KallistoAmdError, match="1 records name a class outside the map"):
            ctx.bus_sort(d, d_map, True)
        assert _host(d).tobytes() == r2.tobytes()


def test_count_sums_are_held_in_64_bits(ctx, ka):
    over = S.make_records([9, 3, 9], 4, 2, 0, [0xFFFFFFFF, 5, 1])
    with pytest.raises(ka.KallistoAmdError, match="0xFFFFFFFF"):
        _sort(ctx, over)
    full = S.make_records([9, 3, 9], 4, 2, 0, [0xFFFFFFFE, 5, 1])
    got, _ = _sort(ctx, full)
    assert got["count"].tolist() == [5, 0xFFFFFFFF] and got["barcode"].tolist() == [3, 9]
    # ... and across wavefronts and blocks: 1000 records of one key, 0xFFFFFFFF in all
    many = S.make_records(np.full(1000, 9, np.uint64), 4, 2, 0, np.full(1000, 4294967, np.uint32))
    many["count"][-1] += 0xFFFFFFFF - int(many["count"].astype(np.int64).sum())
    got, _ = _sort(ctx, many)
    assert len(got) == 1 and int(got["count"][0]) == 0xFFFFFFFF
    many["count"][500] += 1
    with pytest.raises(ka.KallistoAmdError, match="0xFFFFFFFF"):
        _sort(ctx, many)


def test_merging_two_collapsed_halves(ctx):
    rec = _keys("tenx", 50000, 10)
    rec["umi"] &= np.uint64(0xFF)       # many equal keys
    whole, _ = _sort(ctx, rec)
    a, _ = _sort(ctx, rec[:23456])
    b, _ = _sort(ctx, rec[23456:])
    both, _ = _sort(ctx, np.concatenate([a, b]))
    assert both[["barcode", "umi", "ec", "count", "flags"]].tolist() == whole[["barcode", "umi", "ec", "count", "flags"]].tolist()
    assert len(whole) < len(a) + len(b)


def _count(ctx, rec_sorted, mode):
    c = ctx.bus_count(_dev(rec_sorted), mode)
    en = np.ascontiguousarray(c["entries"].cpu().numpy()).reshape(-1).view(S.ENTRY)
    st = {k: v for k, v in c["stats"].items() if k != "ms"}
    return c["barcodes"].cpu().numpy().view(np.uint64), en, _host(c["multi"]), st


def _count_records(what):
    rng = np.random.default_rng(11)
    if what in ("one_barcode", "many_barcodes"):
        nb = 1 if what == "one_barcode" else 300
        n = 3000 if nb == 1 else 40000
        pool = rng.integers(0, 2 ** 32, nb, dtype=np.uint64)
        r = S.make_records(pool[rng.integers(0, nb, n)], rng.integers(0, 64, n, dtype=np.uint64), rng.integers(0, 7, n).astype(np.int32),
                           np.array([0, 1, 5], np.uint32)[rng.integers(0, 3, n)], rng.integers(1, 4, n))
        if nb > 1:   # a barcode whose groups are all multi-class: it still gets a row
            r = np.concatenate([r, S.make_records([2 ** 40] * 6, [1, 1, 2, 2, 2, 3], [4, 5, 1, 2, 3, 0], 0, 1), S.make_records([2 ** 40], [3], [6])])
        return r
    if what == "block_boundary":   # a multi-class group over records 250 .. 269 of the sorted input; single-class groups around it
        return np.concatenate([S.make_records([1] * 250, np.arange(250), 1), S.make_records([1] * 20, 250, np.arange(20)), S.make_records([1] * 300, 251 + np.arange(300), 2),
                               S.make_records([2] * 5, 0, [1, 1, 1, 2, 2])])
    if what == "long_group":       # 70 000 records of one (barcode, UMI, class), between two ordinary barcodes; a long multi-class group as well
        return np.concatenate([S.make_records([1, 1], [1, 2], [3, 4]), S.make_records([5] * 70000, 9, 3, 0, 2), S.make_records([5] * 3, 10, [3, 3, 8]),
                               S.make_records([6] * 2000, 1, np.arange(2000) % 3), S.make_records([7], 1, 0)])
    if what == "no_umi":           # an absent UMI: a whole barcode is one group
        return np.concatenate([S.make_records([1] * 900, NO_UMI, 5, rng.integers(0, 3, 900).astype(np.uint32)), S.make_records([2] * 700, NO_UMI, rng.integers(0, 4, 700).astype(np.int32)),
                               S.make_records([3], NO_UMI, 2)])
    raise KeyError(what)


@pytest.mark.parametrize("what", ["one_barcode", "many_barcodes", "block_boundary", "long_group", "no_umi"])
def test_count_equals_the_dict_restatement(ctx, what):
    rec = _count_records(what)
    srt = S.np_sort(rec)
    for data in (srt, S.np_collapse(srt)[0]):
        for mode in (S.UMIS, S.READS):
            bc, en, mu, st = _count(ctx, data, mode)
            want = S.assert_count_is_the_restatement(data, mode, bc, en, mu, st)
            ebc, een, emu, est, over = S.emu_count(data, mode)             # ... and the CPU build of the same rules says the same
            assert over == 0 and en.tobytes() == een.tobytes() and mu.tobytes() == emu.tobytes() and st == est
            if mode == S.READS:
                assert st["n_multi_groups"] == 0
    want = S.py_count(S.rec_tuples(srt), S.UMIS)
    if what == "many_barcodes":
        row = want["barcodes"].index(2 ** 40)
        assert {(2 ** 40, u) for u in (1, 2, 3)} <= set(want["multi"]) and not any(r == row for r, _ in want["entries"])
    if what == "block_boundary":
        assert (1, 250) in want["multi"] and [int(x) for x in np.flatnonzero((srt["barcode"] == 1) & (srt["umi"] == 250))[[0, -1]]] == [250, 269]
    if what == "long_group":
        assert want["entries"][(1, 3)] == 1 and (5, 10) in want["multi"] and (6, 1) in want["multi"]
    if what == "no_umi":
        assert want["entries"] == {(0, 5): 1, (2, 2): 1} and set(want["multi"]) == {(2, NO_UMI)}


def test_count_refuses_unsorted_input(ctx, ka):
    srt = S.np_sort(_count_records("one_barcode"))
    bad = srt.copy()
    bad[[100, 2000]] = bad[[2000, 100]]
    with pytest.raises(ka.KallistoAmdError, match="not sorted"):
        ctx.bus_count(_dev(bad), S.UMIS)
    bc, en, mu, st = _count(ctx, srt[:0], S.UMIS)   # no records: no rows
    assert len(bc) == len(en) == len(mu) == 0 and st["n_barcodes"] == 0


def _same_ecs(a, b):
    return np.array_equal(a.ec_off, b.ec_off) and np.array_equal(a.ec_ids, b.ec_ids) and np.array_equal(a.counts, b.counts)


def _batch(ka, ctx, name, between=None, behind=None):
    """reset -> bus_split -> pseudoalign -> [between] -> finalize -> read_ecs -> bus_records -> [behind]: (device records with batch-local rows, the rows'
    transcript sets, the finalized result, the layout)"""
    c = B.CASES[name]
    L, _ = ka.BusLayout.parse(c["tech"])
    opts = ka.QuantOpts(0, 200.0, 20.0, 1, B.case_strand(name), 0, 0)
    import torch
    words, lens, n, max_len = B.case_batch(name)
    dw, dl = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0"), torch.from_numpy(lens.view(np.int16).copy()).to("cuda:0")
    ctx.reset()
    sp = ctx.bus_split(L, dw, dl, n, max_len)
    cut = (sp["seq_words"], sp["seq_len"], sp["n_valid"], sp["seq_max_len"])
    ctx.pseudoalign(opts, *cut)
    if between:
        between()
    ecs = ctx.finalize()
    d_ec, _ = ctx.read_ecs(opts, *cut)
    rec = ctx.bus_records(sp["tags"], d_ec, sp["n_valid"])
    if behind:
        behind()
    sets = [tuple(ecs.ec_ids[int(ecs.ec_off[i]):int(ecs.ec_off[i + 1])].tolist()) for i in range(len(ecs.counts))]
    return rec, sets, ecs, L


def test_sort_and_count_leave_the_ec_state_alone(ka, world):
    ctx = world("ref_test_pe")
    rec = S.np_sort(_count_records("many_barcodes"))

    def both():
        got, _ = _sort(ctx, rec[::-1].copy())
        _count(ctx, got, S.UMIS)
    _, _, plain, _ = _batch(ka, ctx, "10xv3")
    d_rec, sets, ecs, _ = _batch(ka, ctx, "10xv3", between=both, behind=both)   # between the batch and its finalize, and behind it
    assert ecs.multiset() == plain.multiset()                                     # (the order of the rows is not fixed from one finalize to the next)
    assert _same_ecs(ctx.download_ecs(), ecs)                                     # the result the context holds is the one finalize described
    assert np.array_equal(np.bincount(_host(d_rec)["ec"], minlength=len(sets)), ecs.counts)


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_matrix_of_the_references_records(ka, world, name):
    """the case run as tests/test_gpu_bus_sc.py runs it, then bus_sort, bus_count and the driver's host resolution: the matrix is the restated count of
    the reference's own lines, barcodes matched by value and classes by transcript set"""
    from kallisto_amd import bus_sc
    ctx = world(B.CASES[name]["fixture"])
    _, lines = B.load_golden(name)
    d_rec, sets, _, L = _batch(ka, ctx, name)
    mode = bus_sc.count_mode(L)
    assert mode == (S.READS if name == "no_umi" else S.UMIS)
    srt, _ = ctx.bus_sort(d_rec, None, True)
    assert sorted((int(r["flags"]), int(r["barcode"]), int(r["umi"]), sets[int(r["ec"])]) for r in _host(srt) for _ in range(int(r["count"]))) == lines
    c = ctx.bus_count(srt, mode)
    en = np.ascontiguousarray(c["entries"].cpu().numpy()).reshape(-1).view(S.ENTRY)
    matrix = dict(zip(zip(en["row"].tolist(), en["ec"].tolist()), en["value"].tolist()))
    ec_sets = list(sets)
    ec_of = {s: i for i, s in enumerate(ec_sets)}
    dropped = bus_sc.resolve_multi(_host(c["multi"]), matrix, ec_of, ec_sets)
    barcodes = c["barcodes"].cpu().numpy().view(np.uint64).tolist()
    got = {(barcodes[r], ec_sets[e]): v for (r, e), v in matrix.items()}
    want, n_multi, n_dropped = S.py_matrix([(bc, umi, s, 1) for _, bc, umi, s in lines], mode, lambda s: s)
    assert got == want
    assert (c["stats"]["n_multi_groups"], dropped) == (n_multi, n_dropped)
    assert barcodes == sorted({bc for _, bc, _, _ in lines})


def test_reads_mode_gives_the_references_tcc_matrix(ka, ctx, tmp_path):
    """`kallisto_amd_quant bus -x bulk --paired` on the samples of tests/golden/bus_tcc/ref_test_pe_boot; its output.bus through bus_sort and bus_count in
    READS mode is the fixture's tcc.mtx (made from the reference's BUS file), classes matched through the two matrix.ec files"""
    from tests import test_gpu_bus_tcc as T
    gold = os.path.join(T.GOLD, "ref_test_pe_boot")
    meta = json.load(open(os.path.join(gold, "case.json")))
    _, out = T._run_bus(meta, tmp_path)
    _, rec = T._read_bus(os.path.join(out, "output.bus"))
    ours, theirs = T._read_ec(os.path.join(out, "matrix.ec")), T._read_ec(os.path.join(gold, "matrix.ec"))
    col = {s: j for j, s in enumerate(theirs)}
    srt, _ = ctx.bus_sort(_dev(rec.view(S.REC)), None, True)
    c = ctx.bus_count(srt, S.READS)
    en = np.ascontiguousarray(c["entries"].cpu().numpy()).reshape(-1).view(S.ENTRY)
    want = T._mtx(os.path.join(gold, "tcc.mtx"))
    got = np.zeros_like(want)
    barcodes = c["barcodes"].cpu().numpy().view(np.uint64).tolist()
    assert barcodes == list(range(want.shape[0])) and c["stats"]["n_multi_records"] == 0
    for e in en:
        got[barcodes[int(e["row"])], col[ours[int(e["ec"])]]] += int(e["value"])
    assert np.array_equal(got, want)


def _bus_file(path):
    b = open(path, "rb").read()
    ver, bclen, umilen, tlen = np.frombuffer(b[4:20], "<u4").tolist()
    return bclen, np.frombuffer(b[20 + tlen:], S.REC)


def _ec_file(path):
    return [tuple(int(x) for x in l.split()[1].split(",")) for l in open(path)]


def test_driver_count(ka, tmp_path):
    """bus_sc --count with merges every 1000 records: output.bus is the bytes of a run without --count and with the default merge threshold; the
    files under counts/ are the restated count of those records; quant-tcc takes them"""
    from kallisto_amd import bus_sc
    from tests.test_gpu_bus_sc import _write_fastq
    name = B.DRIVER_CASES[0]
    c = B.CASES[name]
    L, _, items, _ = B.case_reads(name)
    _, idx, _, _ = common.load_case(c["fixture"])
    files = [str(tmp_path / ("reads_%d.fq" % f)) for f in range(L.n_files)]
    for f, p in enumerate(files):
        _write_fastq(p, [it[f] for it in items], False)
    plain, counted = str(tmp_path / "plain"), str(tmp_path / "counted")
    assert bus_sc.main(["-x", c["tech"], "-i", idx, "-o", plain, "--unit-records", "1000", *c["flags"], *files]) == 0
    info = bus_sc.run(c["tech"], idx, counted, files, unit_records=1000, count=True, merge_records=1000)
    assert open(os.path.join(counted, "output.bus"), "rb").read() == open(os.path.join(plain, "output.bus"), "rb").read()
    assert not os.path.exists(os.path.join(plain, "counts"))
    bclen, rec = _bus_file(os.path.join(counted, "output.bus"))
    assert info["n_pseudoaligned"] > 2 * 1000                                     # more than twice the threshold came in, 1000 read sets at a time: two merges before the final one
    cd = os.path.join(counted, "counts")
    ecs = _ec_file(os.path.join(cd, "output.ec.txt"))
    assert ecs == _ec_file(os.path.join(counted, "matrix.ec")) and ecs[:len(_ec_file(os.path.join(plain, "matrix.ec")))] == _ec_file(os.path.join(plain, "matrix.ec"))
    want, n_multi, n_dropped = S.py_matrix([(int(r["barcode"]), int(r["umi"]), ecs[int(r["ec"])], int(r["count"])) for r in rec], S.UMIS, lambda s: s)
    barcodes = sorted({int(b) for b in rec["barcode"]})
    decode = lambda b: "".join("ACGT"[(b >> (2 * (bclen - 1 - i))) & 3] for i in range(bclen))
    assert open(os.path.join(cd, "output.barcodes.txt")).read().split("\n")[:-1] == [decode(b) for b in barcodes]
    lines = open(os.path.join(cd, "output.mtx")).read().split("\n")[:-1]
    assert lines[0] == "%%MatrixMarket matrix coordinate integer general"
    assert [int(x) for x in lines[1].split()] == [len(barcodes), len(ecs), len(lines) - 2]
    trip = [tuple(int(x) for x in l.split()) for l in lines[2:]]
    assert trip == sorted(trip) and len({t[:2] for t in trip}) == len(trip)
    assert {(barcodes[r - 1], ecs[e - 1]): v for r, e, v in trip} == want
    assert len(set(ecs)) == len(ecs)
    assert (info["n_barcodes"], info["n_multi_umis"]) == (len(barcodes), n_multi) and info["n_umis"] == len({(int(r["barcode"]), int(r["umi"])) for r in rec})
    assert n_multi >= 1
    assert set(json.load(open(os.path.join(counted, "run_info.json")))) == set(json.load(open(os.path.join(plain, "run_info.json"))))
    q = str(tmp_path / "q")
    p = subprocess.run([EXE, "quant-tcc", "-i", idx, "-e", os.path.join(cd, "output.ec.txt"), "-o", q, os.path.join(cd, "output.mtx")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    ab = [l for l in open(os.path.join(q, "matrix.abundance.mtx")) if not l.startswith("%")]
    assert int(ab[0].split()[0]) == len(barcodes)
