"""An index with shades (targets named <base>_shade_<variant>) on the GPU, against the reference's goldens on tests/golden/shades_pe
(tests/golden/make_shades.py): the library's quant flow in every form it can take, the bulk `bus` consumer, the CLI and its refusals, and that
nothing of a shaded index stays behind when an ordinary one follows it.  EC resolution intersects the cores and k_shade_extend (kamd_ec.hip) puts
the surviving shades back; the straight-line kernels (filters, --union, fragment lengths) enumerate the class by kamd_core.h for_each_in_shaded_set."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import common, shades

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
BUS_DTYPE = np.dtype([("bc", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
MODES = ("one_batch", "four_batches", "overflow_after", "overflow_straight", "device_build", "flat_file")


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    kallisto_amd.load_library()
    return kallisto_amd


@pytest.fixture(scope="module")
def idx_path(tmp_path_factory):
    return shades.unpack_index(tmp_path_factory.mktemp("shades"))


@pytest.fixture(scope="module")
def fixture():
    return shades.load_reads()


@pytest.fixture(scope="module")
def ctxs(ka, idx_path, tmp_path_factory):
    """a context per way of bringing the index to the device: host-built table, device-built table, flattened file"""
    cache = {}

    def get(kind):
        if kind not in cache:
            if kind == "device":
                index = ka.Index(idx_path, deferred=True)
            elif kind == "flat":
                flat = str(tmp_path_factory.mktemp("flat") / "index.kamd")
                src = ka.Index(idx_path)
                src.save(flat)
                src.close()
                index = ka.Index(flat)
            else:
                index = ka.Index(idx_path)
            ctx = ka.Context(0)
            cache[kind] = (index, ctx)
        index, ctx = cache[kind]
        ctx.upload(index)   # resets the EC state
        return index, ctx
    yield get
    for _, c in cache.values():
        c.close()


def _fastq(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def _opts(ka, o):
    return ka.QuantOpts(o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"])


def _batches(ka, ctx, r1, r2, paired, n_batches):
    reads = common.interleave(r1, r2 if paired else None)
    words, lens, max_len = ctx.pack_reads_host(reads)
    if n_batches == 1:
        return [(words, lens, len(r1), max_len)]
    per_item = (2 if paired else 1)
    rec = ka.packed_record_words(max_len) * per_item
    cuts = [len(r1) * i // n_batches for i in range(n_batches + 1)]
    return [(words[a * rec:b * rec], lens[a * per_item:b * per_item], b - a, max_len) for a, b in zip(cuts[:-1], cuts[1:])]


def test_index_object_exposes_shades(ka, idx_path, fixture):
    index = ka.Index(idx_path)
    try:
        assert index.n_shades == fixture[0]["n_shades"]
        assert np.array_equal(index.shade_colour, shades.colours_of_names(index.target_names()))
        core_off, core_ids, shade_off, shade_ids = index.shade_sets()
        ec_off, ec_ids = index.ec_sets()
        assert len(core_off) == len(shade_off) == len(ec_off) and len(core_ids) + len(shade_ids) == len(ec_ids)
    finally:
        index.close()
    plain = ka.Index(common.load_case("ref_test_pe")[1])
    try:
        assert plain.n_shades == 0 and (plain.shade_colour == shades.NOT_A_SHADE).all() and all(len(a) == 0 for a in plain.shade_sets())
    finally:
        plain.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", shades.DUMP_VARIANTS)
def test_quant_matches_reference(variant, mode, ka, ctxs, fixture):
    meta, r1, r2 = fixture
    o = common.parse_variant(meta["variants"][variant])
    exp = shades.load_expected(variant)
    index, ctx = ctxs({"device_build": "device", "flat_file": "flat"}.get(mode, "host"))
    assert index.n_shades == meta["n_shades"] and np.array_equal(index.target_lens, exp["lens"])
    if mode == "device_build":
        assert ctx.table_info()["built_on_device"] == 1
    ctx.tune(overflow_second_pass={"overflow_after": 3, "overflow_straight": 2}.get(mode, 1))
    try:
        res = ka.quant(ctx, _opts(ka, o), _batches(ka, ctx, r1, r2, o["paired"], 4 if mode == "four_batches" else 1))
        n_overflow = ctx.profile()["n_overflow_items"]
    finally:
        ctx.tune(overflow_second_pass=1)
    assert res.n_processed == exp["nproc"]
    assert res.ecs.multiset() == exp["ecs"]
    assert np.array_equal(res.flens, exp["flens"])
    assert np.array_equal(res.eff_lens, exp["eff"])
    common.assert_abundance_close(res.est_counts, exp["alpha"], "est_counts")
    assert res.em_rounds == meta["em_rounds"][variant]   # the round the reference's own EM stopped in (case.json, from `kallisto quant`)
    if o["paired"]:
        assert n_overflow > 0   # pairs with more than eight classes took the overflow passes (the long transcript's 24 shades)


def _install(ctx, records, dense):
    """records (count, [set ids]) -> Context.tuples_replace, dense {set id: count} -> Context.dense_counts()"""
    torch = ctx.torch
    dev = f"cuda:{ctx.device}"
    ctx.reset()
    d = ctx.dense_counts()
    d.zero_()
    if dense:
        d[torch.tensor(list(dense.keys()), dtype=torch.int64, device=dev)] = torch.tensor(list(dense.values()), dtype=torch.int32, device=dev)
    words, offs = [], []
    for cnt, es in records:
        offs.append(len(words))
        words += [int(cnt), len(es)] + [int(e) for e in es]
    w = torch.from_numpy(np.array(words, np.int64).astype(np.uint32).view(np.int32)).to(dev)
    ctx.tuples_replace(w, torch.from_numpy(np.array(offs, np.int64)).to(dev))


def test_records_installed_directly(ka, ctxs, fixture, idx_path):
    """EC resolution on an index with shades, path by path: k_resolve / k_resolve_big intersect the CORES, k_shade_extend puts the shades of the
    tuple's sets back whose colour survived, k_cand_singles copies a dense set whole (it holds the colours of its own shades).  Tuples: every
    distinct tuple of the fixture's pairs (tests/emu_shade lists them), pairs and triples of sets around every target with shades, and for every
    kernel path tuples of sets of that size class with a common target.  The host reference is the rule on Python sets (tests/shades.ShadeRule);
    which path takes a tuple follows from the sizes of its cores (bigsets.path_of restates k_bound_tuples), asserted below together with the
    shade situations each path met: no shade, one, more than 16, the same shade from several sets -- for every path, and more than 16 on the
    bitmap arm (the members of the families of 17, 129 and 1025 that carry 20 shades inside the family's segment)."""
    from tests import bigsets
    meta, r1, r2 = fixture
    index, ctx = ctxs("host")
    sets = bigsets.sets_of_device_index(index)
    colour = index.shade_colour
    is_shade = colour != shades.NOT_A_SHADE
    core_off = index.shade_sets()[0].astype(np.int64)
    cores = bigsets.Sets(core_off, index.shade_sets()[1].astype(np.int64), sets.onlist, sets.n_targets)   # (sizes of the cores: what the kernels branch on)
    rule = shades.ShadeRule(lambda e: sets.members(e).tolist(), colour)
    rng = np.random.default_rng(23)
    # (a) the fixture's own tuples
    ex = shades.EmuIndex(idx_path)
    res = shades.emu_quant(ex, r1, r2, common.parse_variant([]), sets_stride=256)
    ex.close()
    tuples = {}
    for i in range(len(r1)):
        n = int(res["n_sets"][i])
        if res["sets"][i][0] and n > 1:
            key = tuple(int(x) for x in res["sets"][i][1:1 + n])
            tuples[key] = tuples.get(key, 0) + 1
    # (b) sets around every target with shades, and (c) per size class sets with a common target
    t_of, e_of = np.nonzero(sets.matrix.T)
    start = np.searchsorted(t_of, np.arange(sets.n_targets + 1))
    holding = lambda t: e_of[start[t]:start[t + 1]]
    for t in np.unique(colour[is_shade]):
        h = holding(int(t))
        for _ in range(12):
            k = int(rng.integers(2, 5))
            if len(h) >= k:
                key = tuple(int(x) for x in rng.choice(h, k, replace=False))
                tuples[key] = tuples.get(key, 0) + int(rng.integers(1, 5))
    for lo, hi in ((17, 64), (65, 128), (129, 1024), (1025, 1 << 30)):
        pool = np.flatnonzero((cores.sizes >= lo) & (cores.sizes <= hi))
        for _ in range(40):
            t = int(rng.choice(sets.members(int(rng.choice(pool)))))
            if is_shade[t]:
                continue
            h = [e for e in holding(t) if cores.sizes[e] >= lo]
            k = min(len(h), int(rng.integers(2, 5)))
            if k >= 2:
                key = tuple(int(x) for x in rng.choice(h, k, replace=False))
                tuples[key] = tuples.get(key, 0) + 1
    # (d) per size class sets that share a shade (the same shade from several sets), and one of them beside a set without shades
    n_shades_of = np.diff(index.shade_sets()[2].astype(np.int64))
    for sh in np.flatnonzero(is_shade):
        for lo, hi in ((1, 16), (17, 1024), (1025, 1 << 30)):
            pool = [int(e) for e in holding(int(sh)) if lo <= cores.sizes[e] <= hi]
            plain = [int(e) for e in holding(int(colour[sh])) if lo <= cores.sizes[e] <= hi and n_shades_of[e] == 0]
            if len(pool) >= 2:
                key = tuple(int(x) for x in rng.choice(pool, min(len(pool), 3), replace=False))
                tuples[key] = tuples.get(key, 0) + 1
            if pool and plain:
                key = (int(rng.choice(pool)), int(rng.choice(plain)))
                tuples[key] = tuples.get(key, 0) + 2
    # (e) many shades beside large cores: the members that carry a stretch of shades (20 inside a family's segment; 24 on the long transcript),
    #     tuples of up to 12 of the shaded sets that hold them, per size class of the cores; and pairs of shade-free sets above 1024
    stretch = [int(t) for t in np.unique(colour[is_shade]) if (colour == t).sum() >= 20]
    assert len(stretch) >= 4
    for t in stretch:
        for lo, hi in ((1, 16), (17, 128), (129, 1024), (1025, 1 << 30)):
            pool = [int(e) for e in holding(t) if lo <= cores.sizes[e] <= hi and n_shades_of[e] > 0]
            for _ in range(8 if pool else 0):
                key = tuple(int(x) for x in rng.choice(pool, min(len(pool), int(rng.integers(6, 13))), replace=False))
                tuples[key] = tuples.get(key, 0) + 1
    # a shade-free pair of small sets; one shade beside cores above 1024 (a set with exactly one shade and a shade-free one)
    small_plain = np.flatnonzero((cores.sizes >= 2) & (cores.sizes <= 16) & (n_shades_of == 0))
    for e in small_plain[:200]:
        t = int(sets.members(int(e))[0])
        h = [int(f) for f in holding(t) if f != e and cores.sizes[f] <= 16 and n_shades_of[f] == 0]
        if h:
            tuples[(int(e), h[0])] = tuples.get((int(e), h[0]), 0) + 1
    one_huge = [int(e) for e in np.flatnonzero((cores.sizes > 1024) & (n_shades_of == 1))]
    for a in one_huge[:6]:
        for b in [int(e) for e in np.flatnonzero((cores.sizes > 1024) & (n_shades_of == 0))][:2]:
            tuples[(a, b)] = tuples.get((a, b), 0) + 1
    plain_huge = [int(e) for e in np.flatnonzero((cores.sizes > 1024) & (n_shades_of == 0))]
    assert len(plain_huge) >= 2
    for i, a in enumerate(plain_huge[:4]):
        for b in plain_huge[i + 1:4]:
            tuples[(a, b)] = tuples.get((a, b), 0) + 3
    records = [(c, list(es)) for es, c in tuples.items()]
    dense = {}
    for lo, hi in ((1, 64), (65, 1 << 30)):   # k_cand_singles: the thread's copy, the wavefront's copy; sets with shades
        pool = np.flatnonzero((sets.sizes >= lo) & (sets.sizes <= hi) & (n_shades_of > 0))
        assert len(pool) > 0
        dense.update({int(e): int(rng.integers(1, 4)) for e in rng.choice(pool, min(len(pool), 6), replace=False)})
    dense.update({int(e): 2 for e in rng.choice(np.flatnonzero(sets.sizes > 0), 20, replace=False)})
    # the host reference, and what every path met
    want, seen, by_core = {}, {}, {}
    for cnt, es in records:
        cls = rule(es)
        core = tuple(t for t in cls if not is_shade[t])
        n_sh = len(cls) - len(core)
        path = bigsets.path_of(cores, es)
        union = [t for e in es for t in sets.members(e).tolist() if is_shade[t]]
        tag = seen.setdefault(path, set())
        if cls:
            want[cls] = want.get(cls, 0) + cnt
            by_core.setdefault(core, set()).add(cls)
            tag.add("none" if not union else "all_fail" if n_sh == 0 else "one" if n_sh == 1 else "many" if n_sh > 16 else "some")
            if len(union) > len(set(union)) and n_sh:
                tag.add("duplicated")
            n_bm = sum(1 for e in es if cores.sizes[e] > bigsets.BM_MIN_MEMBERS)
            if cores.sizes[es].min() > bigsets.RES_BIG_MIN and (n_bm >= 2 or (n_bm == 1 and cores.sizes[es].min() <= bigsets.BM_MIN_MEMBERS)):
                tag.add("bitmap")
                if n_sh > 16:
                    tag.add("bitmap_many")
        else:
            tag.add("empty")
    for e, cnt in dense.items():
        cls = rule([e])
        assert cls == tuple(sets.members(e).tolist())
        want[cls] = want.get(cls, 0) + cnt
    print("PATHS", {k: sorted(v) for k, v in seen.items()})
    for path in ("all_pairs", "chunk_mask", "big1024", "big4096"):
        assert {"none", "one", "many", "duplicated"} <= seen[path], (path, seen[path])
    assert "bitmap" in seen["big1024"] and "bitmap" in seen["big4096"] and "bitmap_many" in seen["big1024"] and "bitmap_many" in seen["big4096"]
    assert any("all_fail" in v for v in seen.values()) and any("empty" in v for v in seen.values())
    assert any(len(v) > 1 for v in by_core.values())                      # equal cores, different shades: different classes
    assert len(want) < sum(1 for _, es in records if rule(es))            # different tuples, equal classes: merged
    _install(ctx, records, dense)
    assert ctx.finalize().multiset() == want


def test_tuple_records_round_trip(ka, ctxs, fixture):
    """what several ranks exchange: dense counts and exported tuple records, installed in a fresh context, finalize to the same classes"""
    meta, r1, r2 = fixture
    exp = shades.load_expected("pe")
    index, ctx = ctxs("host")
    (words, lens, n, max_len), = _batches(ka, ctx, r1, r2, 1, 1)
    ctx.pseudoalign(ka.QuantOpts(1, 0.0, 0.0, 0, 0), words, lens, n, max_len)
    tw, to = ctx.tuples_export()
    assert to.numel() > 0 and int(ctx.dense_counts().sum()) > 0
    fresh = ka.Context(0)
    try:
        fresh.upload(index)
        fresh.dense_counts().copy_(ctx.dense_counts())
        fresh.tuples_replace(tw, to)
        assert fresh.finalize().multiset() == exp["ecs"] == ctx.finalize().multiset()
    finally:
        fresh.close()


def test_library_refusals(ka, ctxs, fixture):
    meta, r1, r2 = fixture
    index, ctx = ctxs("host")
    (words, lens, n, max_len), = _batches(ka, ctx, r1[:64], r2[:64], 1, 1)
    with pytest.raises(ka.api.KallistoAmdError, match=r"\(-5\).*shades"):
        ctx.pseudoalign(ka.QuantOpts(1, 200.0, 20.0, 0, 0), words, lens, n, max_len)          # paired with -l / -s
    (w1, l1, n1, ml1), = _batches(ka, ctx, r1[:64], None, 0, 1)
    with pytest.raises(ka.api.KallistoAmdError, match=r"\(-5\).*shades"):
        ctx.pseudoalign(ka.QuantOpts(0, 200.0, 20.0, 0, 0), w1, l1, n1, ml1)                   # --single without --single-overhang
    with pytest.raises(ka.api.KallistoAmdError, match=r"\(-5\).*shades"):
        ctx.pseudoalign_aa(w1, l1, n1, ml1)                                                   # the translated search
    ctx.pseudoalign(ka.QuantOpts(0, 200.0, 20.0, 1, 0), w1, l1, n1, ml1)                       # --single-overhang is fine


def test_bus_bulk_matches_reference(fixture, idx_path, tmp_path):
    meta, r1, r2 = fixture
    gold = os.path.join(common.case_dir(shades.NAME), "bus_pe")
    f1, f2 = str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq")
    _fastq(f1, r1); _fastq(f2, r2)
    out = str(tmp_path / "bus")
    p = subprocess.run([EXE, "bus", "-x", "bulk", "-i", idx_path, "-o", out, "-t", "5", "--batch-size", "1700", *meta["bus_flags"], f1, f2],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    assert "[build] number of shades: %d" % meta["n_shades"] in p.stderr.decode()
    b = open(os.path.join(out, "output.bus"), "rb").read()
    assert b[:4] == b"BUS\0"
    ver, bclen, umilen, tlen = struct.unpack("<IIII", b[4:20])
    assert [ver, bclen, umilen] == meta["bus_header"]
    rec = np.frombuffer(b[20 + tlen:], dtype=BUS_DTYPE)
    keys = list(zip(rec["bc"].tolist(), rec["ec"].tolist()))
    assert keys == sorted(set(keys)), "records must be sorted by (barcode, class) and collapsed"
    ecs = []
    for i, line in enumerate(open(os.path.join(out, "matrix.ec"))):
        e, trs = line.split()
        ids = [int(x) for x in trs.split(",")]
        assert int(e) == i and ids == sorted(set(ids))
        ecs.append(tuple(ids))
    lines = sorted((int(r["bc"]), ecs[int(r["ec"])], int(r["count"])) for r in rec)
    got = ["%d\t%d\t%s" % (bc, n, ",".join(map(str, s))) for bc, s, n in lines]
    with gzip.open(os.path.join(gold, "bus_expected.txt.gz"), "rt") as f:
        want = f.read().split("\n")[:-1]
    assert got == want
    info = json.load(open(os.path.join(out, "run_info.json")))
    for k, v in json.load(open(os.path.join(gold, "run_info.json"))).items():
        assert info[k] == v, k
    assert open(os.path.join(out, "flens.txt")).read() == open(os.path.join(gold, "flens.txt")).read()


def test_cli_quant_and_refusals(fixture, idx_path, tmp_path):
    meta, r1, r2 = fixture
    exp = shades.load_expected("pe")
    f1, f2 = str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq")
    _fastq(f1, r1); _fastq(f2, r2)
    out = str(tmp_path / "out")
    p = subprocess.run([EXE, "quant", "-i", idx_path, "-o", out, "--plaintext", f1, f2], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    assert "[build] number of shades: %d" % meta["n_shades"] in p.stderr.decode()
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(out, "abundance.tsv"))][1:]
    assert [int(r[1]) for r in rows] == exp["lens"].tolist()
    assert np.allclose([float(r[2]) for r in rows], exp["eff"], rtol=1e-5, atol=0)   # (abundance.tsv prints six significant digits)
    got = np.array([float(r[3]) for r in rows])
    # six significant digits in the file: the project's tolerance (1e-4 relative) still applies to what is printed
    want = np.array([float("%.6g" % x) for x in exp["alpha"]])
    common.assert_abundance_close(got, want, "est_counts", floor=1e-6)
    # the combinations the reference itself aborts on: one `Error:` line, exit status 1
    for extra, files in ((["-l", "200", "-s", "20"], [f1, f2]), (["--single", "-l", "200", "-s", "20"], [f1])):
        q = subprocess.run([EXE, "quant", "-i", idx_path, "-o", str(tmp_path / "refused"), "--plaintext", *extra, *files], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        err = q.stderr.decode()
        assert q.returncode == 1 and len([l for l in err.splitlines() if l.startswith("Error:")]) == 1 and "shades" in err, err
    q = subprocess.run([EXE, "bus", "-x", "bulk", "--aa", "-i", idx_path, "-o", str(tmp_path / "aa"), f1], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = q.stderr.decode()
    assert q.returncode == 1 and len([l for l in err.splitlines() if l.startswith("Error:")]) == 1 and "shades" in err, err


def test_no_shaded_state_leaks_into_a_plain_index(ka, idx_path, fixture):
    """one ordinary case before and after a shaded index in the same context: identical results, and the reference's"""
    meta, pidx, p1, p2 = common.load_case("ref_test_pe")
    exp = common.load_expected("ref_test_pe", "pe")
    plain, shaded = ka.Index(pidx), ka.Index(idx_path)
    ctx = ka.Context(0)
    try:
        def run_plain():
            ctx.upload(plain)
            return ka.quant(ctx, ka.QuantOpts(1, 0.0, 0.0, 0, 0), _batches(ka, ctx, p1, p2, 1, 1))
        before = run_plain()
        ctx.upload(shaded)
        _, r1, r2 = fixture
        mid = ka.quant(ctx, ka.QuantOpts(1, 0.0, 0.0, 0, 1), _batches(ka, ctx, r1, r2, 1, 1))
        assert mid.ecs.multiset() == shades.load_expected("pe_fr")["ecs"]
        after = run_plain()
        assert before.ecs.multiset() == after.ecs.multiset() == exp["ecs"]
        assert np.array_equal(before.flens, after.flens) and np.array_equal(before.eff_lens, after.eff_lens)
        assert np.array_equal(before.est_counts, after.est_counts) and before.em_rounds == after.em_rounds
        stats = ctx.stats()
        assert stats["n_single"] + stats["n_multi"] > 0   # the plain index counts sets and tuples again, not explicit records
    finally:
        ctx.close(); plain.close(); shaded.close()
