"""Per-read equivalence classes on the GPU (kamd_read_ecs, `bus -n`).  The yardsticks are the oracle's per-read transcript sets
(oracle.Index.pseudoalign), the finalized counts (held to the reference by the parity tests) and the reference's own `bus -n` output
(tests/golden/bus_num); never the code under test."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bigsets, common, shades
from tests import read_ecs_common as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
BUS_DTYPE = np.dtype([("bc", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])

PARITY = [("ref_test_pe", "pe"), ("yeast_se", "se"), ("tiny_k7_se", "se"), ("mosaic_pe", "pe_rf"), ("mosaic_pe", "se"), ("mosaic_pe", "pe_union"),
          ("mosaic_pe", "pe_nojump"), ("dlist_pe", "pe"), ("k17_pe", "pe"), ("stress_pe", "pe")]
HISTOGRAM = PARITY + [("shades_pe", "pe"), ("shades_pe", "pe_fr"), ("shades_pe", "pe_union"), ("bigsets_pe", "pe"), ("bigsets_pe", "se")]


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    kallisto_amd.load_library()
    return kallisto_amd


def _load(case, tmp):
    if case == "shades_pe":
        meta, r1, r2 = shades.load_reads()
        return meta, shades.unpack_index(tmp), r1, r2
    if case == "bigsets_pe":
        meta, r1, r2 = bigsets.load_reads()
        return meta, bigsets.unpack_index(tmp), r1, r2
    return common.load_case(case)


@pytest.fixture(scope="module")
def world(ka, tmp_path_factory):
    """one context per fixture, and per (fixture, variant) one run: pseudoalign, finalize, read_ecs on the same batch.  Computed once, shared, not modified."""
    ctxs, runs = {}, {}

    def ctx_of(case):
        if case not in ctxs:
            meta, idx, r1, r2 = _load(case, tmp_path_factory.mktemp(case))
            ctx = ka.Context(0)
            ctx.upload(ka.Index(idx))
            ctxs[case] = (ctx, meta, r1, r2)
        return ctxs[case]

    def batch(case, variant, lo=0, hi=None):
        ctx, meta, r1, r2 = ctx_of(case)
        o = common.parse_variant(meta["variants"][variant])
        opts = ka.QuantOpts(o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"])
        hi = len(r1) if hi is None else hi
        reads = common.interleave(r1[lo:hi], r2[lo:hi] if o["paired"] else None)
        max_len = max(max(len(x) for x in r1), max(len(x) for x in r2) if o["paired"] else 0)   # (one record layout for every cut of the fixture)
        words, lens, max_len = ctx.pack_reads_host(reads, max_len)
        return ctx, opts, o, (words, lens, hi - lo, max_len)

    def run(case, variant, live=False):
        """live: the context must hold this run's result afterwards (a context serves all variants of its fixture): computed again"""
        if live or (case, variant) not in runs:
            ctx, opts, o, b = batch(case, variant)
            ctx.reset()
            ctx.track_order(False)
            ctx.debug_read_ecs(0, 0)
            ctx.pseudoalign(opts, *b)
            ecs = ctx.finalize()
            d_ec, st = ctx.read_ecs(opts, *b)
            runs[(case, variant)] = (ecs, d_ec.cpu().numpy().copy(), st, ctx.debug_read_ecs(0, 0))
        return runs[(case, variant)]

    class W:
        pass
    w = W()
    w.ctx_of, w.batch, w.run = ctx_of, batch, run
    yield w
    for c in ctxs.values():
        c[0].close()


def _rows(ecs):
    return [tuple(ecs.ec_ids[int(ecs.ec_off[i]):int(ecs.ec_off[i + 1])].tolist()) for i in range(len(ecs.counts))]


def _ids(ecs, d):
    """the transcript set every item was looked up to: () for NONE; FOREIGN is kept as the string"""
    rows = _rows(ecs)
    return [() if x == R.NONE else ("FOREIGN" if x == R.FOREIGN else rows[x]) for x in d.tolist()]


def _oracle(case, o):
    return R.oracle_sets(case, (o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"]))


@pytest.mark.parametrize("case,variant", PARITY)
def test_every_read_gets_the_oracles_set(case, variant, world):
    ecs, d, st, dbg = world.run(case, variant)
    _, _, o, _ = world.batch(case, variant, 0, 1)
    want = list(_oracle(case, o))
    got = _ids(ecs, d)
    assert len(got) == len(want) == st["n_items"]
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:3])
    assert st["n_foreign"] == 0 and st["n_none"] == sum(1 for w in want if not w) and st["n_mapped"] == st["n_items"] - st["n_none"]


@pytest.mark.parametrize("case,variant", HISTOGRAM)
def test_histogram_equals_the_finalized_counts(case, variant, world):
    ecs, d, st, dbg = world.run(case, variant)
    assert st["n_foreign"] == 0 and not np.any(d == R.FOREIGN)
    assert np.all(d >= R.NONE) and np.all(d < len(ecs.counts))
    assert np.array_equal(np.bincount(d[d >= 0], minlength=len(ecs.counts)), ecs.counts.astype(np.int64))
    assert st["n_mapped"] == int(ecs.counts.sum()) and st["n_mapped"] + st["n_none"] == st["n_items"] == len(d)


@pytest.mark.parametrize("case,variant", [("stress_pe", "pe"), ("mosaic_pe", "pe_union"), ("mosaic_pe", "pe_rf"), ("bigsets_pe", "pe")])
def test_second_tier_gives_the_same(case, variant, world):
    """a first tier of two list entries: every item whose hits carry three or more distinct sets is re-run by the second launch"""
    ecs, d, st, _ = world.run(case, variant, live=True)
    ctx, opts, o, b = world.batch(case, variant)
    ctx.debug_read_ecs(0, 2)
    try:
        d2, st2 = ctx.read_ecs(opts, *b)
        n_second = ctx.debug_read_ecs(0, 0)["n_second_tier"]
    finally:
        ctx.debug_read_ecs(0, 0)
    assert n_second > 0, "the fixture no longer has items with more than two sets"
    assert np.array_equal(d2.cpu().numpy(), d) and {k: v for k, v in st2.items() if k != "ms"} == {k: v for k, v in st.items() if k != "ms"}


CHUNK = 96


@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1])
def test_batch_shapes(n, world):
    case, variant = "ref_test_pe", "pe"
    ecs, d, _, _ = world.run(case, variant, live=True)
    ctx, opts, o, b = world.batch(case, variant, 0, n)
    ctx.debug_read_ecs(CHUNK, 0)
    try:
        dn, st = ctx.read_ecs(opts, *b)
    finally:
        ctx.debug_read_ecs(0, 0)
    assert st["n_items"] == n and np.array_equal(dn.cpu().numpy(), d[:n])


@pytest.mark.parametrize("chunk", [0, 1000])
def test_one_call_against_five_uneven_calls(chunk, world):
    case, variant = "mosaic_pe", "pe_rf"
    ecs, d, st, _ = world.run(case, variant, live=True)
    n = len(d)
    cuts = [0, 1, 778, 779, 2500, n]
    ctx, opts, _, _ = world.batch(case, variant, 0, 1)
    ctx.debug_read_ecs(chunk, 0)
    try:
        parts, tot = [], dict(n_items=0, n_mapped=0, n_none=0, n_foreign=0)
        for a, b in zip(cuts[:-1], cuts[1:]):
            _, _, _, bt = world.batch(case, variant, a, b)
            dp, sp = ctx.read_ecs(opts, *bt)
            parts.append(dp.cpu().numpy())
            for k in tot:
                tot[k] += sp[k]
    finally:
        ctx.debug_read_ecs(0, 0)
    assert np.array_equal(np.concatenate(parts), d)
    assert tot == {k: st[k] for k in tot}


def test_first_occurrence_order(world, ka):
    case, variant = "ref_test_pe", "pe"
    ctx, opts, o, b = world.batch(case, variant)
    ctx.reset()
    ctx.track_order(True)
    try:
        ctx.pseudoalign(opts, *b)
        ecs = ctx.finalize()
        d = ctx.read_ecs(opts, *b)[0].cpu().numpy()
    finally:
        ctx.reset()
        ctx.track_order(False)
    m = d[d >= 0]
    _, first = np.unique(m, return_index=True)
    assert m[np.sort(first)].tolist() == list(range(len(ecs.counts)))
    assert _ids(ecs, d) == list(_oracle(case, o))


def test_state_is_untouched_and_the_table_follows_the_result(world, ka):
    import torch
    case, variant = "ref_test_pe", "pe"
    ref, _, _, _ = world.run(case, variant)   # (first: it uses the same context)
    want = list(_oracle(case, common.parse_variant([])))
    ctx, opts, o, b1 = world.batch(case, variant, 0, 300)
    _, _, _, b2 = world.batch(case, variant, 300, None)
    _, _, _, ball = world.batch(case, variant)
    ctx.reset()
    ctx.pseudoalign(opts, *b1)
    e1 = ctx.finalize()
    dense1 = ctx.dense_counts().clone()
    d1, st1 = ctx.read_ecs(opts, *b1)
    after = ctx.download_ecs()
    assert np.array_equal(after.ec_off, e1.ec_off) and np.array_equal(after.ec_ids, e1.ec_ids) and np.array_equal(after.counts, e1.counts)
    assert torch.equal(ctx.dense_counts(), dense1)
    assert _ids(e1, d1.cpu().numpy()) == want[:300] and st1["n_foreign"] == 0
    # a batch that never went into the result: its sets are served where the result holds them, FOREIGN elsewhere, () stays NONE
    dx, stx = ctx.read_ecs(opts, *b2)
    have = set(_rows(e1))
    gx = _ids(e1, dx.cpu().numpy())
    assert gx == [w if (not w or w in have) else "FOREIGN" for w in want[300:]]
    assert stx["n_foreign"] == sum(1 for g in gx if g == "FOREIGN") > 0
    # a further batch and a second finalize: the counts of both, and a look-up that is right for both (the table was rebuilt)
    ctx.pseudoalign(opts, *b2)
    e2 = ctx.finalize()
    assert e2.multiset() == ref.multiset()
    dall, stall = ctx.read_ecs(opts, *ball)
    assert _ids(e2, dall.cpu().numpy()) == want and stall["n_foreign"] == 0
    assert np.array_equal(np.bincount(dall.cpu().numpy()[dall.cpu().numpy() >= 0], minlength=len(e2.counts)), e2.counts.astype(np.int64))
    # set_counts keeps the table
    ctx.ec_set_counts(np.zeros(len(e2.counts), np.uint32))
    assert np.array_equal(ctx.read_ecs(opts, *ball)[0].cpu().numpy(), dall.cpu().numpy())


def test_reset_and_another_result(world, ka):
    """after reset() there is no result (the call says so); after a result from other reads of the fixture the old ids are not served"""
    case, variant = "yeast_se", "se"
    ctx, opts, o, ba = world.batch(case, variant, 0, 3000)
    _, _, _, bb = world.batch(case, variant, 3000, None)
    want = list(_oracle(case, o))
    ctx.reset()
    ctx.pseudoalign(opts, *ba)
    ea = ctx.finalize()
    da = ctx.read_ecs(opts, *ba)[0].cpu().numpy()
    assert _ids(ea, da) == want[:3000]
    ctx.reset()
    with pytest.raises(ka.KallistoAmdError, match="no EC result"):
        ctx.read_ecs(opts, *ba)
    ctx.pseudoalign(opts, *bb)
    with pytest.raises(ka.KallistoAmdError, match="no EC result"):   # (pseudoaligned, not finalized)
        ctx.read_ecs(opts, *bb)
    eb = ctx.finalize()
    have = set(_rows(eb))
    assert _ids(eb, ctx.read_ecs(opts, *bb)[0].cpu().numpy()) == want[3000:]
    assert _ids(eb, ctx.read_ecs(opts, *ba)[0].cpu().numpy()) == [w if (not w or w in have) else "FOREIGN" for w in want[:3000]]


def test_read_ecs_before_any_finalize_raises(ka):
    _, idx, r1, r2 = common.load_case("tiny_k7_se")
    ctx = ka.Context(0)
    try:
        ctx.upload(ka.Index(idx))
        words, lens, max_len = ctx.pack_reads_host(r1[:10])
        with pytest.raises(ka.KallistoAmdError, match="kamd_read_ecs: no EC result"):
            ctx.read_ecs(ka.QuantOpts(0, 40.0, 5.0, 0, 0), words, lens, 10, max_len)
    finally:
        ctx.close()


def test_uploaded_subset_of_the_classes(world, ka):
    case, variant = "ref_test_pe", "pe"
    ecs, d, _, _ = world.run(case, variant)
    rows = _rows(ecs)   # (only the sets matter: the upload below replaces the context's result)
    keep = [r for i, r in enumerate(rows) if i % 3 != 1][::-1]   # two thirds of the classes, in another order
    ctx, opts, o, b = world.batch(case, variant)
    off, ids = R.csr(keep)
    ctx.ec_upload(off, ids[:-1])
    try:
        du, st = ctx.read_ecs(opts, *b)
    finally:
        ctx.reset()
    du = du.cpu().numpy()
    kept = set(keep)
    want = list(_oracle(case, o))
    got = [() if x == R.NONE else ("FOREIGN" if x == R.FOREIGN else keep[x]) for x in du.tolist()]
    assert got == [w if (not w or w in kept) else "FOREIGN" for w in want]
    assert st["n_foreign"] == sum(1 for g in got if g == "FOREIGN") > 0


# ---- bus -n -------------------------------------------------------------------------------------------------------------------------------------
def _fastq(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def _read_bus(path):
    b = open(path, "rb").read()
    assert b[:4] == b"BUS\0"
    ver, bclen, umilen, tlen = struct.unpack("<IIII", b[4:20])
    assert (len(b) - 20 - tlen) % 32 == 0
    return [ver, bclen, umilen], np.frombuffer(b[20 + tlen:], dtype=BUS_DTYPE)


def _read_ec(path):
    return [tuple(int(x) for x in line.split()[1].split(",")) for line in open(path)]


def _run_bus(meta, tmp_path, out, extra):
    _, idx, r1, r2 = common.load_case(meta["fixture"])
    paired = "--paired" in meta["bus_flags"]
    files = []
    for s, (bc, a, b) in enumerate(R.samples_of(meta)):
        fs = [str(tmp_path / ("s%d_1.fq" % s))]
        _fastq(fs[0], r1[a:b])
        if paired:
            fs.append(str(tmp_path / ("s%d_2.fq" % s)))
            _fastq(fs[1], r2[a:b])
        files.append(fs)
    if meta["batch_ids"] is None:
        inputs = [f for fs in files for f in fs]
    else:
        bf = str(tmp_path / "batch.txt")
        with open(bf, "w") as f:
            for i, fs in zip(meta["batch_ids"], files):
                f.write(" ".join([i] + fs) + "\n")
        inputs = ["-B", bf]
    p = subprocess.run([EXE, "bus", "-x", "bulk", "-i", idx, "-o", str(tmp_path / out), "-t", "4", "--batch-size", "700", *meta["bus_flags"], *extra, *inputs],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, KAMD_FASTQ_CHUNK="3000"))
    assert p.returncode == 0, p.stderr.decode()
    return str(tmp_path / out)


@pytest.mark.parametrize("case", R.BUS_CASES)
def test_bus_num_matches_the_reference(case, tmp_path):
    assert os.path.exists(EXE), "build kallisto_amd_quant with `make -C kallisto_amd/csrc all`"
    meta, want = R.load_bus_case(case)
    out = _run_bus(meta, tmp_path, "num", ["-n"])
    plain = _run_bus(meta, tmp_path, "plain", [])
    hdr, rec = _read_bus(os.path.join(out, "output.bus"))
    assert hdr == meta["bus_header"] == [1, 16, 1]
    assert np.all(rec["count"] == 1) and np.all(rec["umi"] == np.uint64(2 ** 64 - 1)) and np.all(rec["pad"] == 0)
    keys = list(zip(rec["bc"].tolist(), rec["umi"].tolist(), rec["ec"].tolist(), rec["flags"].tolist()))
    assert keys == sorted(keys), "records must be sorted by (barcode, UMI, class, flags)"
    ecs = _read_ec(os.path.join(out, "matrix.ec"))
    got = sorted((int(r["flags"]), int(r["bc"]), ecs[int(r["ec"])]) for r in rec)
    assert got == want
    for fn in ["matrix.cells"] + (["flens.txt"] if "--paired" in meta["bus_flags"] else []):
        assert open(os.path.join(out, fn), "rb").read() == open(os.path.join(plain, fn), "rb").read(), fn
    # matrix.ec: the same classes.  Their numbers are the order in which a sample's finalized rows come back, which without kamd_ec_track_order is
    # not the same from one run to the next (with or without -n), so the files are compared with the numbering taken out -- and through it the
    # records of both runs: per (barcode, class) as many records here as the plain run counts
    ecs_plain = _read_ec(os.path.join(plain, "matrix.ec"))
    assert len(ecs) == len(ecs_plain) == len(set(ecs)) and set(ecs) == set(ecs_plain)
    _, rec_plain = _read_bus(os.path.join(plain, "output.bus"))
    hist = {}
    for r in rec:
        k = (int(r["bc"]), ecs[int(r["ec"])])
        hist[k] = hist.get(k, 0) + 1
    assert hist == {(int(r["bc"]), ecs_plain[int(r["ec"])]): int(r["count"]) for r in rec_plain}
    ia, ib = (json.load(open(os.path.join(d, "run_info.json"))) for d in (out, plain))
    for k in ("start_time", "call"):
        ia.pop(k), ib.pop(k)
    assert ia == ib and ia["n_pseudoaligned"] == len(rec) == meta["n_records"]
