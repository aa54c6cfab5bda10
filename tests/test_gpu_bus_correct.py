"""Barcode whitelists on the GPU (kamd_bus_whitelist_create, kamd_bus_correct, `bus_sc -w`).  The yardstick is the brute-force restatement of
tests/bus_correct_common.py (a Python set and a loop over the 3 L neighbours), applied to generated records and to the reference's own records
(tests/golden/bus_sc); never the code under test.  Integers only: every comparison is exact."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from tests import bus_correct_common as K
from tests import bus_sc_common as B
from tests import bus_sort_common as S
from tests import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
N_RECORDS = [0, 1, 63, 64, 65, 255, 256, 257, 4 * 65536 + 1234]


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


def _correct(ctx, wl, rec, want_status=True):
    """-> (survivors REC, status or None, the counters of the stats)"""
    res = ctx.bus_correct(wl, _dev(rec), want_status)
    st = {k: v for k, v in res[1].items() if k not in ("ms", "neigh_ms")}
    return _host(res[0]), (res[2].cpu().numpy() if want_status else None), st


def _assert_is_the_restatement(ctx, wl, W, L, rec):
    out, status, st = _correct(ctx, wl, rec)
    want_out, want_status, want_st = K.py_correct(W, L, rec)
    assert st == want_st
    assert np.array_equal(status, want_status)
    assert out.tobytes() == want_out.tobytes()          # every field of every survivor, in input order (pad = the input index)
    return want_st


@pytest.mark.parametrize("L", K.LENGTHS)
def test_whitelist_membership(ctx, L):
    """every key is found, 1000 other barcodes are found exactly when they are keys: read off the status kamd_bus_correct gives them"""
    for size in K.SIZES + [100000]:
        W = K.random_codes(L, size, 1000 * L + size)
        wl = ctx.bus_whitelist(W, L)
        assert wl.stats["n_in"] == len(W) and wl.stats["n_distinct"] == len(set(W.tolist())) and wl.stats["bc_len"] == L
        assert wl.stats["n_buckets"] == int(K.emu().buscorrect_emu_n_buckets(len(W))) and wl.stats["bytes"] == 64 * wl.stats["n_buckets"]
        assert 1 <= wl.stats["max_chain"] <= wl.stats["n_buckets"]
        rng = np.random.default_rng(size)
        rec = K.with_fields(np.concatenate([W, K.rand_barcodes(rng, L, 1000)]), rng)
        _, status, _ = _correct(ctx, wl, rec)
        Wset = set(W.tolist())
        assert np.array_equal(status == K.EXACT, np.array([b in Wset for b in rec["barcode"].tolist()]))
        assert np.all(status[:len(W)] == K.EXACT)
        _assert_is_the_restatement(ctx, wl, W, L, rec)
        wl.free()


def test_duplicates_and_shuffles_give_the_same_corrections(ctx):
    W = K.random_codes(16, 5000, 3)
    rec = K.mixture(W, 16, 20000, 4)
    want = K.py_correct(W, 16, rec)
    rng = np.random.default_rng(5)
    for codes in (W, np.concatenate([W, W[:1000], W[:1000]]), W[rng.permutation(len(W))], W[rng.permutation(len(W))]):
        wl = ctx.bus_whitelist(codes, 16)
        assert wl.stats["n_distinct"] == 5000 and wl.stats["n_in"] == len(codes)
        out, status, st = _correct(ctx, wl, rec)
        assert out.tobytes() == want[0].tobytes() and np.array_equal(status, want[1]) and st == want[2]
        wl.free()


@pytest.mark.parametrize("bucket", [5, 15])
def test_chain_over_several_buckets(ctx, bucket):
    """40 keys with one home bucket in the 16 buckets their table gets: a chain over five buckets; from the last bucket it wraps to bucket 0"""
    L, nb = 16, 16
    W = K.colliding_keys(L, 40, nb, bucket, 10 + bucket)
    others = K.colliding_keys(L, 200, nb, (bucket + 2) % nb, 11)
    near = np.array([K.substitute(np.random.default_rng(i), int(W[i % 40]), L) for i in range(200)], np.uint64)
    rec = K.with_fields(np.concatenate([W, others, near]), np.random.default_rng(12))
    wl = ctx.bus_whitelist(W, L)
    assert (wl.stats["n_distinct"], wl.stats["n_buckets"], wl.stats["max_chain"]) == (40, nb, 5)
    st = _assert_is_the_restatement(ctx, wl, W, L, rec)
    assert st["n_exact"] >= 40 and st["n_corrected"] > 0
    wl.free()


def test_l32_marker_value(ctx, ka):
    L, ones = 32, K.ALL_ONES
    base = K.random_codes(L, 50, 7)
    probes = np.array([0, ones, ones ^ 1, ones ^ (3 << 62), 1, 2 << 62, ones ^ 5] + base[:10].tolist(), np.uint64)
    rec = K.with_fields(np.tile(probes, 20), np.random.default_rng(6))
    for extra in ([0, ones], [], [ones], [0], [ones ^ 1, ones ^ 2]):
        W = np.concatenate([base, np.array(extra, np.uint64)])
        wl = ctx.bus_whitelist(W, L)
        assert wl.stats["n_distinct"] == len(W)
        _assert_is_the_restatement(ctx, wl, W, L, rec)
        wl.free()
    wl = ctx.bus_whitelist(np.array([ones, ones], np.uint64), L)      # the marker value alone, twice
    assert wl.stats["n_distinct"] == 1
    _, status, _ = _correct(ctx, wl, rec[:7])
    assert status.tolist() == [K.UNCORRECTABLE, K.EXACT, K.CORRECTED, K.CORRECTED, K.UNCORRECTABLE, K.UNCORRECTABLE, K.UNCORRECTABLE]
    wl.free()


def test_record_counts(ctx):
    """one block and several, whole and partial wavefronts, no record at all"""
    L = 16
    W = K.random_codes(L, 1000, 20)
    wl = ctx.bus_whitelist(W, L)
    for n in N_RECORDS:
        st = _assert_is_the_restatement(ctx, wl, W, L, K.mixture(W, L, n, 21 + n))
        assert st["n_in"] == n
    assert st["n_exact"] and st["n_corrected"] and st["n_uncorrectable"] and st["n_out"] < st["n_in"]
    wl.free()


MIXTURES = ["all_exact", "all_correctable", "none_survives", "first_dropped", "last_dropped", "every_miss_ambiguous"]


@pytest.mark.parametrize("what", MIXTURES)
def test_mixtures(ctx, what):
    L, n = 16, 3000
    rng = np.random.default_rng(30)
    W = K.random_codes(L, 400, 31)
    bc = W[rng.integers(0, len(W), n)].copy()
    one_off = lambda b: b ^ (rng.integers(1, 4, len(b)).astype(np.uint64) << (2 * rng.integers(0, L, len(b))).astype(np.uint64))
    far = np.uint64(0x55550000)                             # the first eight bases changed: far from every member (the restatement's counters below say so)
    if what == "all_correctable":
        bc = one_off(bc)
    elif what == "none_survives":
        bc ^= far
    elif what == "first_dropped":
        bc[0] ^= far
    elif what == "last_dropped":
        bc[-1] ^= far
    elif what == "every_miss_ambiguous":                    # W holds two neighbours of every probe, the probes themselves are no members
        probes = K.random_codes(L, 200, 32)
        W = np.concatenate([probes ^ np.uint64(1), probes ^ np.uint64(2)])
        bc = np.concatenate([probes[rng.integers(0, 200, n - 500)], W[rng.integers(0, 400, 500)]])[rng.permutation(n)]
    wl = ctx.bus_whitelist(W, L)
    st = _assert_is_the_restatement(ctx, wl, W, L, K.with_fields(bc, rng))
    got = tuple(st[k] for k in K.STAT_KEYS)
    want = {"all_exact": (n, 0, 0, 0), "all_correctable": (0, n, 0, 0), "none_survives": (0, 0, 0, n), "first_dropped": (n - 1, 0, 0, 1),
            "last_dropped": (n - 1, 0, 0, 1), "every_miss_ambiguous": (500, 0, n - 500, 0)}[what]
    assert got == want
    wl.free()


@pytest.mark.parametrize("L", [21, 22, 32])
def test_either_side_of_the_64_neighbour_boundary(ctx, L):
    """3 * 21 = 63 neighbours fit one round of a wavefront, 3 * 22 = 66 need two; a substitution at every position, the last lanes of each round included"""
    W = K.random_codes(L, 300, 40 + L)
    bc = np.array([int(W[i % 300]) ^ (x << (2 * p)) for i, (p, x) in enumerate((p, x) for p in range(L) for x in (1, 2, 3))], np.uint64)
    rng = np.random.default_rng(41)
    rec = K.with_fields(np.concatenate([bc, K.mixture(W, L, 2000, 42)["barcode"]]), rng)
    wl = ctx.bus_whitelist(W, L)
    st = _assert_is_the_restatement(ctx, wl, W, L, rec)
    assert st["n_corrected"] >= 3 * L
    # two members that differ in the first and in the last base from a probe: one hit in each of the two rounds at L >= 22
    probe = int(K.random_codes(L, 1, 43)[0])
    W2 = np.array([probe ^ (1 << (2 * (L - 1))), probe ^ 3], np.uint64)
    wl2 = ctx.bus_whitelist(W2, L)
    _, status, _ = _correct(ctx, wl2, K.with_fields(np.array([probe, probe ^ 3, probe ^ 2], np.uint64), rng))
    assert status.tolist() == [K.AMBIGUOUS, K.EXACT, K.CORRECTED]
    wl.free()
    wl2.free()


def test_high_bits(ctx, ka):
    L = 8
    W = K.random_codes(L, 100, 8)
    w = int(W[0])
    bc = np.array([w, w | 1 << 16, w | 1 << 63, (w ^ 1) | 1 << 16, 1 << 16, K.ALL_ONES] * 50, np.uint64)
    wl = ctx.bus_whitelist(W, L)
    st = _assert_is_the_restatement(ctx, wl, W, L, K.with_fields(bc, np.random.default_rng(9)))
    assert (st["n_exact"], st["n_uncorrectable"]) == (50, 250)
    wl.free()
    for bad, why in ((np.array([w, 1 << 16], np.uint64), "code 1 has a bit set above bit 15"), (np.zeros(0, np.uint64), "empty whitelist")):
        with pytest.raises(ka.KallistoAmdError, match=why):
            ctx.bus_whitelist(bad, L)
    for bad_len in (0, 33):
        with pytest.raises(ka.KallistoAmdError, match=r"must be in \[1, 32\]"):
            ctx.bus_whitelist(W, bad_len)


def test_runs_and_status_argument(ctx, ka):
    """two runs give the same bytes; with and without a status array the records are the same; input and output must not overlap"""
    L = 16
    W = K.random_codes(L, 3000, 50)
    rec = K.mixture(W, L, N_RECORDS[-1], 51)
    wl = ctx.bus_whitelist(W, L)
    a, sa, st_a = _correct(ctx, wl, rec)
    b, sb, st_b = _correct(ctx, wl, rec)
    c, sc, st_c = _correct(ctx, wl, rec, want_status=False)
    assert a.tobytes() == b.tobytes() == c.tobytes() and np.array_equal(sa, sb) and sc is None and st_a == st_b == st_c
    d = _dev(rec)
    n_out = ka.api.C.c_uint64(5)
    rc = ka.load_library().kamd_bus_correct(ctx._h, wl._h, d.data_ptr(), len(rec), d.data_ptr() + 32, None, ka.api.C.byref(n_out), None)
    assert rc == -1 and n_out.value == 0 and b"overlap" in ka.load_library().kamd_last_error()
    assert _host(d).tobytes() == rec.tobytes()
    other = ka.Context(0)                                   # a whitelist belongs to its context
    with pytest.raises(ka.KallistoAmdError, match="whitelist of this context"):
        other.bus_correct(wl, d)
    wl2 = other.bus_whitelist(W, L)                         # ... which frees the ones it still holds when it closes
    other.close()
    wl2.free()
    wl.free()
    with pytest.raises(ka.KallistoAmdError, match="whitelist of this context"):
        ctx.bus_correct(wl, d)


def _same_ecs(a, b):
    return np.array_equal(a.ec_off, b.ec_off) and np.array_equal(a.ec_ids, b.ec_ids) and np.array_equal(a.counts, b.counts)


def _batch(ka, ctx, name, between=None, behind=None):
    """reset -> bus_split -> pseudoalign -> [between] -> finalize -> read_ecs -> bus_records -> [behind]: (device records with batch-local rows, the rows'
    transcript sets, the finalized result, the layout)"""
    import torch
    c = B.CASES[name]
    L, _ = ka.BusLayout.parse(c["tech"])
    opts = ka.QuantOpts(0, 200.0, 20.0, 1, B.case_strand(name), 0, 0)
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


def test_whitelist_and_correct_leave_the_ec_state_alone(ka, world):
    ctx = world("ref_test_pe")
    W = K.random_codes(16, 2000, 60)
    rec = K.mixture(W, 16, 30000, 61)

    def both():
        wl = ctx.bus_whitelist(W, 16)
        _assert_is_the_restatement(ctx, wl, W, 16, rec)
        wl.free()
    _, _, plain, _ = _batch(ka, ctx, "10xv3")
    d_rec, sets, ecs, _ = _batch(ka, ctx, "10xv3", between=both, behind=both)   # between the batch and its finalize, and behind it
    assert ecs.multiset() == plain.multiset()
    assert _same_ecs(ctx.download_ecs(), ecs)
    assert np.array_equal(np.bincount(_host(d_rec)["ec"], minlength=len(sets)), ecs.counts)


def _expected_lines(name):
    """the restatement applied to the reference's golden records -> (W, L, the corrected lines (flags, barcode, umi, set), its counters)"""
    W, L, lines = K.golden_whitelist(name)
    rec = S.make_records([bc for _, bc, _, _ in lines], [u for _, _, u, _ in lines], np.arange(len(lines)), [fl for fl, _, _, _ in lines])
    out, _, st = K.py_correct(W, L, rec)
    return W, L, [(int(r["flags"]), int(r["barcode"]), int(r["umi"]), lines[int(r["ec"])][3]) for r in out], st


@pytest.mark.parametrize("name", K.golden_bc_cases())
def test_chain_on_the_references_records(ka, world, name):
    """split, pseudoalign, finalize, read_ecs, bus_records, bus_correct, bus_sort, bus_count on a golden case: the records and the matrix are the
    restated correction of the reference's own lines, followed by the restated sort and count"""
    from kallisto_amd import bus_sc
    ctx = world(B.CASES[name]["fixture"])
    W, L, want_lines, want_st = _expected_lines(name)
    d_rec, sets, _, layout = _batch(ka, ctx, name)
    wl = ctx.bus_whitelist(np.array(W, np.uint64), L)
    d_cor, st, status = ctx.bus_correct(wl, d_rec, True)
    assert {k: st[k] for k in want_st} == want_st
    assert int((status <= 1).sum()) == st["n_out"] == d_cor.shape[0]
    srt, _ = ctx.bus_sort(d_cor, None, True)
    got = sorted((int(r["flags"]), int(r["barcode"]), int(r["umi"]), sets[int(r["ec"])]) for r in _host(srt) for _ in range(int(r["count"])))
    assert got == sorted(want_lines)
    mode = bus_sc.count_mode(layout)
    c = ctx.bus_count(srt, mode)
    en = np.ascontiguousarray(c["entries"].cpu().numpy()).reshape(-1).view(S.ENTRY)
    matrix = dict(zip(zip(en["row"].tolist(), en["ec"].tolist()), en["value"].tolist()))
    ec_sets = list(sets)
    ec_of = {s: i for i, s in enumerate(ec_sets)}
    dropped = bus_sc.resolve_multi(_host(c["multi"]), matrix, ec_of, ec_sets)
    barcodes = c["barcodes"].cpu().numpy().view(np.uint64).tolist()
    want, n_multi, n_dropped = S.py_matrix([(bc, umi, s, 1) for _, bc, umi, s in want_lines], mode, lambda s: s)
    assert {(barcodes[r], ec_sets[e]): v for (r, e), v in matrix.items()} == want
    assert (c["stats"]["n_multi_groups"], dropped) == (n_multi, n_dropped)
    assert set(barcodes) <= set(W) and barcodes == sorted({bc for _, bc, _, _ in want_lines})
    wl.free()


def _write_fastq(path, reads):
    with open(path, "wb") as f:
        f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))


def _case_files(name, tmp_path):
    c = B.CASES[name]
    L, _, items, _ = B.case_reads(name)
    _, idx, _, _ = common.load_case(c["fixture"])
    files = [str(tmp_path / ("reads_%d.fq" % f)) for f in range(L.n_files)]
    for f, p in enumerate(files):
        _write_fastq(p, [it[f] for it in items])
    return c, idx, files


def _bus_file(path):
    b = open(path, "rb").read()
    assert b[:4] == b"BUS\0"
    ver, bclen, umilen, tlen = np.frombuffer(b[4:20], "<u4").tolist()
    return [ver, bclen, umilen], np.frombuffer(b[20 + tlen:], S.REC)


def _ec_file(path):
    return [tuple(int(x) for x in l.split()[1].split(",")) for l in open(path)]


@pytest.mark.parametrize("name,gz", [("10xv3", False), ("vasa", True)])
def test_driver_with_a_whitelist(ka, name, gz, tmp_path):
    from kallisto_amd import bus_sc
    c, idx, files = _case_files(name, tmp_path)
    meta, _ = B.load_golden(name)
    W, L, want_lines, want_st = _expected_lines(name)
    wpath = str(tmp_path / ("whitelist.txt.gz" if gz else "whitelist.txt"))
    with (gzip.open(wpath, "wb") if gz else open(wpath, "wb")) as f:
        f.write(K.whitelist_text(W, L, "\r\n" if gz else "\n"))
    out = str(tmp_path / "out")
    assert bus_sc.main(["-x", c["tech"], "-i", idx, "-o", out, "-w", wpath, "--count", *c["flags"], *files]) == 0
    hdr, rec = _bus_file(os.path.join(out, "output.bus"))
    ecs = _ec_file(os.path.join(out, "matrix.ec"))
    ec_of = {s: i for i, s in enumerate(ecs)}
    exp = S.make_records([bc for _, bc, _, _ in want_lines], [u for _, _, u, _ in want_lines], [ec_of[s] for _, _, _, s in want_lines], [fl for fl, _, _, _ in want_lines])
    exp = S.np_collapse(S.np_sort(exp))[0]
    assert hdr == meta["bus_header"] and rec.tobytes() == exp.tobytes()
    counters = json.load(open(os.path.join(out, "correct.json")))
    assert counters == {k: want_st[k] for k in K.STAT_KEYS}
    info = json.load(open(os.path.join(out, "run_info.json")))
    assert info["n_pseudoaligned"] == meta["n_pseudoaligned"] and info["n_processed"] == meta["n_processed"] and not set(counters) & set(info)
    cd = os.path.join(out, "counts")
    listed = open(os.path.join(cd, "output.barcodes.txt")).read().split("\n")[:-1]
    assert set(listed) <= {K.decode(w, L) for w in W} and listed == [K.decode(b, L) for b in sorted({bc for _, bc, _, _ in want_lines})]
    q = str(tmp_path / "q")
    p = subprocess.run([EXE, "quant-tcc", "-i", idx, "-e", os.path.join(cd, "output.ec.txt"), "-o", q, os.path.join(cd, "output.mtx")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    ab = [l for l in open(os.path.join(q, "matrix.abundance.mtx")) if not l.startswith("%")]
    assert int(ab[0].split()[0]) == len(listed)


def test_driver_refusals(ka, tmp_path, capsys):
    from kallisto_amd import bus_sc
    _, idx, _, _ = common.load_case("ref_test_pe")
    w8, w16 = str(tmp_path / "w8.txt"), str(tmp_path / "w16.txt")
    open(w8, "wb").write(K.whitelist_text(K.random_codes(8, 20, 1), 8))
    open(w16, "wb").write(K.whitelist_text(K.random_codes(16, 20, 1), 16))
    for tech, w, why in (("0,0,0:0,0,10:1,0,0", w8, "open-ended"), ("-1,-1,-1:0,0,10:1,0,0", w8, "has no barcode"),
                         ("10XV3", w8, r"barcode length of whitelist \(8\) differs from the technology's \(16\)"),
                         ("0,0,8:0,8,16:1,0,0", w16, r"barcode length of whitelist \(16\) differs from the technology's \(8\)")):
        with pytest.raises(ka.KallistoAmdError, match=why):
            bus_sc.run(tech, idx, str(tmp_path / "never"), ["a.fq", "b.fq"], whitelist=w)
    assert bus_sc.main(["-x", "10XV3", "-i", idx, "-o", str(tmp_path / "never"), "-w", w8, "a.fq", "b.fq"]) == 1
    assert "barcode length of whitelist (8) differs from the technology's (16)" in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "never"))


def test_driver_without_a_whitelist_is_unchanged(ka, tmp_path):
    """no -w: the records are the reference's, as tests/test_gpu_bus_sc.py expects them, the same bytes whether the argument is left out or None,
    and no correct.json"""
    from kallisto_amd import bus_sc
    name = "10xv3"
    c, idx, files = _case_files(name, tmp_path)
    meta, want = B.load_golden(name)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert bus_sc.main(["-x", c["tech"], "-i", idx, "-o", a, *c["flags"], *files]) == 0
    info = bus_sc.run(c["tech"], idx, b, files, whitelist=None)
    assert open(os.path.join(a, "output.bus"), "rb").read() == open(os.path.join(b, "output.bus"), "rb").read()
    hdr, rec = _bus_file(os.path.join(a, "output.bus"))
    ecs = _ec_file(os.path.join(a, "matrix.ec"))
    assert hdr == meta["bus_header"]
    assert sorted((int(r["flags"]), int(r["barcode"]), int(r["umi"]), ecs[int(r["ec"])]) for r in rec for _ in range(int(r["count"]))) == want
    ec_of = {s: i for i, s in enumerate(ecs)}
    exp = S.make_records([bc for _, bc, _, _ in want], [u for _, _, u, _ in want], [ec_of[s] for _, _, _, s in want], [fl for fl, _, _, _ in want])
    assert rec.tobytes() == S.np_collapse(S.np_sort(exp))[0].tobytes()
    assert not os.path.exists(os.path.join(a, "correct.json")) and not set(K.STAT_KEYS) & set(info)
