"""Barcode / UMI technologies on the GPU (kamd_bus_split, kamd_bus_records, kallisto_amd.bus_sc).  The yardsticks are the CPU build of the per-item
rules (tests/emu_bustag), the Python restatement of them with the host packer (tests/bus_sc_common.py), and the reference's own `bus -x` output
(tests/golden/bus_sc); never the code under test.  Integers only: every comparison is exact."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bus_sc_common as B
from tests import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUS_DTYPE = np.dtype([("bc", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
NONE, FOREIGN = -1, -2


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    kallisto_amd.load_library()
    return kallisto_amd


@pytest.fixture(scope="module")
def world(ka):
    """one context per fixture index (uploaded once), shared by the tests; a test that needs an EC state resets it first"""
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


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    v = a.view(np.int32) if a.dtype == np.uint32 else (a.view(np.int16) if a.dtype == np.uint16 else a)
    return torch.from_numpy(v.copy()).to("cuda:0")


def _split(ka, ctx, tech, words, lens, n, max_len, seq_max_len=None):
    """Context.bus_split on host arrays -> host arrays in the emu's form, and the device dict"""
    from kallisto_amd import api as A
    L, _ = ka.BusLayout.parse(tech)
    sp = ctx.bus_split(L, _dev(words), _dev(lens), n, max_len, seq_max_len)
    st = {k: v for k, v in sp["stats"].items() if k != "ms"}
    return (A.bus_tags_numpy(sp["tags"]), sp["src"].cpu().numpy().view(np.uint32), sp["seq_words"].cpu().numpy().view(np.uint32),
            sp["seq_len"].cpu().numpy().view(np.uint16), st, sp["seq_max_len"]), sp


def _assert_equals_emu(ka, ctx, tech, words, lens, n, max_len, seq_max_len=None):
    L, _ = B.parse(tech)
    want = B.emu_split(L, words, lens, n, max_len, seq_max_len)
    got, sp = _split(ka, ctx, tech, words, lens, n, max_len, seq_max_len)
    assert got[4] == want[4]                                  # the statistics: survivors, drops, both histograms, the longest cut
    assert got[5] == want[5]
    assert np.array_equal(got[0], want[0].view(got[0].dtype))   # tags, every field
    assert np.array_equal(got[1], want[1])                    # the input item of every compact item
    assert np.array_equal(got[3], want[3])
    assert np.array_equal(got[2], want[2])                    # the cut batch, every word
    return want, sp


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_split_equals_emu_and_host_packer(ka, world, name):
    ctx = world(B.CASES[name]["fixture"])
    L, _, items, _ = B.case_reads(name)
    words, lens, n, max_len = B.case_batch(name)
    want, _ = _assert_equals_emu(ka, ctx, B.CASES[name]["tech"], words, lens, n, max_len)
    # ... and the cut batch is what the host packer makes of the substrings cut in Python, mask and padding words included
    surv, pst = B.py_split(L.as_dict(), items)
    assert want[4] == pst
    w, l, _ = B.pack_host([d["seq"] for _, d in surv], want[5])
    assert np.array_equal(want[2], w) and np.array_equal(want[3], l)
    if name in ("10xv3", "indropsv2"):   # the two files' longest reads differ, one way and the other: one record stride for both
        by_file = [max(len(it[f]) for it in items) for f in (0, 1)]
        assert by_file[0] != by_file[1] and max_len == max(by_file)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_split_small_batches(ka, world, n):
    ctx = world("ref_test_pe")
    words, lens, _, max_len = B.case_batch("10xv3")
    rw = B.record_words(max_len)
    for first in (0, 11):   # (item 11 of the case is a dropped one: a batch that begins with a drop)
        _assert_equals_emu(ka, ctx, "10XV3", words[first * 2 * rw:(first + n) * 2 * rw], lens[first * 2:(first + n) * 2], n, max_len)


def test_split_scan_across_blocks(ka, world):
    """4 x 65 536 + 1 234 items, the case's records tiled on the device: more than a thousand blocks, several trips of the scan's carry"""
    import torch
    from kallisto_amd import api as A
    ctx = world("ref_test_pe")
    words, lens, n0, max_len = B.case_batch("10xv3")
    n = 4 * 65536 + 1234
    reps = -(-n // n0)
    rw = B.record_words(max_len)
    dw = _dev(words).repeat(reps)[:n * 2 * rw].contiguous()
    dl = _dev(lens).repeat(reps)[:n * 2].contiguous()
    L, _ = ka.BusLayout.parse("10XV3")
    sp = ctx.bus_split(L, dw, dl, n, max_len)
    Le, _ = B.parse("10XV3")
    want = B.emu_split(Le, np.tile(words, reps)[:n * 2 * rw], np.tile(lens, reps)[:n * 2], n, max_len)
    assert {k: v for k, v in sp["stats"].items() if k != "ms"} == want[4]
    assert np.array_equal(A.bus_tags_numpy(sp["tags"]), want[0].view(A.BUS_TAG_DTYPE))
    assert np.array_equal(sp["src"].cpu().numpy().view(np.uint32), want[1])
    assert np.array_equal(sp["seq_len"].cpu().numpy().view(np.uint16), want[3])
    assert np.array_equal(sp["seq_words"].cpu().numpy().view(np.uint32), want[2])


def test_split_all_none_first_last_dropped(ka, world):
    ctx = world("ref_test_pe")
    _, _, items, names = B.case_reads("10xv3")
    good = [it for it, nm in zip(items, names) if nm not in ("short_bc", "short_umi")][:300]
    bad = [it for it, nm in zip(items, names) if nm in ("short_bc", "short_umi")][:300]
    for what, batch in (("all", bad), ("none", good), ("first", bad[:1] + good), ("last", good + bad[:1]), ("first and last", bad[:1] + good + bad[1:2])):
        w, l, max_len = B.pack_host([r for it in batch for r in it])
        want, _ = _assert_equals_emu(ka, ctx, "10XV3", w, l, len(batch), max_len)
        assert want[4]["n_valid"] == {"all": 0, "none": 300, "first": 300, "last": 300, "first and last": 300}[what], what


@pytest.mark.parametrize("start", [0, 1, 15, 16, 17, 31, 32, 33])
def test_split_repack_corners(ka, world, start):
    """cuts that begin at, before and behind a word (16 bases) and a mask-word (32 bases) boundary; len - start of 0, 1, 16, 32 and the sizes around;
    Ns inside and outside the cut; an open end and a stop; seq_max_len exact and larger than needed"""
    ctx = world("ref_test_pe")
    rnd = B.lcg(2000 + start)
    items = []
    for n in (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 90):
        for rep in range(3):
            s = bytearray(b"ACGT"[next(rnd) % 4] for _ in range(start + n))
            for _ in range(rep * 2):
                if s:
                    s[next(rnd) % len(s)] = ord("N")
            items.append((b"ACGTACGTAACCGGTT", bytes(s)))
    w, l, max_len = B.pack_host([r for it in items for r in it])
    for tech in ("0,0,8:0,8,16:1,%d,0" % start, "0,0,8:0,8,16:1,%d,%d" % (start, start + 32), "0,0,8:0,8,16:1,%d,%d" % (start, start + 1)):
        for sml in (None, 150):
            want, _ = _assert_equals_emu(ka, ctx, tech, w, l, len(items), max_len, sml)
            L, _ = B.parse(tech)
            surv, _ = B.py_split(L.as_dict(), items)
            pw, pl, _ = B.pack_host([d["seq"] for _, d in surv], want[5])
            assert np.array_equal(want[2], pw) and np.array_equal(want[3], pl)


def _tags(n, seed):
    rnd = B.lcg(seed)
    t = np.zeros(n, B.TAG_DTYPE)
    t["barcode"] = [next(rnd) for _ in range(n)]
    t["umi"] = np.arange(n, dtype=np.uint64) << np.uint64(3)
    t["flags"] = np.arange(n, dtype=np.uint32) % 1021
    t["bc_len"], t["umi_len"] = 16, 12
    return t


@pytest.mark.parametrize("n,kind", [(1, "none_none"), (1, "all_none"), (300, "all_none"), (300, "none_none"), (300, "mixed"), (65537, "mixed"), (65537, "none_none")])
def test_records_compaction(ka, world, n, kind):
    import torch
    from kallisto_amd import api as A
    ctx = world("ref_test_pe")
    tags = _tags(n, 7 + n)
    rnd = B.lcg(n)
    ec = np.array([next(rnd) % 5000 for _ in range(n)], np.int32)
    if kind == "all_none":
        ec[:] = NONE
    elif kind == "mixed":
        ec[np.array([next(rnd) % 3 == 0 for _ in range(n)])] = NONE
        ec[0], ec[-1] = NONE, 17
    d_tags = torch.from_numpy(tags.view(np.int64).reshape(n, 3).copy()).to("cuda:0")
    rec = A.bus_records_numpy(ctx.bus_records(d_tags, _dev(ec), n))
    keep = ec >= 0
    assert len(rec) == int(keep.sum())
    assert np.array_equal(rec["barcode"], tags["barcode"][keep]) and np.array_equal(rec["umi"], tags["umi"][keep])   # order preserved
    assert np.array_equal(rec["ec"], ec[keep]) and np.array_equal(rec["flags"], tags["flags"][keep])
    assert np.all(rec["count"] == 1) and np.all(rec["pad"] == 0)


def test_records_foreign_row_is_an_error(ka, world):
    import torch
    ctx = world("ref_test_pe")
    n = 1000
    tags = _tags(n, 3)
    ec = np.arange(n, dtype=np.int32)
    ec[777] = FOREIGN
    d_tags = torch.from_numpy(tags.view(np.int64).reshape(n, 3).copy()).to("cuda:0")
    out = torch.full((n, 4), -1, dtype=torch.int64, device="cuda:0")
    n_out = ka.api.C.c_uint64(123)
    rc = ka.load_library().kamd_bus_records(ctx._h, d_tags.data_ptr(), _dev(ec).data_ptr(), n, out.data_ptr(), ka.api.C.byref(n_out))
    assert rc == -4 and n_out.value == 0
    assert b"KAMD_READ_EC_FOREIGN" in ka.load_library().kamd_last_error()
    assert bool((out == -1).all())   # no record written
    with pytest.raises(ka.KallistoAmdError, match="not part of the finalized EC result"):
        ctx.bus_records(d_tags, _dev(ec), n)


def _rows(ecs):
    return [tuple(ecs.ec_ids[int(ecs.ec_off[i]):int(ecs.ec_off[i + 1])].tolist()) for i in range(len(ecs.counts))]


def _same_ecs(a, b):
    return np.array_equal(a.ec_off, b.ec_off) and np.array_equal(a.ec_ids, b.ec_ids) and np.array_equal(a.counts, b.counts)


def _run_batch(ka, ctx, L, opts, dw, dl, n, max_len, check_state=False):
    """reset -> bus_split -> pseudoalign -> finalize -> read_ecs -> bus_records -> [(flags, barcode, umi, transcript set)] of the batch"""
    from kallisto_amd import api as A
    ctx.reset()
    sp = ctx.bus_split(L, dw, dl, n, max_len)
    nv = sp["n_valid"]
    if nv == 0:
        return [], sp["stats"]
    cut = (sp["seq_words"], sp["seq_len"], nv, sp["seq_max_len"])
    ctx.pseudoalign(opts, *cut)
    if check_state:   # a bus_split and a bus_records between the batch and its finalize leave the EC state alone
        sp2 = ctx.bus_split(L, dw, dl, n, max_len)
        ctx.bus_records(sp2["tags"], _dev(np.full(nv, NONE, np.int32)), nv)
    ecs = ctx.finalize()
    d_ec, st = ctx.read_ecs(opts, *cut)
    rec = A.bus_records_numpy(ctx.bus_records(sp["tags"], d_ec, nv))
    rows = _rows(ecs)
    assert int(ecs.counts.sum()) == len(rec) == st["n_mapped"]
    if check_state:   # ... and so do they behind it: the result the context holds is the one finalize described
        ctx.bus_split(L, dw, dl, n, max_len)
        assert _same_ecs(ctx.download_ecs(), ecs)
        hist = np.bincount(rec["ec"], minlength=len(rows))
        assert np.array_equal(hist, ecs.counts)
    return [(int(r["flags"]), int(r["barcode"]), int(r["umi"]), rows[int(r["ec"])]) for r in rec], sp["stats"]


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_end_to_end_equals_the_reference(ka, world, name):
    c = B.CASES[name]
    ctx = world(c["fixture"])
    meta, want = B.load_golden(name)
    L, _ = ka.BusLayout.parse(c["tech"])
    opts = ka.QuantOpts(0, 200.0, 20.0, 1, B.case_strand(name), 0, 0)
    words, lens, n, max_len = B.case_batch(name)
    dw, dl = _dev(words), _dev(lens)
    rw = B.record_words(max_len) * L.n_files
    got, st = _run_batch(ka, ctx, L, opts, dw, dl, n, max_len, check_state=True)
    assert sorted(got) == want
    assert st["n_valid"] == meta["n_processed"]
    assert (1,) + L.header_lens(st["bc_len_hist"], st["umi_len_hist"]) == tuple(meta["bus_header"])
    # five uneven batches: class ids are batch-local, the records are merged by transcript set
    cuts = [int(round(f * n)) for f in (0.0, 0.07, 0.3, 0.31, 0.8, 1.0)]
    merged, n_valid = [], 0
    for a, b in zip(cuts, cuts[1:]):
        g, s = _run_batch(ka, ctx, L, opts, dw[a * rw:b * rw], dl[a * L.n_files:b * L.n_files], b - a, max_len)
        merged += g
        n_valid += s["n_valid"]
    assert sorted(merged) == want and n_valid == meta["n_processed"]


def _write_fastq(path, reads, gz):
    data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(data)


def _parse_out(d):
    b = open(os.path.join(d, "output.bus"), "rb").read()
    assert b[:4] == b"BUS\0"
    ver, bclen, umilen, tlen = np.frombuffer(b[4:20], "<u4").tolist()
    rec = np.frombuffer(b[20 + tlen:], BUS_DTYPE)
    ecs = {}
    for i, line in enumerate(open(os.path.join(d, "matrix.ec"))):
        e, trs = line.split()
        assert int(e) == i
        ecs[i] = tuple(int(x) for x in trs.split(","))
    return (ver, bclen, umilen), rec, ecs, json.load(open(os.path.join(d, "run_info.json")))


@pytest.mark.parametrize("name", B.DRIVER_CASES)
def test_driver_writes_the_references_output(ka, name, tmp_path):
    """python -m kallisto_amd.bus_sc, once as a process on plain FASTQ with the default (sorted, collapsed) records, once in this process on gzip
    files with --bus-per-read and units of 1000 read sets (so that batch-local classes are merged)"""
    from kallisto_amd import bus_sc
    c = B.CASES[name]
    meta, want = B.load_golden(name)
    L, _, items, _ = B.case_reads(name)
    _, idx, _, _ = common.load_case(c["fixture"])
    files = {}
    for gz in (False, True):
        files[gz] = [str(tmp_path / ("reads_%d.fq%s" % (f, ".gz" if gz else ""))) for f in range(L.n_files)]
        for f, p in enumerate(files[gz]):
            _write_fastq(p, [it[f] for it in items], gz)
    out1, out2 = str(tmp_path / "out_plain"), str(tmp_path / "out_gz")
    p = subprocess.run([sys.executable, "-m", "kallisto_amd.bus_sc", "-x", c["tech"].lower(), "-i", idx, "-o", out1, *c["flags"], *files[False]], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    assert bus_sc.main(["-x", c["tech"], "-i", idx, "-o", out2, "--bus-per-read", "--unit-records", "1000", *c["flags"], *files[True]]) == 0
    for out, per_read in ((out1, False), (out2, True)):
        hdr, rec, ecs, info = _parse_out(out)
        assert list(hdr) == meta["bus_header"]
        lines = sorted((int(r["flags"]), int(r["bc"]), int(r["umi"]), ecs[int(r["ec"])]) for r in rec for _ in range(int(r["count"])))
        assert lines == want
        assert set(ecs.values()) == {l[3] for l in want} and len(set(ecs.values())) == len(ecs)
        assert info["n_processed"] == meta["n_processed"] and info["n_pseudoaligned"] == meta["n_pseudoaligned"] and info["n_unique"] == meta["n_unique"]
        assert info["n_reads"] == meta["n_reads"]
        key = [(int(r["bc"]), int(r["umi"]), int(r["ec"]), int(r["flags"])) for r in rec]
        assert key == sorted(key)
        if per_read:
            assert np.all(rec["count"] == 1)
        else:
            assert len(set(key)) == len(key) and int(rec["count"].max()) > 1
