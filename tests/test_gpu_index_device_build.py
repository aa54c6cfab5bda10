"""The k-mer table built on the GPU (kamd_index_load_deferred + kamd_index_upload, kallisto_amd/csrc/kamd_ixbuild.hip): byte for byte the
table the host builder produces with one thread, deterministic from build to build, and the quant results through it are the reference's.

The shapes are the fixtures': tiny_k7_se (k = 7, 624 unitigs for 1 325 k-mers, one scan block), ref_test_pe (21 long unitigs), yeast_se /
stress_pe (412-415 k k-mers, 115-277 k home buckets: a multi-block scan, pad buckets at a load of 0.9), dlist_pe (D-list table, dummy hit)."""
import os
import subprocess

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
LAYOUTS = [("wide", "wide", 0.0), ("compact", "compact", 0.0), ("compact09", "compact", 0.9)]


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    kallisto_amd.load_library()
    return kallisto_amd


@pytest.fixture(scope="module")
def ctx(ka):
    c = ka.Context(0)
    yield c
    c.close()


def _host_tables(ka, index):
    v = index.view
    lines = v.n_buckets + v.pad_buckets
    np_ = ka.api._np
    return {"table": np_(v.table, lines * 8, np.uint64), "slot_block": np_(v.slot_block, lines * v.slots_per_bucket, np.uint32),
            "slot_dist": np_(v.slot_dist, lines * v.slots_per_bucket, np.uint32), "dtable": np_(v.dtable, (v.n_dbuckets + v.dpad_buckets) * 8, np.uint64)}


@pytest.mark.parametrize("lname,layout,load", LAYOUTS, ids=[x[0] for x in LAYOUTS])
@pytest.mark.parametrize("case", common.CASES)
def test_device_built_table_is_the_one_thread_host_table(case, lname, layout, load, ka, ctx):
    meta, idx_path, r1, r2 = common.load_case(case)
    host = ka.Index(idx_path, 1, layout, load)
    want = _host_tables(ka, host)
    hv = host.view
    deferred = ka.Index(idx_path, 2, layout, load, deferred=True)
    assert not deferred.view.table and not deferred.view.slot_block and not deferred.view.slot_dist and not deferred.view.dtable and deferred.view.n_buckets == 0
    ctx.upload(deferred)
    info = ctx.table_info()
    got = ctx.table_download()
    assert info["built_on_device"] == 1 and info["build_rounds"] == 1 and info["build_ms"] > 0
    for n, h in (("n_buckets", hv.n_buckets), ("pad_buckets", hv.pad_buckets), ("table_layout", hv.table_layout), ("slots_per_bucket", hv.slots_per_bucket),
                 ("tag_q", hv.tag_q), ("tag_dsh", hv.tag_dsh), ("tag_w", hv.tag_w), ("n_dbuckets", hv.n_dbuckets), ("dpad_buckets", hv.dpad_buckets),
                 ("dummy_slot", hv.dummy_slot), ("dummy_uec", hv.dummy_uec), ("dummy_strand", hv.dummy_strand)):
        assert info[n] == h, n
    assert (case == "dlist_pe") == (want["dtable"].size > 0)
    for n in ("table", "slot_block", "slot_dist", "dtable"):
        assert got[n].tobytes() == want[n].tobytes(), n
    # a second build on the same context (the first one's tables are freed): the same bytes
    ctx.upload(deferred)
    again = ctx.table_download()
    for n in ("table", "slot_block", "slot_dist", "dtable"):
        assert again[n].tobytes() == got[n].tobytes(), n
    # the case's default variant through the device-built index: the assertions of test_gpu_parity.py
    variant = next(iter(meta["variants"]))
    o = common.parse_variant(meta["variants"][variant])
    exp = common.load_expected(case, variant)
    reads = common.interleave(r1, r2 if o["paired"] else None)
    words, lens, max_len = ctx.pack_reads_host(reads)
    opts = ka.QuantOpts(o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"])
    res = ka.quant(ctx, opts, [(words, lens, len(r1), max_len)])
    assert res.n_processed == exp["nproc"]
    assert res.ecs.multiset() == exp["ecs"]
    assert np.array_equal(res.flens, exp["flens"])
    assert np.array_equal(res.eff_lens, exp["eff"])
    common.assert_abundance_close(res.est_counts, exp["alpha"], "est_counts")
    tiny = lambda x: np.where(np.abs(x) < 1e-200, 0.0, x)
    common.assert_abundance_close(tiny(res.alpha_before_zeroes), tiny(exp["abz"]), "alpha_before_zeroes", floor=1e-9)


def test_table_info_and_download_after_a_host_upload(ka, ctx):
    """both entry points work after either kind of upload"""
    host = ka.Index(common.load_case("dlist_pe")[1], 1, "compact", 0.0)
    ctx.upload(host)
    info = ctx.table_info()
    assert info["built_on_device"] == 0 and info["build_ms"] == 0 and info["n_buckets"] == host.view.n_buckets and info["n_dbuckets"] == host.view.n_dbuckets
    got, want = ctx.table_download(), _host_tables(ka, host)
    for n in ("table", "slot_block", "slot_dist", "dtable"):
        assert got[n].tobytes() == want[n].tobytes(), n


def _fastq(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def test_cli_index_build_device(tmp_path):
    """`quant --index-build device` writes the abundance.tsv of `--index-build host`, byte for byte"""
    assert os.path.exists(EXE), "build kallisto_amd_quant with `make -C kallisto_amd/csrc all`"
    meta, idx_path, r1, r2 = common.load_case("ref_test_pe")
    f1, f2 = str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq")
    _fastq(f1, r1)
    _fastq(f2, r2)
    outs = {}
    for where in ("host", "device"):
        out = str(tmp_path / where)
        p = subprocess.run([EXE, "quant", "-i", idx_path, "-o", out, "--plaintext", "--verbose", "--index-build", where, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, KAMD_NO_FLAT_INDEX="1"))
        assert p.returncode == 0, p.stderr.decode()
        assert ("k-mer table built on the device" in p.stderr.decode()) == (where == "device")
        outs[where] = open(os.path.join(out, "abundance.tsv"), "rb").read()
    assert outs["host"] == outs["device"] and len(outs["host"]) > 100
    p = subprocess.run([EXE, "quant", "-i", idx_path, "-o", str(tmp_path / "bad"), "--index-build", "elsewhere", f1, f2], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and b"--index-build expects host or device" in p.stderr
