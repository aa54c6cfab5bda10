"""The fragment-length sample (kamd_fld_prefetch / kamd_fld_from_batch: k_fld_first, k_fld, k_fld_count, k_fld_scan, k_fld_emit, the host loop over
prefixes, the class-list overflow path, the sample carried over batches, ranks and the front-end's batches) at and beyond its cut of 10 000 pairs.

Every expectation is "the first 10 000 qualifying pairs in input order" restated in numpy over the ORACLE's per-pair flags of one tile of a
fixture (tests/fld_sample_common.py; test_fld_sample_cpu.py holds that against the oracle's own walk) -- never a run of the code under test.
All comparisons are exact: np.array_equal on flens plus the returned `used`.  kamd_profile's last_fld_* counters show that the path a test is
about actually ran.  Tests that tune put the defaults back in a `finally`; the contexts are shared."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import common
from tests import fld_sample_common as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
H5DUMP = "/opt/conda/bin/h5dump"
DEFAULTS = dict(fld_list_cap=64, fld_first_chunk=F.FIRST_CHUNK, align_chunks=-1)


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    kallisto_amd.load_library()
    return kallisto_amd


@pytest.fixture(scope="module")
def ctxs(ka):
    """one index and one context per fixture; a use starts from an empty EC state and the default tuning"""
    cache = {}

    def get(case):
        if case not in cache:
            index = ka.Index(F.case_reads(case)[0])
            ctx = ka.Context(0)
            ctx.upload(index)
            cache[case] = (index, ctx)
        ctx = cache[case][1]
        ctx.reset()
        got = ctx.tune()
        assert {k: got[k] for k in DEFAULTS} == DEFAULTS
        return ctx
    yield get
    for _, c in cache.values():
        F.forget_packed(c)
        c.close()


def _opts(ka, strand=0, single_overhang=0, no_jump=0, union=0):
    return ka.QuantOpts(1, 0.0, 0.0, single_overhang, strand, no_jump, union)


def _expected(inp, start_used=0, **o):
    q, tls = F.pair_flags(inp.case, **o)
    return F.expected_flens(q, tls, inp.order(), start_used)


def _sample(ka, ctx, dev, flens=None, used=0, **o):
    """kamd_fld_from_batch on a device input -> (flens, used, profile)"""
    words, lens, n, max_len = dev
    flens, used = ctx.fld_from_batch(_opts(ka, **o), words, lens, n, max_len, flens, used)
    return flens, used, ctx.profile()


def _assert_sample(got, want, chunks=None, prefetched=0):
    flens, used, prof = got
    wflens, wused = want
    print(f"used {used} (expected {wused}), sum {int(flens.sum())}, chunks {prof['last_fld_chunks']}, candidates {prof['last_fld_candidates']}, "
          f"list overflows {prof['last_fld_list_overflows']}, prefetched {prof['last_fld_prefetched']}")
    assert used == wused
    assert np.array_equal(flens, wflens), np.flatnonzero(flens != wflens)[:10]
    if chunks is not None:
        assert prof["last_fld_chunks"] == chunks
    assert prof["last_fld_prefetched"] == prefetched


# ---- 1. the cut, one batch -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tiles,o", [(2, {}), (4, {"strand": 1}), (4, {"strand": 2}), (4, {"single_overhang": 1})],
                         ids=["pe x 2", "fr x 4", "rf x 4", "single-overhang x 4"])
def test_cut_in_one_batch(tiles, o, ka, ctxs):
    ctx = ctxs("ref_test_pe")
    inp = F.tiled("ref_test_pe", tiles)
    want = _expected(inp, **o)
    assert want[1] == F.WANT
    got = _sample(ka, ctx, inp.device(ka, ctx), **o)
    _assert_sample(got, want, chunks=1)
    assert got[2]["last_fld_list_overflows"] == 0 and 0 < got[2]["last_fld_candidates"] <= inp.n_items


@pytest.mark.parametrize("nq", [9999, 10000, 10001])
def test_batch_with_exactly_that_many_qualifying_pairs(nq, ka, ctxs):
    ctx = ctxs("ref_test_pe")
    inp = F.prefix_with(nq)
    want = _expected(inp)
    assert want[1] == min(nq, F.WANT)
    _assert_sample(_sample(ka, ctx, inp.device(ka, ctx)), want, chunks=1)


@pytest.mark.parametrize("item", [16383, 16384, 16895, 16896, 16900])
def test_cut_against_the_ranking_kernels_tiling(item, ka, ctxs):
    """k_fld_count / k_fld_emit rank 8 items per thread, 512 per wavefront, 8192 per block: the 10 000th qualifying pair as the last item of
    the second block, the first of the third, the last / first item of a wavefront and the fifth item of a thread"""
    assert (item + 1) % F.RANK_PER_BLOCK == 0 or item % F.RANK_PER_BLOCK == 0 or (item + 1) % F.RANK_PER_WAVE == 0 or item % F.RANK_PER_WAVE == 0 \
        or item % F.RANK_PER_THREAD == 4
    ctx = ctxs("ref_test_pe")
    inp = F.cut_at(item)
    want = _expected(inp)
    assert want[1] == F.WANT
    _assert_sample(_sample(ka, ctx, inp.device(ka, ctx)), want, chunks=1)


@pytest.mark.parametrize("n_items", [16383, 16384, 16385])
def test_batch_that_ends_with_the_last_pair_of_the_sample(n_items, ka, ctxs):
    """n_items one short of two blocks, two blocks, two blocks and one item; the batch's last item is the 10 000th qualifying pair"""
    ctx = ctxs("ref_test_pe")
    inp = F.cut_at(n_items - 1).prefix(n_items)
    q, _ = F.pair_flags("ref_test_pe")
    pos = F.qualifying_positions(q, inp.order())
    assert inp.n_items == n_items and len(pos) == F.WANT and pos[-1] == n_items - 1
    _assert_sample(_sample(ka, ctx, inp.device(ka, ctx)), _expected(inp), chunks=1)


# ---- 2. the sample carried across calls ----------------------------------------------------------------------------------------------

def _carry_cuts():
    q, _ = F.pair_flags("ref_test_pe")
    pos = F.qualifying_positions(q, F.tiled("ref_test_pe", 2).order())
    first, last_but_one, last = int(pos[0]), int(pos[F.WANT - 2]), int(pos[F.WANT - 1])
    return {
        # used == 1 before the last contributing batch
        "1 then the rest": ([first + 1, first + 1, 20000], [1, 1, F.WANT]),
        # used == 9 999 before it
        "9999 then one": ([3000, 3000, 3001, last_but_one + 1, last_but_one + 1, 20000], [None, None, None, F.WANT - 1, F.WANT - 1, F.WANT]),
        # already 10 000 before further batches
        "full then more": ([7, last + 1, last + 1, last + 2, 20000], [None, F.WANT, F.WANT, F.WANT, F.WANT]),
    }


@pytest.mark.parametrize("name", ["1 then the rest", "9999 then one", "full then more"])
def test_sample_carried_across_calls(name, ka, ctxs):
    """the same reads in ragged batches (batches of 0 items among them), flens / used handed on: the result is the one-batch result and the
    expectation; a call that finds the sample full leaves it untouched"""
    ends, used_after = _carry_cuts()[name]
    ctx = ctxs("ref_test_pe")
    whole = F.tiled("ref_test_pe", 2)
    want = _expected(whole)
    flens, used, lo = np.zeros(common.MAX_FRAG_LEN, np.uint32), 0, 0
    for hi, want_used in zip(ends, used_after):
        part = whole.window(lo, hi)
        words, lens, n, max_len = part.device(ka, ctx)
        before, used_before = flens.copy(), used
        f, wu = _expected(part, used)                                    # what this batch adds, from the oracle's flags
        flens, used, prof = _sample(ka, ctx, (words.clone(), lens.clone(), n, max_len), flens, used)
        print(f"batch [{lo}, {hi}): used {used_before} -> {used}")
        assert used == wu and (want_used is None or used == want_used)
        assert np.array_equal(flens, before + f)
        if used_before == F.WANT or n == 0:
            assert np.array_equal(flens, before) and prof["last_fld_chunks"] == 0
        lo = hi
    assert lo == whole.n_items and used == want[1] == F.WANT
    assert np.array_equal(flens, want[0])
    _assert_sample(_sample(ka, ctx, whole.device(ka, ctx)), want, chunks=1)     # the one-batch result


# ---- 3. second and later prefixes ----------------------------------------------------------------------------------------------------

def test_later_prefixes_with_a_small_first_prefix(ka, ctxs):
    ctx = ctxs("ref_test_pe")
    try:
        assert ctx.tune(fld_first_chunk=8192)["fld_first_chunk"] == 8192
        # dense, nothing, dense: the second prefix finds nothing, the third is sized from the diluted rate
        dsd = F.dense_sparse_dense()
        dev = dsd.device(ka, ctx)
        _assert_sample(_sample(ka, ctx, dev), _expected(dsd), chunks=3)
        # the cut inside the second prefix
        two = F.tiled("ref_test_pe", 2)
        _assert_sample(_sample(ka, ctx, two.device(ka, ctx)), _expected(two), chunks=2)
        # a sample that arrives half full: fewer pairs wanted from the same prefixes
        f0, u0 = _expected(F.tiled("ref_test_pe", 1))
        f1, u1 = _expected(dsd, u0)
        assert u0 == 6429 and u1 == F.WANT
        got = _sample(ka, ctx, dev, f0.copy(), u0)
        assert got[1] == u1 and np.array_equal(got[0], f0 + f1) and got[2]["last_fld_chunks"] >= 1
    finally:
        ctx.tune(**DEFAULTS)
    _assert_sample(_sample(ka, ctx, dev), _expected(dsd), chunks=1)                # the same input without the hook


def test_tuning_hooks_keep_their_ranges(ka, ctxs):
    ctx = ctxs("ref_test_pe")
    try:
        for bad in (dict(fld_first_chunk=63), dict(fld_first_chunk=F.FIRST_CHUNK + 1), dict(fld_list_cap=65), dict(fld_list_cap=-1)):
            got = ctx.tune(**bad)
            assert {k: got[k] for k in DEFAULTS} == DEFAULTS, bad        # values outside a field's range are ignored, 0 keeps
        got = ctx.tune(fld_first_chunk=64, fld_list_cap=1)
        assert got["fld_first_chunk"] == 64 and got["fld_list_cap"] == 1
    finally:
        ctx.tune(**DEFAULTS)


def test_later_prefixes_at_the_default_size(ka, ctxs):
    """human_pe x 300 (1.5 M pairs, tiled on the device): 7.5 k qualifying pairs in the first 1 048 576 items, so the loop goes on"""
    ctx = ctxs("human_pe")
    inp = F.tiled("human_pe", 300)
    want = _expected(inp)
    assert want[1] == F.WANT
    got = _sample(ka, ctx, inp.device(ka, ctx))
    _assert_sample(got, want)
    assert got[2]["last_fld_chunks"] >= 2


# ---- 4. through ka.quant -------------------------------------------------------------------------------------------------------------

def _oracle_eff(case, flens):
    from oracle import oracle as O
    eff, _ = O.eff_lens(F.oracle_index(case).target_lens, O.mean_frag_lens_trunc(flens))
    return eff


def _batches(dev, per, ka):
    words, lens, n, max_len = dev
    rec = 2 * ka.packed_record_words(max_len)
    return [(words[lo * rec:min(lo + per, n) * rec], lens[2 * lo:2 * min(lo + per, n)], min(lo + per, n) - lo, max_len) for lo in range(0, n, per)]


def test_quant_one_batch_and_batches_of_3000(ka, ctxs):
    ctx = ctxs("ref_test_pe")
    inp = F.tiled("ref_test_pe", 2)
    want = _expected(inp)
    eff = _oracle_eff("ref_test_pe", want[0])
    dev = inp.device(ka, ctx)
    res = ka.quant(ctx, _opts(ka), [dev])
    prof = ctx.profile()
    assert res.n_processed == inp.n_items
    assert np.array_equal(res.flens, want[0]) and res.flens.sum() == F.WANT
    assert np.array_equal(res.eff_lens, eff)
    assert prof["last_fld_prefetched"] == 1 and prof["last_fld_chunks"] == 1      # the launch behind kernel A was the one consumed
    ctx.reset()
    parts = _batches(dev, 3000, ka)
    assert len(parts) == 7 and parts[-1][2] == 2000
    res = ka.quant(ctx, _opts(ka), parts)
    assert res.n_processed == inp.n_items
    assert np.array_equal(res.flens, want[0]) and np.array_equal(res.eff_lens, eff)
    assert ctx.profile()["last_fld_prefetched"] == 0                                # (the last call was on a later batch: only the first is prefetched)


def test_quant_deferred_launch_behind_chunked_kernel_a(ka, ctxs):
    """align_chunks = 2 on 14 tiles (140 000 items, two chunks of at least 65 536): the deferred launch sits behind kernel A's second chunk"""
    ctx = ctxs("ref_test_pe")
    inp = F.tiled("ref_test_pe", 14)
    assert inp.n_items >= 2 * 65536
    want = _expected(inp)
    dev = inp.device(ka, ctx)
    try:
        assert ctx.tune(align_chunks=2)["align_chunks"] == 2
        res = ka.quant(ctx, _opts(ka), [dev], download_ecs=False)
        prof = ctx.profile()
    finally:
        ctx.tune(**DEFAULTS)
    assert res.n_processed == inp.n_items
    assert np.array_equal(res.flens, want[0]) and np.array_equal(res.eff_lens, _oracle_eff("ref_test_pe", want[0]))
    assert prof["last_fld_prefetched"] == 1 and prof["last_fld_chunks"] == 1


# ---- 5. a prefetch that must not be used ---------------------------------------------------------------------------------------------

def test_prefetch_of_another_batch_is_not_used(ka, ctxs):
    """fld_prefetch on A, then fld_from_batch on B at other pointers"""
    ctx = ctxs("ref_test_pe")
    a = F.tiled("ref_test_pe", 1).window(5000, 10000)          # a batch whose sample differs from B's
    b = F.tiled("ref_test_pe", 1).window(0, 5000)
    da, db = a.device(ka, ctx), b.device(ka, ctx)
    assert not np.array_equal(_expected(a)[0], _expected(b)[0])
    ctx.fld_prefetch(_opts(ka), da[0], da[1], da[2], da[3])
    ctx.pseudoalign(_opts(ka), da[0], da[1], da[2], da[3])
    _assert_sample(_sample(ka, ctx, db), _expected(b), chunks=1, prefetched=0)
    # ... and A itself afterwards: the pending result was dropped as stale, not kept for later
    _assert_sample(_sample(ka, ctx, da), _expected(a), chunks=1, prefetched=0)


def test_prefetch_under_other_strand_option_is_not_used(ka, ctxs):
    """fld_prefetch + pseudoalign unstranded, then fld_from_batch with --rf on the same pointers"""
    ctx = ctxs("ref_test_pe")
    inp = F.tiled("ref_test_pe", 4)
    dev = inp.device(ka, ctx)
    assert not np.array_equal(_expected(inp)[0], _expected(inp, strand=2)[0])
    ctx.fld_prefetch(_opts(ka), dev[0], dev[1], dev[2], dev[3])
    ctx.pseudoalign(_opts(ka), dev[0], dev[1], dev[2], dev[3])
    _assert_sample(_sample(ka, ctx, dev, strand=2), _expected(inp, strand=2), chunks=1, prefetched=0)
    # the control: the same sequence with matching options does consume the prefetch, and gives the unstranded sample
    ctx.reset()
    ctx.fld_prefetch(_opts(ka), dev[0], dev[1], dev[2], dev[3])
    ctx.pseudoalign(_opts(ka), dev[0], dev[1], dev[2], dev[3])
    _assert_sample(_sample(ka, ctx, dev), _expected(inp), chunks=1, prefetched=1)


def test_prefetch_under_other_union_option_is_not_used(ka, ctxs):
    """fld_prefetch + pseudoalign with --union, then fld_from_batch without it on the same pointers: the launch behind kernel A read --union from
    the device index, its sample is not this call's (dlist_pe: the two samples differ)"""
    ctx = ctxs("dlist_pe")
    inp = F.tiled("dlist_pe", 1)
    dev = inp.device(ka, ctx)
    plain, union = common.load_expected("dlist_pe", "pe")["flens"], common.load_expected("dlist_pe", "pe_union")["flens"]
    assert not np.array_equal(plain, union)
    ou = _opts(ka, union=1)
    ctx.fld_prefetch(ou, dev[0], dev[1], dev[2], dev[3])
    ctx.pseudoalign(ou, dev[0], dev[1], dev[2], dev[3])
    got = _sample(ka, ctx, dev)
    _assert_sample(got, _expected(inp), chunks=1, prefetched=0)
    assert np.array_equal(got[0], plain)


def test_prefetch_nobody_picked_up_is_not_used(ka, ctxs):
    """fld_prefetch with no pseudoalign before fld_from_batch: nothing was launched, the sample is computed by the call"""
    ctx = ctxs("ref_test_pe")
    inp = F.tiled("ref_test_pe", 2)
    dev = inp.device(ka, ctx)
    ctx.fld_prefetch(_opts(ka), dev[0], dev[1], dev[2], dev[3])
    _assert_sample(_sample(ka, ctx, dev), _expected(inp), chunks=1, prefetched=0)


def test_prefetch_picked_up_by_another_batch_is_not_used(ka, ctxs):
    """fld_prefetch on A, pseudoalign on B, fld_from_batch on A"""
    ctx = ctxs("ref_test_pe")
    a, b = F.tiled("ref_test_pe", 2), F.cut_at(16900)
    da, db = a.device(ka, ctx), b.device(ka, ctx)
    ctx.fld_prefetch(_opts(ka), da[0], da[1], da[2], da[3])
    ctx.pseudoalign(_opts(ka), db[0], db[1], db[2], db[3])
    _assert_sample(_sample(ka, ctx, da), _expected(a), chunks=1, prefetched=0)
    _assert_sample(_sample(ka, ctx, db), _expected(b), chunks=1, prefetched=0)


def test_prefetch_with_a_small_first_prefix_is_consumed(ka, ctxs):
    """kamd_fld_prefetch and kamd_fld_from_batch size the first prefix alike: with the hook the prefetched prefix is still the one asked for"""
    ctx = ctxs("ref_test_pe")
    inp = F.tiled("ref_test_pe", 2)
    dev = inp.device(ka, ctx)
    try:
        ctx.tune(fld_first_chunk=8192)
        ctx.fld_prefetch(_opts(ka), dev[0], dev[1], dev[2], dev[3])
        ctx.pseudoalign(_opts(ka), dev[0], dev[1], dev[2], dev[3])
        _assert_sample(_sample(ka, ctx, dev), _expected(inp), chunks=2, prefetched=1)
    finally:
        ctx.tune(**DEFAULTS)


# ---- 6. the class-list overflow path -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,o", [("pe", {}), ("pe_union", {"union": 1})])
def test_class_list_overflow_path(variant, o, ka, ctxs):
    """fld_list_cap = 1: every candidate pair with two distinct classes overflows the first k_fld launch, is re-run with the large list, and the
    prefix's sample is taken on the host from the two downloaded vectors.  Expected: the reference's own sample of the fixture."""
    ctx = ctxs("dlist_pe")
    inp = F.tiled("dlist_pe", 1)
    dev = inp.device(ka, ctx)
    gold = common.load_expected("dlist_pe", variant)["flens"]
    want = _expected(inp, **o)
    assert np.array_equal(want[0], gold)
    try:
        assert ctx.tune(fld_list_cap=1)["fld_list_cap"] == 1
        got = _sample(ka, ctx, dev, **o)
    finally:
        ctx.tune(**DEFAULTS)
    _assert_sample(got, want, chunks=1)
    assert got[2]["last_fld_list_overflows"] > 0
    got = _sample(ka, ctx, dev, **o)                       # the default list: nothing overflows, the device-ranked sample
    _assert_sample(got, want, chunks=1)
    assert got[2]["last_fld_list_overflows"] == 0


def test_class_list_overflow_with_the_cut_inside_the_prefix(ka, ctxs):
    """dlist_pe x 1000 (4.5 M pairs, 11 000 qualifying) with a list of one entry: every prefix holds whole tiles, so every prefix overflows and
    takes the host loop; the 10 000th qualifying pair falls inside the last prefix, which holds more (test_fld_sample_cpu.py) -- the host
    loop's own cut.  (A bounded search over simulated reads of 100 / 150 / 250 bases against the human_pe, dlist_pe and k29_pe indexes found no
    QUALIFYING pair with two classes, so the pairs that overflow here do not themselves enter the sample.)"""
    ctx = ctxs("dlist_pe")
    inp = F.tiled("dlist_pe", 1000)
    want = _expected(inp)
    assert want[1] == F.WANT
    dev = inp.device(ka, ctx)
    try:
        ctx.tune(fld_list_cap=1, fld_first_chunk=65536)
        got = _sample(ka, ctx, dev)
    finally:
        ctx.tune(**DEFAULTS)
    _assert_sample(got, want)
    assert got[2]["last_fld_chunks"] >= 2 and got[2]["last_fld_list_overflows"] >= got[2]["last_fld_chunks"]


# ---- 7. two ranks ----------------------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kallisto_amd as ka
        index = ka.Index(F.case_reads("ref_test_pe")[0])
        ctx = ka.Context(0)
        ctx.upload(index)
        dev = F.tiled("ref_test_pe", 1).device(ka, ctx)       # rank r holds tile r + 1 of the input
        comm = ka.Comm.over_process_group(ctx)
        res = ka.quant(ctx, ka.QuantOpts(1, 0.0, 0.0, 0, 0), [dev], download_ecs=False, comm=comm)
        prof = ctx.profile()
        comm.close()
        q.put((rank, res.flens, res.eff_lens, res.n_processed, prof["last_fld_chunks"]))
    finally:
        dist.destroy_process_group()


def test_two_ranks_sample_cut_inside_the_second_shard():
    """gloo, two processes on one device: rank 0's tile holds 6 429 qualifying pairs, rank 1 continues the same sample over its own and is cut
    inside it; both ranks end with the sample of the whole input"""
    import torch.multiprocessing as mp
    want = _expected(F.tiled("ref_test_pe", 2))
    assert want[1] == F.WANT
    eff = _oracle_eff("ref_test_pe", want[0])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res = {g[0]: g for g in got}
    for r in (0, 1):
        _, flens, eff_r, n_proc, chunks = res[r]
        assert n_proc == 20000 and chunks == 1
        assert np.array_equal(flens, want[0]), r
        assert np.array_equal(eff_r, eff), r


# ---- 8. the front-end ------------------------------------------------------------------------------------------------------------------

def test_cli_sample_over_batches_of_3000(tmp_path):
    """`kallisto_amd_quant quant` on FASTQ of ref_test_pe x 2 in batches of 3000 pairs: aux/fld of abundance.h5 is the oracle's sample"""
    if not os.path.exists(H5DUMP):
        pytest.skip("h5dump not installed")
    assert os.path.exists(EXE), "build kallisto_amd_quant with `make -C kallisto_amd/csrc all`"
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import h5dump_tools as H
    idx_path, r1, r2 = F.case_reads("ref_test_pe")
    want = _expected(F.tiled("ref_test_pe", 2))
    files = []
    for name, reads in (("r_1.fq", r1), ("r_2.fq", r2)):
        files.append(str(tmp_path / name))
        with open(files[-1], "wb") as f:
            for i, r in enumerate(list(reads) * 2):
                f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    out = str(tmp_path / "out")
    p = subprocess.run([EXE, "quant", "-i", idx_path, "-o", out, "-t", "4", *files], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, KAMD_FQ_BATCH_ITEMS="3000"))
    assert p.returncode == 0, p.stderr.decode()
    dump = subprocess.run([H5DUMP, "-p", "-m", "%.12g", os.path.join(out, "abundance.h5")], check=True, stdout=subprocess.PIPE).stdout.decode()
    got = H.parse(dump)
    fld = np.array(got["aux/fld"]["values"], np.int64)
    assert len(fld) == common.MAX_FRAG_LEN and fld.sum() == F.WANT
    assert np.array_equal(fld, want[0].astype(np.int64))
    assert np.allclose(got["aux/eff_lengths"]["values"], _oracle_eff("ref_test_pe", want[0]), rtol=1e-11, atol=0)
