"""Kernel A (k_match_v3, its second pass, k_classify and the absorption behind it) in the launch forms that kamd_tuning and the index
select: include/kallisto_amd.h promises of the tuning fields that "none of them changes a result".  Everything goes through Context.tune
and Index(path, table_layout=...); the expected values are the reference's goldens, the oracle on the same reads where a test feeds a
prefix or a tiling of a fixture, and for the order of the finalized classes the one-chunk run that every other test pins."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

# the tuning a fresh context has (tuning_defaults): every test puts it back in a `finally`, the contexts are shared
DEFAULTS = dict(text_verify=True, items_per_wave=1024, refill_min=8, lds_pad=-1, align_chunks=-1)
CHUNK_ITEMS = 65536               # align_batch: a chunk holds at least this many items
N_TILED = 4 * CHUNK_ITEMS + 1234  # four chunks, the last one shorter than the others


def chunks_that_run(align_chunks, n_items):
    """align_batch's rule, restated: min(align_chunks, 64, n_items // 65536), one chunk when the field is at its default (-1)"""
    return max(1, min(align_chunks if align_chunks > 0 else 1, 64, n_items // CHUNK_ITEMS))


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    kallisto_amd.load_library()
    return kallisto_amd


@pytest.fixture(scope="module")
def ctxs(ka):
    """one index and one context per (case, table layout); a use starts from an empty EC state"""
    cache = {}

    def get(case, layout=None):
        key = (case, layout)
        if key not in cache:
            index = ka.Index(common.load_case(case)[1], table_layout=layout)
            ctx = ka.Context(0)
            ctx.upload(index)
            if layout is not None:
                assert ctx.table_info()["table_layout"] == ka.Index.TABLE_LAYOUTS[layout]
            cache[key] = (index, ctx)
        else:
            cache[key][1].reset()
        return cache[key]
    yield get
    for _, c in cache.values():
        c.close()


@pytest.fixture(scope="module")
def oracle_prefix():
    """the oracle's classes of the first n items of a fixture under a variant's options, computed once per (case, variant, n)"""
    from oracle import oracle as O
    cache, indices = {}, {}

    def get(case, variant, n):
        key = (case, variant, n)
        if key not in cache:
            meta, idx_path, r1, r2 = common.load_case(case)
            o = common.parse_variant(meta["variants"][variant])
            if case not in indices:
                indices[case] = O.Index(idx_path)
            buf, off, lens = O.pack_reads(common.interleave(r1[:n], r2[:n] if o["paired"] else None))
            res = O.process_reads(indices[case], O.Opts(o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"]), buf, off, lens)
            cache[key] = _nonzero(res.multiset())
        return cache[key]
    return get


def _nonzero(ms):
    return {k: v for k, v in ms.items() if v}


def _opts(ka, o):
    return ka.QuantOpts(o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"])


def _packed(ctx, case, variant):
    meta, idx_path, r1, r2 = common.load_case(case)
    o = common.parse_variant(meta["variants"][variant])
    words, lens, max_len = ctx.pack_reads_host(common.interleave(r1, r2 if o["paired"] else None))
    return o, words, lens, len(r1), max_len


def _quant_and_check(ka, ctx, case, variant, **tune):
    """one quant of the whole fixture under `tune`: n_processed, the EC multiset, flens and eff_lens exact, est_counts at the suite's
    tolerance; returns (stats, profile)"""
    exp = common.load_expected(case, variant)
    o, words, lens, n, max_len = _packed(ctx, case, variant)
    try:
        got = ctx.tune(**tune)
        for f, v in tune.items():
            assert got[f] == ({True: 1, False: 2}[v] if isinstance(v, bool) else v), (f, got[f])
        ctx.reset()
        res = ka.quant(ctx, _opts(ka, o), [(words, lens, n, max_len)])
        prof = ctx.profile()
    finally:
        ctx.tune(**DEFAULTS)
    assert res.n_processed == exp["nproc"]
    assert res.ecs.multiset() == exp["ecs"]
    assert np.array_equal(res.flens, exp["flens"])
    assert np.array_equal(res.eff_lens, exp["eff"])
    common.assert_abundance_close(res.est_counts, exp["alpha"], "est_counts")
    return res.stats, prof


# ---- 1. text_verify off, both layouts ------------------------------------------------------------------------------------------------

TEXT_CASES = [("human_pe", "pe"), ("dlist_pe", "pe"), ("mosaic_pe", "pe_nojump"), ("mosaic_pe", "pe"), ("stress_pe", "pe"), ("yeast_se", "se_rf"),
              ("k17_pe", "pe"), ("k29_pe", "pe_union")]


@pytest.mark.parametrize("text", ["text_on", "text_off"])
@pytest.mark.parametrize("layout", ["wide", "compact"])
@pytest.mark.parametrize("case,variant", TEXT_CASES)
def test_text_verify_off_gives_the_same_result(case, variant, layout, text, ka, ctxs):
    """text_verify off selects the TXT = false instantiations of k_match_v3, in the first and in the second pass (stress_pe), with and
    without a D-list (dlist_pe), for paired and single-end items, on both layouts of the k-mer table.  n_text_hits shows that the switch
    took effect: a window is answered from the unitig text only where match() jumps, so the counter is positive exactly when the switch is
    on and the run jumps -- under --no-jump (mosaic_pe/pe_nojump) no window is ever a jump target and the counter is 0 either way;
    mosaic_pe/pe is here so that this index sees the switch, too."""
    index, ctx = ctxs(case, layout)
    meta = common.load_case(case)[0]
    no_jump = common.parse_variant(meta["variants"][variant])["no_jump"]
    stats, prof = _quant_and_check(ka, ctx, case, variant, text_verify=(text == "text_on"))
    assert (stats["n_text_hits"] > 0) == (text == "text_on" and not no_jump), stats
    if text == "text_off":
        assert stats["n_text_hits"] == 0
    assert stats["n_probes"] > 0
    if case == "stress_pe":
        assert prof["n_overflow_second_pass"] > 0, prof


# ---- 2. the shape of a wavefront's share of the items -------------------------------------------------------------------------------

@pytest.mark.parametrize("refill_min", [1, 8, 64])
@pytest.mark.parametrize("items_per_wave", [64, 100, 1000])
@pytest.mark.parametrize("case", ["human_pe", "stress_pe"])
def test_items_per_wave_and_refill_min(case, items_per_wave, refill_min, ka, ctxs):
    """items_per_wave (any value >= 64, a multiple of 64 or not) and refill_min (1 .. 64) shape the refill of the persistent wavefronts:
    a share of exactly one wavefront's lanes, shares that end inside a wavefront's lanes, a refill at every free lane and only when all
    64 are free."""
    index, ctx = ctxs(case)
    stats, prof = _quant_and_check(ka, ctx, case, "pe", items_per_wave=items_per_wave, refill_min=refill_min)
    if case == "stress_pe":
        assert prof["n_overflow_second_pass"] > 0, prof


def test_items_per_wave_on_the_wide_table(ka, ctxs):
    index, ctx = ctxs("human_pe", "wide")
    _quant_and_check(ka, ctx, "human_pe", "pe", items_per_wave=100, refill_min=1)


def _prefix_sizes(ipw):
    return sorted({1, 63, 64, 65, ipw - 1, ipw, ipw + 1, 2 * ipw + 1})


@pytest.mark.parametrize("ipw,n", [(ipw, n) for ipw in (64, 100) for n in _prefix_sizes(ipw)])
def test_batch_sizes_around_a_wavefronts_share(ipw, n, ka, ctxs, oracle_prefix):
    """the first n pairs of human_pe with n around a wavefront's lanes and around items_per_wave: the last wavefront's share is one item,
    one short of full, full, and the grid gains a wavefront for a single item"""
    meta, idx_path, r1, r2 = common.load_case("human_pe")
    index, ctx = ctxs("human_pe")
    words, lens, max_len = ctx.pack_reads_host(common.interleave(r1[:n], r2[:n]), 100)
    try:
        assert ctx.tune(items_per_wave=ipw)["items_per_wave"] == ipw
        ctx.reset()
        ctx.pseudoalign(ka.QuantOpts(1, 0.0, 0.0, 0, 0), words, lens, n, max_len)
        ecs = ctx.finalize()
        n_proc = ctx.stats()["n_processed"]
    finally:
        ctx.tune(**DEFAULTS)
    assert n_proc == n
    assert _nonzero(ecs.multiset()) == oracle_prefix("human_pe", "pe", n)


# ---- 3. lds_pad ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [16384, 60000])
def test_lds_pad_changes_nothing(pad, ka, ctxs):
    """unused LDS per block (fewer resident wavefronts; the host clamps the block's total at 64 KB): the result of the reference, and the
    finalized classes of the unpadded run of the same context"""
    index, ctx = ctxs("human_pe")
    o, words, lens, n, max_len = _packed(ctx, "human_pe", "pe")
    ctx.reset()
    plain = ka.quant(ctx, _opts(ka, o), [(words, lens, n, max_len)])
    try:
        assert ctx.tune(lds_pad=pad)["lds_pad"] == pad
        ctx.reset()
        padded = ka.quant(ctx, _opts(ka, o), [(words, lens, n, max_len)])
    finally:
        ctx.tune(**DEFAULTS)
    assert ctx.tune()["lds_pad"] == -1
    assert padded.n_processed == plain.n_processed == n
    assert padded.ecs.multiset() == plain.ecs.multiset() == common.load_expected("human_pe", "pe")["ecs"]
    assert np.array_equal(padded.flens, plain.flens) and np.array_equal(padded.eff_lens, plain.eff_lens)
    assert np.array_equal(padded.est_counts.view(np.uint64), plain.est_counts.view(np.uint64))   # (the EM plan orders rows by content: identical bits)


# ---- 4. several chunks per batch -----------------------------------------------------------------------------------------------------

class _Tiled:
    """A fixture's packed reads tiled ON THE DEVICE to N_TILED items (records have a fixed size, so Tensor.repeat is a valid input), the
    multiset expected of `calls` batches of it -- the golden one times the whole tiles plus the oracle's of the partial tile -- and the
    one-chunk run (align_chunks = 1) of the same input."""

    def __init__(self, ka, ctx, case, variant, calls, oracle_prefix):
        import torch
        self.ka, self.ctx, self.calls = ka, ctx, calls
        self.o, words, lens, n, self.max_len = _packed(ctx, case, variant)
        nm = 2 if self.o["paired"] else 1
        rec = ka.packed_record_words(self.max_len)
        assert words.numel() == n * nm * rec and lens.numel() == n * nm
        tiles, rem = divmod(N_TILED, n)
        self.words = torch.cat([words.repeat(tiles), words[:rem * nm * rec]])
        self.lens = torch.cat([lens.repeat(tiles), lens[:rem * nm]])
        exp = {k: v * tiles * calls for k, v in common.load_expected(case, variant)["ecs"].items()}
        for k, v in oracle_prefix(case, variant, rem).items():
            exp[k] = exp.get(k, 0) + v * calls
        self.expected = _nonzero(exp)
        assert chunks_that_run(1, N_TILED) == 1
        self.one_chunk = self.run(1)

    def run(self, align_chunks):
        """the quant flow over `calls` batches of the tiled input from an empty state, first-occurrence order tracked: the fragment-length
        sample is the one that kamd_fld_prefetch starts underneath kernel A's chunks -> (ECs in first-occurrence order, flens, n_processed, profile)"""
        ka, ctx = self.ka, self.ctx
        try:
            assert ctx.tune(align_chunks=align_chunks)["align_chunks"] == align_chunks
            ctx.reset()
            ctx.track_order(True)
            res = ka.quant(ctx, _opts(ka, self.o), [(self.words, self.lens, N_TILED, self.max_len)] * self.calls)
            prof = ctx.profile()
        finally:
            ctx.tune(**DEFAULTS)
            ctx.reset()
            ctx.track_order(False)
        return res.ecs, res.flens, res.n_processed, prof


@pytest.fixture(scope="module")
def tiled(ka, ctxs, oracle_prefix):
    cache = {}

    def get(case, variant, layout=None, calls=1):
        key = (case, variant, layout, calls)
        if key not in cache:
            cache[key] = _Tiled(ka, ctxs(case, layout)[1], case, variant, calls, oracle_prefix)
        return cache[key]
    return get


def _assert_same_as_one_chunk(got, one, expected, calls=1):
    ecs, flens, n_proc, prof = got
    ecs1, flens1, n_proc1, prof1 = one
    assert n_proc == n_proc1 == calls * N_TILED
    assert _nonzero(ecs1.multiset()) == expected          # the one-chunk path, which every other test pins, on this input
    assert _nonzero(ecs.multiset()) == expected
    assert np.array_equal(flens, flens1)
    assert np.array_equal(ecs.counts, ecs1.counts) and np.array_equal(ecs.ec_off, ecs1.ec_off) and np.array_equal(ecs.ec_ids, ecs1.ec_ids)


@pytest.mark.parametrize("align_chunks", [2, 4])
@pytest.mark.parametrize("case,variant", [("human_pe", "pe"), ("human_pe", "pe_rf"), ("mosaic_pe", "pe_union"), ("yeast_se", "se"), ("stress_pe", "pe")])
def test_several_chunks_per_batch(case, variant, align_chunks, ka, tiled):
    """A batch of four chunks' worth of items in 2 and 4 chunks: kernel A's chunks on the caller's stream, k_classify and the absorption of
    chunk k on the side stream beside the matching of chunk k + 1 (WorkStream::fork, the per-chunk events), every chunk at its own offsets
    into the slots, the record offsets, the first-occurrence keys and the item numbers (k_classify's four `first` arguments, absorb_tuples'
    and k_tup_absorb4's item0), overflow and explicit-filter item lists that grow from chunk to chunk (stress_pe; pe_rf, pe_union), and
    the second pass behind the absorption instead of beside it (stress_pe)."""
    t = tiled(case, variant)
    n_chunks = chunks_that_run(align_chunks, N_TILED)
    assert n_chunks == align_chunks >= 2
    got = t.run(align_chunks)
    print(f"chunks that ran: {case}/{variant} align_chunks={align_chunks} n_items={N_TILED} -> {n_chunks}")
    _assert_same_as_one_chunk(got, t.one_chunk, t.expected)
    if case == "stress_pe":
        assert got[3]["n_overflow_items"] > 0 and got[3]["n_overflow_second_pass"] > 0, got[3]


def test_several_chunks_on_the_wide_table(ka, tiled):
    t = tiled("human_pe", "pe", "wide")
    assert chunks_that_run(4, N_TILED) == 4
    _assert_same_as_one_chunk(t.run(4), t.one_chunk, t.expected)


def test_several_chunks_into_a_populated_tuple_table(ka, tiled):
    """the same tiled batch twice without a reset, in four chunks each: from the second chunk on every tuple record finds its owner in
    the store (k_tup_absorb4's straight-line case across chunks), and the second call's keys continue behind the first's"""
    t = tiled("human_pe", "pe", None, 2)
    assert chunks_that_run(4, N_TILED) == 4
    _assert_same_as_one_chunk(t.run(4), t.one_chunk, t.expected, calls=2)
