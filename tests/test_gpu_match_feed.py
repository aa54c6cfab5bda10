"""Kernel A's item feed on the device: persistent blocks whose wavefronts take their items in grants of `match_grant` positions from one cursor per
launch (`match_continuous`, the default), against the fixed-chunk form of the same build (`match_continuous` off) and the reference's goldens.
The feed decides which wavefront matches which item and nothing else: a raw record is a function of the item, and the counters of
kamd_align_stats that count probes are functions of index and reads.  The helpers and the tiled input are those of tests/test_gpu_match_forms.py.

`match_max_blocks` is reported as 0 where no cap is in force; a tuning field of 0 keeps its value, so the cap is taken away with a negative one."""
import numpy as np
import pytest

from tests import common, manyclass
from tests.test_gpu_match_forms import N_TILED, _assert_same_as_one_chunk, _opts, _packed, chunks_that_run
from tests.test_gpu_match_forms import DEFAULTS as FORM_DEFAULTS
from tests.test_gpu_match_forms import ka, oracle_prefix, tiled   # noqa: F401  (fixtures)
from tests.test_gpu_match_forms import ctxs as form_ctxs

pytestmark = pytest.mark.gpu

# the tuning a fresh context has for the fields these tests move; -1 takes the cap on the blocks away
DEFAULTS = dict(FORM_DEFAULTS, match_continuous=True, match_grant=256, match_max_blocks=-1)
FIXTURES = [("human_pe", "pe"), ("yeast_se", "se"), ("stress_pe", "pe"), ("dlist_pe", "pe"), ("k17_pe", "pe"), ("manyclass_pe", "pe")]
COUNTERS = ("n_probes", "n_bucket_reads", "n_text_hits", "n_raw_words")


@pytest.fixture(scope="module")
def ctxs(ka, form_ctxs, tmp_path_factory):
    """tests/test_gpu_match_forms.py's contexts, and one for manyclass_pe, whose index is committed gzipped"""
    own = {}

    def get(case, layout=None):
        if case != manyclass.NAME:
            return form_ctxs(case, layout)
        if "m" not in own:
            index = ka.Index(manyclass.unpack_index(tmp_path_factory.mktemp("manyclass")))
            ctx = ka.Context(0)
            ctx.upload(index)
            own["m"] = (index, ctx)
        else:
            own["m"][1].reset()
        return own["m"]
    yield get
    for _, c in own.values():
        c.close()


def _tune(ctx, **tune):
    """set the fields and check that they took effect (match_max_blocks: 0 asks for "no cap")"""
    send = {f: (-1 if f == "match_max_blocks" and v == 0 else v) for f, v in tune.items()}
    got = ctx.tune(**send)
    for f, v in tune.items():
        assert got[f] == ({True: 1, False: 2}[v] if isinstance(v, bool) else v), (f, got[f])


def _quant_and_check(ka, ctx, case, variant, **tune):
    """one quant of the whole fixture under `tune`: n_processed, the EC multiset, flens and eff_lens exact, est_counts at the suite's tolerance;
    returns (stats, profile)"""
    exp = common.load_expected(case, variant)
    o, words, lens, n, max_len = _packed(ctx, case, variant)
    try:
        _tune(ctx, **tune)
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


def _utilisation(stats):
    return stats["n_lane_iters"] / max(64 * stats["n_wave_iters"], 1)


@pytest.fixture(scope="module")
def fixed_form(ka, ctxs):
    """the fixed-chunk run of a fixture in this build, checked against the goldens like every other: (stats, profile), once per fixture"""
    cache = {}

    def get(case, variant):
        if (case, variant) not in cache:
            cache[(case, variant)] = _quant_and_check(ka, ctxs(case)[1], case, variant, match_continuous=False)
        return cache[(case, variant)]
    return get


def test_the_defaults(ka, ctxs):
    index, ctx = ctxs("human_pe")
    t = ctx.tune()
    assert (t["match_continuous"], t["match_grant"], t["match_max_blocks"]) == (1, 256, 0)
    try:
        assert ctx.tune(match_grant=63)["match_grant"] == 256          # below a wavefront's lanes: ignored
        assert ctx.tune(match_max_blocks=3)["match_max_blocks"] == 3
        assert ctx.tune(match_max_blocks=0)["match_max_blocks"] == 3   # 0 keeps
        assert ctx.tune(match_max_blocks=-1)["match_max_blocks"] == 0
    finally:
        ctx.tune(**DEFAULTS)


@pytest.mark.parametrize("case,variant", FIXTURES)
def test_fixed_chunk_form(case, variant, fixed_form):
    """match_continuous off launches the fixed chunks of items_per_wave items: the goldens (stress_pe: through the second pass, too)"""
    stats, prof = fixed_form(case, variant)
    assert stats["n_probes"] > 0
    if case == "stress_pe":
        assert prof["n_overflow_second_pass"] > 0, prof


@pytest.mark.parametrize("refill_min", [1, 64])
@pytest.mark.parametrize("items_per_wave", [64, 100, 1000])
@pytest.mark.parametrize("case", ["human_pe", "stress_pe"])
def test_fixed_chunk_form_shapes(case, items_per_wave, refill_min, ka, ctxs, fixed_form):
    """items_per_wave shapes the fixed-chunk form only, so its values are run here with match_continuous off: chunks of exactly one wavefront's
    lanes, chunks that end inside them, a refill at every free lane and only when all 64 are free -- in the first pass and in the second
    (stress_pe)."""
    index, ctx = ctxs(case)
    stats, prof = _quant_and_check(ka, ctx, case, "pe", match_continuous=False, items_per_wave=items_per_wave, refill_min=refill_min)
    for f in COUNTERS:
        assert stats[f] == fixed_form(case, "pe")[0][f], f
    if case == "stress_pe":
        assert prof["n_overflow_second_pass"] > 0, prof


@pytest.mark.parametrize("continuous", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batches_of_a_few_items(n, continuous, ka, ctxs, oracle_prefix):
    """the first n pairs of human_pe, n around a wavefront's lanes, with grants and chunks of 64: a launch whose only grant is one item, one short
    of a wavefront, full, and one more; in the fixed-chunk form the grid gains a wavefront for a single item"""
    meta, idx_path, r1, r2 = common.load_case("human_pe")
    index, ctx = ctxs("human_pe")
    words, lens, max_len = ctx.pack_reads_host(common.interleave(r1[:n], r2[:n]), 100)
    try:
        _tune(ctx, match_continuous=continuous, match_grant=64, items_per_wave=64)
        ctx.reset()
        ctx.pseudoalign(ka.QuantOpts(1, 0.0, 0.0, 0, 0), words, lens, n, max_len)
        ecs = ctx.finalize()
        n_proc = ctx.stats()["n_processed"]
    finally:
        ctx.tune(**DEFAULTS)
    assert n_proc == n
    assert {k: v for k, v in ecs.multiset().items() if v} == oracle_prefix("human_pe", "pe", n)


@pytest.mark.parametrize("max_blocks", [1, 2, 0])
@pytest.mark.parametrize("grant", [64, 100, 256])
@pytest.mark.parametrize("case,variant", FIXTURES)
def test_continuous_feed(case, variant, grant, max_blocks, ka, ctxs, fixed_form):
    """grants of exactly a wavefront's lanes, of no multiple of them and of the default size; one block (its four wavefronts take every grant), two
    (the grants interleave between blocks) and as many as are resident.  Paired and single-end items, the second pass over an item list
    (stress_pe), a D-list, ragged and 15-base mates and all-N reads (k17_pe), and a batch of fewer items than one grant for most wavefronts
    (manyclass_pe).  The result is the goldens'; the probe counters are those of the fixed-chunk run."""
    index, ctx = ctxs(case)
    stats, prof = _quant_and_check(ka, ctx, case, variant, match_continuous=True, match_grant=grant, match_max_blocks=max_blocks)
    fixed_stats, fixed_prof = fixed_form(case, variant)
    for f in COUNTERS:
        assert stats[f] == fixed_stats[f], (f, stats[f], fixed_stats[f])
    assert stats["n_probes"] > 0
    if case == "stress_pe":
        assert prof["n_overflow_second_pass"] == fixed_prof["n_overflow_second_pass"] > 0, prof


@pytest.mark.parametrize("layout", ["compact", "wide"])
def test_chunk_launches_have_their_own_cursors(layout, ka, tiled):
    """one tiled batch of 4 x 65 536 + 1234 items in four chunks: four launches of kernel A queued one behind the other on one stream, their
    cursors zeroed once in front of the first, each taking positions 0 .. of its own chunk from its own cursor.  A shared cursor would leave items of the later chunks unmatched: compare with the
    one-chunk run, whose classes, counts, order and fragment lengths must come out again."""
    t = tiled("human_pe", "pe", layout)
    assert chunks_that_run(4, N_TILED) == 4
    assert t.ctx.tune()["match_continuous"] == 1
    _assert_same_as_one_chunk(t.run(4), t.one_chunk, t.expected)


def test_grants_span_the_wavefronts_of_one_block(ka, ctxs, fixed_form):
    """match_max_blocks = 1, match_grant = 64 on human_pe: one block's four wavefronts consume every grant, each refilling its lanes across
    the boundaries of grants that are a single refill's worth of positions.  The result holds, and the lanes are busier than in the
    fixed-chunk run of the same input, whose wavefronts drain one by one at the end of their chunks."""
    index, ctx = ctxs("human_pe")
    stats, prof = _quant_and_check(ka, ctx, "human_pe", "pe", match_continuous=True, match_grant=64, match_max_blocks=1)
    fixed_stats, _ = fixed_form("human_pe", "pe")
    for f in COUNTERS:
        assert stats[f] == fixed_stats[f], (f, stats[f], fixed_stats[f])
    u, u_fixed = _utilisation(stats), _utilisation(fixed_stats)
    print(f"lane utilisation: continuous (one block, grants of 64) {u:.4f}, fixed chunks {u_fixed:.4f}")
    assert u > u_fixed, (u, u_fixed)
