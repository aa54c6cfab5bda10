"""Short tuples counted by k_classify under an exact tag (kamd_tuning.classify_counts_short, short_id_bits; kamd_core.h tuple_tag).

A tuple record of two sets, or of three whose ids fit short_id_bits, is its own tag in the table of distinct tuples: k_classify claims / finds the slot
and adds the count itself, the absorption pass (k_tup_absorb4 / k_tup_absorb) sees only the other tuple records, k_tup_store rebuilds the store's
record from the tag, k_tup_rehash re-tags from the store.  Checked here against the CPU emulation (emu_binding.ec_state + resolve): the finalized EC
multiset and the number of distinct tuples, for item counts around a wavefront / a tile of the persistent block, with exact and hashed three-set
tuples in one table, across a table growth, through the fail list (tup_max_probe = 1), and against the path with the switch off.
"""
import numpy as np
import pytest

from tests import common
from tests import emu_binding as E

pytestmark = pytest.mark.gpu

CASES = ["human_pe", "stress_pe"]
COUNTS = [1, 63, 64, 65, 257, None]   # one lane, a partial wavefront, a whole one, a second one, a second block, the fixture (several tiles per block: test_several_tiles_per_block)


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    kallisto_amd.load_library()
    return kallisto_amd


class _Case:
    """a fixture, its context, and the emulation's answer per item count (computed once, never changed)"""

    def __init__(self, ka, name):
        self.ka = ka
        self.meta, self.idx_path, self.r1, self.r2 = common.load_case(name)
        self.n = len(self.r1)
        self.index = ka.Index(self.idx_path)
        self.ctx = ka.Context(0)
        self.ctx.upload(self.index)
        self.emu = E.EmuIndex(self.idx_path)
        self.words, self.lens, self.max_len = self.ctx.pack_reads_host(common.interleave(self.r1, self.r2), 100)
        self.rec = ka.packed_record_words(self.max_len)
        self.ewords, self.el16, _ = E.pack(common.interleave(self.r1, self.r2), self.max_len)
        self._ref = {}

    def ref(self, n=None):
        """(EC multiset, distinct tuples as a set of id tuples) of the first n items"""
        n = self.n if n is None else n
        if n not in self._ref:
            dense, stream, rec_off = E.ec_state(self.emu, self.ewords, self.el16, n, 1, self.max_len)
            tuples = {tuple(stream[int(o) + 2:int(o) + 2 + int(stream[int(o) + 1])].tolist()) for o in rec_off}
            self._ref[n] = (E.resolve(self.emu, dense, stream, rec_off), tuples)
        return self._ref[n]

    def narrow_bits(self):
        """a width at which some three-set tuples of the fixture are exact and some are not: (bits, exact ones, others)"""
        top = sorted(max(t) for t in self.ref()[1] if len(t) == 3)
        assert top, "the fixture has no three-set tuple"
        bits = min(max(int(top[len(top) // 2]).bit_length() - 1, 4), 20)   # (2^bits <= the median of the tuples' largest ids)
        fit = sum(1 for x in top if x < (1 << bits))
        return bits, fit, len(top) - fit

    def run(self, cuts, counts_short=1, bits=20, max_probe=64, max_blocks=-1):
        """pseudoalign items [cuts[0], cuts[1]), [cuts[1], cuts[2]) .. as batches: (multiset, stats, profile).  counts_short: 1 = k_classify counts the
        short tuples and lists what it leaves, 3 = it counts them and the absorption pass walks every slot, 2 = off; max_blocks: k_classify's blocks"""
        ctx = self.ctx
        ctx.tune(classify_counts_short=int(counts_short), short_id_bits=bits, tup_max_probe=max_probe, classify_max_blocks=max_blocks)
        try:
            ctx.reset()
            opts = self.ka.QuantOpts(1, 0.0, 0.0, 0, 0)
            for a, b in zip(cuts[:-1], cuts[1:]):
                ctx.pseudoalign(opts, self.words[a * 2 * self.rec:b * 2 * self.rec], self.lens[2 * a:2 * b], b - a, self.max_len)
            ms = ctx.finalize(download=True).multiset()
            return ms, ctx.stats(), ctx.profile()
        finally:
            ctx.tune(classify_counts_short=1, short_id_bits=20, tup_max_probe=64, classify_max_blocks=-1)

    def close(self):
        self.ctx.close()
        self.emu.close()


@pytest.fixture(scope="module")
def cases(ka):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Case(ka, name)
        return cache[name]
    yield get
    for c in cache.values():
        c.close()


def _check(case, n, got, what):
    ms, st, _ = got
    want_ms, want_tuples = case.ref(n)
    assert st["n_distinct_tuples"] == len(want_tuples), f"{what}: {st['n_distinct_tuples']} distinct tuples, the emulation has {len(want_tuples)}"
    assert ms == want_ms, f"{what}: the EC multiset differs from the emulation's"


MODES = [1, 3]   # with the list of the items k_classify leaves / with the absorption pass walking every slot


@pytest.mark.parametrize("mode", MODES, ids=["list", "walk"])
@pytest.mark.parametrize("narrow", [False, True], ids=["bits20", "narrow"])
@pytest.mark.parametrize("n", COUNTS, ids=lambda n: "all" if n is None else str(n))
@pytest.mark.parametrize("name", CASES)
def test_item_counts_and_both_tag_forms(name, n, narrow, mode, cases):
    case = cases(name)
    bits, fit, rest = case.narrow_bits()
    assert fit > 0 and rest > 0, f"{name}: at {bits} bits {fit} three-set tuples are exact and {rest} are not"
    n_items = case.n if n is None else n
    got = case.run([0, n_items], counts_short=mode, bits=bits if narrow else 20)
    _check(case, n_items, got, f"{name} {n_items} items")
    st = got[1]
    short_recs = st["n_classify_counted"]
    assert short_recs <= st["n_multi"]
    if n is None:
        # the path ran, and with the narrow width both forms of a three-set tuple were in the table
        assert short_recs > 0, st
        if narrow:
            assert st["n_three_exact"] > 0 and st["n_three_hashed"] > 0, st
        else:
            assert st["n_three_exact"] > 0 and st["n_three_hashed"] == 0, st


@pytest.mark.parametrize("mode", MODES, ids=["list", "walk"])
@pytest.mark.parametrize("max_probe", [64, 1])
@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_several_tiles_per_block(name, blocks, max_probe, mode, cases):
    """k_classify held to one block (20 / 24 tiles of 256 items each, one after the other) and to three (7 or 8 tiles each, the last one partial): a
    wavefront carries the slots it claimed and its list of left items from tile to tile, appends its claims to the owners' list in the middle of the
    loop (more than 32 of them pending), and its segment of the list (1280 / 1536 entries with one block) takes more than one row of k_tup_absorb4's
    blocks; in one batch and in two, with exact and hashed three-set tags in the table"""
    case = cases(name)
    bits = case.narrow_bits()[0]
    for cuts in ([0, case.n], [0, 1500, case.n]):
        got = case.run(cuts, counts_short=mode, bits=bits, max_probe=max_probe, max_blocks=blocks)
        _check(case, case.n, got, f"{name} {blocks} block(s) max_probe {max_probe} {cuts}")
        st = got[1]
        assert st["n_classify_counted"] > 64 * blocks * 4 and st["n_three_exact"] > 0 and st["n_three_hashed"] > 0, st


@pytest.mark.parametrize("narrow", [False, True], ids=["bits20", "narrow"])
@pytest.mark.parametrize("first", [64, 4999])
@pytest.mark.parametrize("name", CASES)
def test_second_batch_meets_a_table_of_short_tags(name, first, narrow, cases):
    """first 64 items, then the rest: the second batch grows the table (tuples_resize, k_tup_rehash over exact and hashed tags) and finds the tuples of
    the first in the store; 4999 / 1: a batch that (almost) only repeats meets a full table"""
    case = cases(name)
    first = min(first, case.n - 1)
    bits = case.narrow_bits()[0] if narrow else 20
    got = case.run([0, first, case.n], bits=bits)
    _check(case, case.n, got, f"{name} {first} + {case.n - first} items")
    if first == 64:
        assert got[2]["tuple_table_slots"] > 1024, got[2]   # (the first batch's table: 1024 slots)


@pytest.mark.parametrize("narrow", [False, True], ids=["bits20", "narrow"])
@pytest.mark.parametrize("name", CASES)
def test_fail_list_and_retries(name, narrow, cases):
    """one probe per record: whatever does not find its tuple or an empty slot at its first slot goes through the fail list, the table grows, the
    record is tried again (k_tup_absorb over the fail list), in one batch and in two"""
    case = cases(name)
    bits = case.narrow_bits()[0] if narrow else 20
    for cuts in ([0, case.n], [0, 257, case.n]):
        got = case.run(cuts, bits=bits, max_probe=1)
        _check(case, case.n, got, f"{name} max_probe 1 {cuts}")
        assert got[2]["tuple_table_slots"] > 2048, got[2]   # (the table did grow: there were failures)


@pytest.mark.parametrize("name", CASES)
def test_switch_off_agrees_bitwise(name, cases, ka):
    case = cases(name)
    out = {}
    for on in (1, 3, 2):
        case.ctx.tune(classify_counts_short=on)
        try:
            case.ctx.reset()   # (quant accumulates into the context's EC state)
            res = ka.quant(case.ctx, ka.QuantOpts(1, 0.0, 0.0, 0, 0), [(case.words, case.lens, case.n, case.max_len)])
            st = case.ctx.stats()
        finally:
            case.ctx.tune(classify_counts_short=1)
        assert (st["n_classify_counted"] > 0) == (on != 2), st
        out[on] = (res.ecs.multiset(), st["n_distinct_tuples"], np.array(res.est_counts, copy=True))
    assert out[1][0] == out[3][0] == out[2][0] == case.ref()[0]
    assert out[1][1] == out[3][1] == out[2][1] == len(case.ref()[1])
    assert out[1][2].tobytes() == out[2][2].tobytes() == out[3][2].tobytes(), "est_counts differ between the forms of classify_counts_short"


@pytest.mark.parametrize("variant", ["pe_rf", "pe_union", "track_order"])
def test_other_paths_do_not_take_it(variant, cases, ka):
    """a positional filter, --union (mate flags in the ids) and first-occurrence keys keep the old path: nothing is counted in k_classify"""
    case = cases("stress_pe")
    index, ctx = case.index, ka.Context(0)
    try:
        ctx.upload(index)
        assert ctx.tune()["classify_counts_short"] == 1
        if variant == "track_order":
            o = common.parse_variant(case.meta["variants"]["pe"])
            exp = common.load_expected("stress_pe", "pe")
            ctx.track_order(True)
        else:
            o = common.parse_variant(case.meta["variants"][variant])
            exp = common.load_expected("stress_pe", variant)
        opts = ka.QuantOpts(o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"])
        ctx.pseudoalign(opts, case.words, case.lens, case.n, case.max_len)
        ms = ctx.finalize(download=True).multiset()
        st = ctx.stats()
        assert st["n_multi"] > 0 and st["n_classify_counted"] == 0 and st["n_three_exact"] == 0, st
        assert ms == exp["ecs"]
    finally:
        ctx.close()
