"""Kernel A's long class lists (kallisto_amd/csrc/kamd_match.hip) on the manyclass_pe fixture (tests/golden/make_manyclass.py), route by route:
items of at most eight classes that k_classify finishes, items whose appended list of 9 .. 192 classes k_classify_long ranks three entries per
lane, and items that overflow again and go to the straight-line kernel.  Everything is integer-exact.  The items of tests/common.CASES append 31
classes at the most (the emulation, item by item): tests/test_gpu_parity.py::test_items_with_long_class_lists runs those and asserts only that the
route was taken.

The intermediate state -- dense counts, de-duplicated tuple records, explicit records of the positional filters, read between Context.pseudoalign
and finalize -- is compared with manyclass.ec_state_opts on the same packed reads: match_mate on the host, which shares none of the append,
compaction or ranking code.  Two things in which the device's state differs from that reference by design, not by content, are taken out before
the comparison: a long-list item whose classes map to ONE set leaves a tuple record of one set on the device (the long routes never count into the
dense vector) where the reference counts the set densely -- such records are folded into the dense vector; and the device's records are
de-duplicated with a count.  The sets of a record must be strictly ascending: a wrong rank shows there even where the multiset would match.

Which route an item takes is known from case.json (D, A, S per item, recomputed by tests/test_manyclass_fixture_cpu.py): D > 8 leaves the first
pass, A <= 192 stays in the second.  Every test runs under overflow_second_pass = 1 (second pass beside the absorption), 3 (after it) and 2
(straight-line kernel only)."""
from collections import Counter, namedtuple

import numpy as np
import pytest

from tests import common, emu_binding as E, manyclass as M

pytestmark = pytest.mark.gpu

Env = namedtuple("Env", "ka index ctx emu meta r1 r2")
SETTINGS = [1, 3, 2]
State = namedtuple("State", "dense tuples explicit prof")


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    import kallisto_amd as ka
    ka.load_library()
    path = M.unpack_index(tmp_path_factory.mktemp("manyclass"))
    index = ka.Index(path)
    ctx = ka.Context(0)
    ctx.upload(index)
    emu = E.EmuIndex(path)
    meta, r1, r2 = M.load_reads()
    yield Env(ka, index, ctx, emu, meta, r1, r2)
    ctx.close()
    emu.close()


def opts_of(env, variant):
    o = common.parse_variant(env.meta["variants"][variant])
    return o, env.ka.QuantOpts(o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"])


def pack(env, items, paired):
    """the chosen items packed once on the host (for the emulation) and copied to the device as they are"""
    torch = env.ctx.torch
    reads = [x for i in items for x in ((env.r1[i], env.r2[i]) if paired else (env.r1[i],))]
    words, l16, max_len = E.pack(reads, env.meta["max_read"])
    dev = f"cuda:{env.ctx.device}"
    return (words, l16, max_len), (torch.from_numpy(words.view(np.int32)).to(dev), torch.from_numpy(l16.view(np.int16)).to(dev))


def records(words, offs, union, what):
    """[count, m, e0 ..] records -> (Counter {set tuple: count} of the records of two or more sets, Counter {set id: count} of those of one)"""
    multi, single = Counter(), Counter()
    words = np.asarray(words).view(np.uint32).astype(np.int64)
    for o in np.asarray(offs).astype(np.int64).tolist():
        cnt, m = int(words[o]), int(words[o + 1])
        es = words[o + 2:o + 2 + m]
        ids = es & M.ID_MASK
        assert m >= 1 and (np.diff(ids) > 0).all(), f"{what}: the sets of a record are not strictly ascending: {es.tolist()}"
        assert union or (es == ids).all(), f"{what}: mate flags without --union"
        assert not union or ((es >> 30) != 0).all(), f"{what}: a set without a mate flag under --union"
        if m == 1:
            single[int(ids[0])] += cnt
        else:
            multi[tuple(es.tolist())] += cnt
    return multi, single


def device_state(env, union):
    ctx = env.ctx
    tw, to = ctx.tuples_export()
    multi, single = records(tw.cpu().numpy(), to.cpu().numpy(), union, "device")
    dense = ctx.dense_counts().cpu().numpy().astype(np.int64).copy()
    for e, c in single.items():
        dense[e] += c
    ew, eo = ctx.explicit_export()
    ew, explicit = ew.cpu().numpy().view(np.uint32), Counter()
    for o in eo.cpu().numpy().tolist():
        explicit[tuple(ew[o + 2:o + 2 + int(ew[o + 1])].tolist())] += int(ew[o])
    return State(dense, multi, explicit, ctx.profile())


def reference_state(env, host, n, o):
    """the straight-line host reference on the same packed reads; with the strand filter the items it changes become explicit records of the
    filtered set, the items it empties vanish"""
    words, l16, max_len = host
    paired = o["paired"]
    ids, explicit = None, Counter()
    has_fl = o["fld"] != 0.0
    if o["strand"] or (has_fl and not o["single_overhang"]):      # (kamd_pseudoalign: when the positional filters are on)
        mode = o["no_jump"] | (o["union"] << 1)
        off0, ids0 = E.pseudoalign_opts(env.emu, words, l16, n, paired, max_len, 1, 0, 0, 0, mode)
        off1, ids1 = E.pseudoalign_opts(env.emu, words, l16, n, paired, max_len, o["single_overhang"], o["strand"], int(o["fld"]), int(has_fl), mode)
        ids = []
        for i in range(n):
            a, b = ids0[off0[i]:off0[i + 1]], ids1[off1[i]:off1[i + 1]]
            if np.array_equal(a, b):
                ids.append(i)
            elif len(b):
                explicit[tuple(b.tolist())] += 1
    dense, stream, rec_off = M.ec_state_opts(env.emu, words, l16, n, paired, max_len, no_jump=o["no_jump"], union=o["union"], item_ids=ids)
    multi, single = records(stream, rec_off, o["union"], "reference")
    assert not single
    return State(dense.astype(np.int64), multi, explicit, None)


def run(env, items, variant, setting):
    """pseudoalign the chosen items under one overflow_second_pass setting: (device state, reference state)"""
    o, opts = opts_of(env, variant)
    host, (dw, dl) = pack(env, items, o["paired"])
    ctx = env.ctx
    ctx.tune(overflow_second_pass=setting)
    try:
        ctx.reset()
        ctx.pseudoalign(opts, dw, dl, len(items), host[2])
        got = device_state(env, o["union"])
    finally:
        ctx.tune(overflow_second_pass=True)      # (the default)
    return got, reference_state(env, host, len(items), o)


def assert_same_state(got, want, what=""):
    assert np.array_equal(got.dense, want.dense), f"{what}: dense counts differ at sets {np.flatnonzero(got.dense != want.dense)[:10].tolist()}"
    if got.tuples != want.tuples:
        miss, extra = want.tuples - got.tuples, got.tuples - want.tuples
        raise AssertionError(f"{what}: {len(miss)} tuple records missing, {len(extra)} unexpected; first missing "
                             f"{[(len(k), k[:6], v) for k, v in list(miss.items())[:3]]}, first unexpected {[(len(k), k[:6], v) for k, v in list(extra.items())[:3]]}")
    assert got.explicit == want.explicit, f"{what}: explicit records differ"


def figures(env, variant):
    f = env.meta["figures"]["se" if variant == "se" else "pe_nojump" if variant == "pe_nojump" else "pe"]
    return [M.Item(d, a, s, False, False, False, False) for d, a, s in zip(f["D"], f["A"], f["S"])]


def assert_routes(prof, figs, items, setting, what=""):
    routes = [M.route(figs[i]) for i in items]
    n_over = len(routes) - routes.count("first")
    assert prof["n_overflow_items"] == n_over, f"{what}: {prof['n_overflow_items']} items left the first pass, {n_over} have more than eight classes"
    want = routes.count("long") if setting != 2 else 0
    assert prof["n_overflow_second_pass"] == want, f"{what}: the second pass kept {prof['n_overflow_second_pass']} items, {want} append at most 192 classes"


VARIANTS = ["pe", "pe_union", "pe_fr", "pe_nojump", "se"]


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_intermediate_state_and_routes(variant, setting, env):
    """the whole fixture in one batch: the state before finalize is the reference's, and the device's counters of the routes are the emulation's"""
    items = list(range(env.meta["n"]))
    got, want = run(env, items, variant, setting)
    assert sum(want.tuples.values()) > 60 and max(len(k) for k in want.tuples) > M.LONG_CAP
    assert_same_state(got, want, variant)
    assert_routes(got.prof, figures(env, variant), items, setting, variant)
    if variant == "pe_union":
        flags = Counter(e >> 30 for k in got.tuples for e in k)
        assert flags[1] and flags[2] and flags[3]
    if variant == "pe_fr":
        assert sum(want.explicit.values()) >= 4 and len(want.explicit) >= 2


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_quant_gives_the_golden_result(variant, setting, env):
    o, opts = opts_of(env, variant)
    exp = common.load_expected(M.NAME, variant)
    ctx = env.ctx
    words, lens, max_len = ctx.pack_reads_host(common.interleave(env.r1, env.r2 if o["paired"] else None), env.meta["max_read"])
    ctx.tune(overflow_second_pass=setting)
    try:
        ctx.reset()
        res = env.ka.quant(ctx, opts, [(words, lens, len(env.r1), max_len)])
    finally:
        ctx.tune(overflow_second_pass=True)
    assert np.array_equal(env.index.target_lens, exp["lens"]) and res.n_processed == exp["nproc"]
    assert res.ecs.multiset() == exp["ecs"]
    assert np.array_equal(res.flens, exp["flens"])
    common.assert_abundance_close(res.est_counts, exp["alpha"], "est_counts")


def by_route(env, variant="pe"):
    figs = figures(env, variant)
    out = {"first": [], "long": [], "straight": []}
    for i, it in enumerate(figs):
        out[M.route(it)].append(i)
    return figs, out


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("n_over", [1, 7, 8, 9, 31, 32, 33])
def test_batches_of_n_overflow_items(n_over, setting, env):
    """k_classify_long takes eight items per wavefront and 32 per block: batches with one short of, exactly and one more than a wavefront's and a
    block's worth of overflow items, spread among items of the first pass"""
    figs, r = by_route(env)
    rng = np.random.default_rng(100 + n_over)
    n_straight = min(2, n_over // 4)
    over = rng.choice(r["long"], n_over - n_straight, replace=False).tolist() + rng.choice(r["straight"], n_straight, replace=False).tolist()
    items = over + rng.choice(r["first"], 20, replace=False).tolist()
    rng.shuffle(items)
    got, want = run(env, items, "pe", setting)
    assert_same_state(got, want, f"{n_over} overflow items")
    assert_routes(got.prof, figs, items, setting)


def wavefront_mixes(env):
    """groups of eight overflow items, one wavefront of k_classify_long each (batches of their own, so that nothing else shares the wavefront; the
    overflow items reach the kernel in the order k_classify's atomic counter hands out, the input order as a rule): a re-overflowing item first, in the
    middle or last, among long items of every kind"""
    g = env.meta["groups"]
    big = g["S>256"][0]
    base = []
    for name in ("long,S<=8,A>=150", "A=192", "long,mate_merge", "A=129", "long,cross_slice_dup", "long,mate2_revisit", "A=65"):
        base.append(next(i for i in g[name] if i not in base))
    return {"first": [big] + base, "middle": base[:4] + [big] + base[4:], "last": base + [big],
            "two_straight": [g["D=9,A>=193"][0]] + base[:3] + [g["A=193"][0]] + base[3:6]}


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("order", ["first", "middle", "last", "two_straight"])
@pytest.mark.parametrize("variant", ["pe", "pe_union", "pe_fr"])
def test_one_wavefront_of_mixed_items(variant, order, setting, env):
    """eight overflow items of one wavefront: items that overflow again (no record, listed for the straight-line kernel), items of nearly all
    duplicates, of exactly 192 classes, with merged mate flags -- and under the strand filter items that it removes, changes and leaves alone.
    The record offsets of the wavefront (one atomic for all eight) must leave every record whole."""
    items = wavefront_mixes(env)[order]
    if variant == "pe_fr":     # swap three of the ordinary items for one the filter empties and two it changes
        g = env.meta["groups"]
        items = list(items)
        swap = [g["long,filter_removed"][0], g["long,filter_changed"][0], g["long,filter_changed"][1]]
        slots = [j for j, i in enumerate(items) if M.route(figures(env, "pe")[i]) == "long"][-3:]
        for j, i in zip(slots, swap):
            items[j] = i
    assert len(items) == 8
    # (an item that pair_is_mapped refuses cannot reach this kernel on an index without empty sets -- case.json's note --: the unmapped pair and the
    # two-class pair that join the batch are finished by the first pass, between the eight)
    figs = figures(env, "pe")
    items = items[:3] + [next(i for i, it in enumerate(figs) if it.D == 0)] + items[3:6] + [next(i for i, it in enumerate(figs) if it.D == 2)] + items[6:]
    got, want = run(env, items, variant, setting)
    assert_same_state(got, want, order)
    assert_routes(got.prof, figures(env, variant), items, setting, order)


@pytest.mark.parametrize("setting", SETTINGS)
def test_input_order_does_not_matter(setting, env):
    items = list(range(env.meta["n"]))
    a, want = run(env, items, "pe", setting)
    rng = np.random.default_rng(5)
    for _ in range(2):
        rng.shuffle(items)
        b, _ = run(env, items, "pe", setting)
        assert_same_state(b, want, "shuffled")
        assert b.tuples == a.tuples and np.array_equal(b.dense, a.dense)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_first_pass_edge_batches(n, env):
    """items of 2 .. 8 classes only (D = 7, D = 8, eight classes visited forty times and more, classes that map to one set or to fewer sets than
    classes): k_classify alone, at batch sizes around its wavefront of 64 and its block of 256 items (the tail of the 16-byte copy loop)"""
    figs = figures(env, "pe")
    g = env.meta["groups"]
    pool = sorted(set(g["D=7"] + g["D=8"] + g["D=8,A>=40"] + g["D>=2,S=1"] + g["D=8,S<8"]))
    pool = [i for i in pool if figs[i].D <= M.FIRST_CAP]
    assert len(pool) >= 30
    rng = np.random.default_rng(n)
    items = [pool[j % len(pool)] for j in range(n)]
    rng.shuffle(items)
    got, want = run(env, items, "pe", 1)
    assert_same_state(got, want, f"{n} items")
    assert got.prof["n_overflow_items"] == 0 and sum(got.tuples.values()) + int(got.dense.sum()) == n
