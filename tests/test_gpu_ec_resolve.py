"""Record absorption (kamd_ec_tuples_replace -> absorb_tuples) and EC resolution (kamd_ec_finalize) on transcript sets of up to 4340 members,
path by path, against plain set algebra on the host (tests/bigsets.py), and the whole quant flow on the same index against the reference.

The index is the bigsets_pe fixture (tests/golden/make_bigsets.py): the only one with sets of more than 128 members, so the only one on which
kamd_index_upload builds bitmaps and k_resolve_big<4096> and the plain path have work.  Records [count, m, e0..e(m-1)] are installed directly
(Context.tuples_replace), dense counts written into Context.dense_counts(); everything is integer-exact.  Which kernel path takes a tuple is
decided on the host from the sizes of its sets (bigsets.path_of restates k_bound_tuples / k_resolve / k_resolve_big) and asserted by every
test for its own tuples; `PATH <name>: <tuples>` lines (pytest -s) say how many tuples met each condition.

Not reachable: the LDS tile loop of k_resolve_big past its first tile of 1024 ids -- only a set of more than 1024 members WITHOUT a bitmap
gets there, which takes more than BM_MAX_BYTES (256 MB) of bitmaps.  And a tuple of more than 256 DISTINCT sets that are all larger than
4096 members does not exist in an index of 4400 targets that fits a committed file: that one case repeats set ids (say so where it does)."""
from collections import namedtuple

import numpy as np
import pytest

from tests import bigsets, common

pytestmark = pytest.mark.gpu

Env = namedtuple("Env", "ka index ctx sets holding")
INF = 1 << 30


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    import kallisto_amd as ka
    ka.load_library()
    index = ka.Index(bigsets.unpack_index(tmp_path_factory.mktemp("bigsets")))
    ctx = ka.Context(0)
    ctx.upload(index)
    sets = bigsets.sets_of_device_index(index)
    assert sets.onlist.all() and (sets.sizes > 0).all()
    t_of, e_of = np.nonzero(sets.matrix.T)               # grouped by target
    start = np.searchsorted(t_of, np.arange(sets.n_targets + 1))
    holding = [e_of[start[t]:start[t + 1]] for t in range(sets.n_targets)]
    yield Env(ka, index, ctx, sets, holding)
    ctx.close()


# ---- choosing sets on the host ----------------------------------------------------------------------------------------------------
def sized(env, ids, lo, hi=INF):
    ids = np.asarray(ids, np.int64)
    s = env.sets.sizes[ids]
    return ids[(s >= lo) & (s <= hi)]


def every(env, lo, hi=INF):
    return sized(env, np.arange(len(env.sets.sizes)), lo, hi)


def hold(env, t, lo=1, hi=INF):
    """the sets of lo..hi members that hold transcript t"""
    return sized(env, env.holding[t], lo, hi)


def richest(env, lo, hi=INF, k=1):
    """the k transcripts held by the most sets of lo..hi members"""
    n = env.sets.matrix[(env.sets.sizes >= lo) & (env.sets.sizes <= hi)].sum(axis=0)
    return [int(t) for t in np.argsort(-n, kind="stable")[:k]]


def pick(rng, pool, n):
    assert len(pool) >= n, (len(pool), n)
    return [int(x) for x in rng.choice(pool, n, replace=False)]


def shuffled(rng, es):
    es = list(es)
    rng.shuffle(es)
    assert len(set(es)) == len(es)       # distinct set ids in a tuple
    return es


def smallest(env, es):
    """(index, size) of the tuple's smallest set, the first one on ties (what the kernels take)"""
    s = env.sets.sizes[np.asarray(es, np.int64)]
    return int(np.argmin(s)), int(s.min())


def n_bitmap_others(env, es):
    """sets of the tuple that exist as bitmaps (more than BM_MIN_MEMBERS members), the smallest set not counted"""
    b, _ = smallest(env, es)
    return sum(1 for j, e in enumerate(es) if j != b and env.sets.sizes[e] > bigsets.BM_MIN_MEMBERS)


def paths(env, records):
    return [bigsets.path_of(env.sets, es) for _, es in records]


def report(name, n):
    print(f"PATH {name}: {n} tuples")


# ---- the helper: records + dense counts -> finalize ---------------------------------------------------------------------------------
def install(env, records):
    """records: (count, [set ids]) or None (a record slot whose offset is ~0: skipped) -> Context.tuples_replace"""
    torch = env.ctx.torch
    words, offs = [], []
    for r in records:
        if r is None:
            offs.append(-1)
            continue
        offs.append(len(words))
        words.append(int(r[0])); words.append(len(r[1])); words.extend(int(e) for e in r[1])
    w = torch.from_numpy(np.array(words or [0], np.int64).astype(np.uint32).view(np.int32)).to(f"cuda:{env.ctx.device}")
    o = torch.from_numpy(np.array(offs, np.int64)).to(f"cuda:{env.ctx.device}")
    env.ctx.tuples_replace(w[:len(words)], o)


def resolve(env, records, dense=None):
    torch = env.ctx.torch
    ctx = env.ctx
    ctx.reset()
    d = ctx.dense_counts()
    d.zero_()
    if dense:
        dev = f"cuda:{ctx.device}"
        d[torch.tensor(list(dense.keys()), dtype=torch.int64, device=dev)] = torch.tensor(list(dense.values()), dtype=torch.int32, device=dev)
    install(env, records)
    ecs = ctx.finalize()
    return ecs, ctx.profile(), int(ctx.ec_result.n_ecs), int(ctx.ec_result.nnz)


def check(env, records, dense, result):
    ecs, prof, n_ecs, nnz = result
    live = [r for r in records if r is not None]
    want = bigsets.expected_ecs(env.sets, live, dense)
    got = ecs.multiset()
    assert len(got) == len(ecs.counts), "the same member list twice in the result"
    if got != want:
        missing = [k for k in want if k not in got]
        extra = [k for k in got if k not in want]
        wrong = [(k[:8], len(k), want[k], got[k]) for k in want if k in got and got[k] != want[k]]
        raise AssertionError(f"multiset differs: {len(missing)} missing (sizes {sorted(len(k) for k in missing)[:10]}), {len(extra)} not expected "
                             f"(sizes {sorted(len(k) for k in extra)[:10]}), wrong counts (first ids, size, want, got) {wrong[:5]}")
    # ascending ids inside every EC
    inner = np.ones(len(ecs.ec_ids), bool)
    inner[ecs.ec_off[:-1].astype(np.int64)[ecs.ec_off[:-1] < len(inner)]] = False
    assert np.all(np.diff(ecs.ec_ids.astype(np.int64))[inner[1:]] > 0)
    assert n_ecs == len(want) and nnz == sum(len(k) for k in want)
    assert prof["n_distinct_tuples"] == len({tuple(es) for cnt, es in live if cnt})
    return want


def run(env, records, dense=None):
    return check(env, records, dense, resolve(env, records, dense))


def n_empty(env, records):
    return sum(1 for _, es in records if len(env.sets.intersect(es)) == 0)


# ---- tuple builders, one per path (used by the path tests and by the calls that mix the paths) ---------------------------------------
def all_pairs_tuples(env, seed=1):
    """m in 2..12, every set <= 16 members: sets with a common transcript (not empty), exactly 16 members, ties for the smallest, disjoint"""
    rng = np.random.default_rng(seed)
    recs = []
    for t in richest(env, 1, 16, 6):
        pool = hold(env, t, 1, 16)
        for m in range(2, 13):
            recs.append((int(rng.integers(1, 50)), shuffled(rng, pick(rng, pool, m))))
        sz = env.sets.sizes[pool]
        for s in np.unique(sz):
            same = pool[sz == s]
            larger = pool[sz > s]
            if len(same) >= 2 and len(larger):     # a tie for the smallest size
                recs.append((int(rng.integers(1, 50)), [int(same[0]), int(same[1]), int(larger[0])]))
                recs.append((int(rng.integers(1, 50)), [int(larger[0]), int(same[1]), int(same[0])]))
    for e in every(env, 16, 16):                 # sets of exactly 16 members, as the smallest and as another set
        t = int(env.sets.members(e)[0])
        others = [x for x in hold(env, t, 1, 16) if x != e]
        for m in (1, 2, min(len(others), 11)):
            if 1 <= m <= len(others):
                recs.append((int(rng.integers(1, 50)), shuffled(rng, [int(e)] + pick(rng, others, m))))
    for m in (2, 3, 7, 12):                      # disjoint: empty
        recs.append((int(rng.integers(1, 50)), pick(rng, every(env, 2, 16), m)))
    return recs


def chunk_mask_tuples(env, seed=2):
    """smallest set <= 16 members, not the all-pairs shape"""
    rng = np.random.default_rng(seed)
    recs, kinds = [], {}

    def add(kind, es):
        recs.append((int(rng.integers(1, 50)), es))
        kinds[kind] = kinds.get(kind, 0) + 1
    t_small = richest(env, 1, 16, 3)
    for t in t_small:
        pool = hold(env, t, 1, 16)
        for m in range(13, min(len(pool), 20) + 1):      # all sets <= 16: m 13..16 (one chunk of sets), 17.. (the serial scan for the smallest)
            add("m13_16_small" if m <= 16 else "m17_40", shuffled(rng, pick(rng, pool, m)))
    hub = richest(env, 17, INF, 1)[0]
    for t in [hub] + richest(env, 129, INF, 2) + richest(env, 65, 128, 2):
        small, short, bm = hold(env, t, 1, 16), hold(env, t, 17, 128), hold(env, t, 129)
        for s in pick(rng, small, min(len(small), 4)):
            for r in (1, 2, 5, 9, 15, 20, 30):
                if len(bm) >= r:
                    add("bitmaps_only", shuffled(rng, [s] + pick(rng, bm, r)))
                if len(short) >= r:
                    add("short_only", shuffled(rng, [s] + pick(rng, short, r)))
                if len(bm) >= r and len(short) >= r:
                    add("both", shuffled(rng, [s] + pick(rng, bm, r) + pick(rng, short, r)))
            big = hold(env, t, 17)
            for m in (17, 18, 31, 32, 33, 40):           # m 17..40: the serial scan, j0 advances
                if len(big) >= m - 1:
                    add("m17_40", shuffled(rng, [s] + pick(rng, big, m - 1)))
    for m in (2, 5, 17, 40):                             # empty: a small set and sets from anywhere
        add("disjoint", shuffled(rng, pick(rng, every(env, 1, 16), 1) + pick(rng, every(env, 17), m - 1)))
    return recs, kinds


def big1024_tuples(env, seed=3):
    """smallest set of 17..1024 members, at most 256 sets"""
    rng = np.random.default_rng(seed)
    sz = env.sets.sizes
    recs, kinds = [], {}

    def add(kind, es):
        recs.append((int(rng.integers(1, 50)), es))
        kinds[kind] = kinds.get(kind, 0) + 1
    hub = richest(env, 17, INF, 1)[0]
    # bitmap sets beside the smallest: 1, 2, 3, 4, 5, 9 (the min(b + q, nbm - 1) clamps), the smallest a short list or a bitmap set itself
    for t in [hub] + richest(env, 129, 1024, 3):
        for lo, hi in ((17, 128), (129, 1024)):
            for s in pick(rng, hold(env, t, lo, hi), min(len(hold(env, t, lo, hi)), 3)):
                larger = np.array([e for e in hold(env, t, 129) if sz[e] > sz[s]], np.int64)
                for nbm in (1, 2, 3, 4, 5, 9):
                    if len(larger) >= nbm:
                        add("bitmap_sets", shuffled(rng, [int(s)] + pick(rng, larger, nbm)))
    # more than 256 survivors enter the bitmap pass (its loop runs more than once)
    for s in every(env, 257, 1024):
        t = int(rng.choice(env.sets.members(s)))
        larger = np.array([e for e in hold(env, t, 129) if sz[e] > sz[s]], np.int64)
        for nbm in (1, 3, 6):
            if len(larger) >= nbm:
                add("over_256_survivors", shuffled(rng, [int(s)] + pick(rng, larger, nbm)))
    # short lists of 65..128 members meet more than 64 survivors: the LDS tile loop and its compaction
    short = every(env, 65, 128)
    cm = env.sets.matrix[short].astype(np.int32) @ env.sets.matrix[short].astype(np.int32).T
    for i, j in zip(*np.nonzero(np.triu(cm > 64, 1))):
        a, b = int(short[i]), int(short[j])
        t = int(env.sets.intersect([a, b])[0])
        add("tile_loop", [a, b])
        add("tile_loop", [b, a])
        more = [int(e) for e in hold(env, t, 65, 128) if e not in (a, b)]
        if more:
            add("tile_loop", shuffled(rng, [a, b] + more[:3]))
        add("tile_loop", shuffled(rng, [a, b] + pick(rng, hold(env, t, 129), 3)))     # (bitmap pass first, more than 64 left)
    # 64 or fewer survivors meet several open sets: the final all-pairs round with cnt * R > 64; no bitmap sets at all
    f17 = hold(env, hub, 17, 17)
    for r in (4, 5, 8, 30, 100, 255):
        add("final_round", pick(rng, f17, r + 1))
    for s in every(env, 64, 64):
        t = int(env.sets.members(s)[0])
        others = [int(e) for e in hold(env, t, 65, 128)]
        if len(others) >= 2:
            add("final_round", shuffled(rng, [int(s)] + others[:4]))
    for t in richest(env, 17, 64, 4):
        pool = hold(env, t, 17, 64)
        for m in (2, 3, 6, 12):
            if len(pool) >= m:
                add("final_round", shuffled(rng, pick(rng, pool, m)))
    # the smallest set has exactly 1024 members
    for s in every(env, 1024, 1024):
        for t in rng.choice(env.sets.members(s), 3, replace=False):
            for m in (1, 2, 6):
                larger = hold(env, int(t), 1025)
                add("exactly_1024", shuffled(rng, [int(s)] + pick(rng, larger, min(m, len(larger)))))
    # empty: disjoint sets of 129..1024 (bitmap pass), of 17..128 (LDS and final round)
    mid = every(env, 129, 1024)
    cmid = env.sets.matrix[mid].astype(np.int32) @ env.sets.matrix[mid].astype(np.int32).T
    for i, j in list(zip(*np.nonzero(np.triu(cmid == 0, 1))))[:6]:
        add("disjoint", [int(mid[i]), int(mid[j])])
        add("disjoint", [int(mid[j]), int(mid[i])] + pick(rng, every(env, 1025), 2))
    for m in (2, 3, 9):
        add("disjoint", pick(rng, every(env, 17, 64), m))
        add("disjoint", pick(rng, every(env, 65, 128), m))
    return recs, kinds


def big4096_tuples(env, seed=4):
    """smallest set of 1025..4096 members (every set of the tuple has more than 1024, so all of them are bitmaps)"""
    rng = np.random.default_rng(seed)
    sz = env.sets.sizes
    recs = []
    pool = every(env, 1025)
    for s in list(every(env, 1025, 1025)) + list(every(env, 4096, 4096)) + pick(rng, every(env, 1026, 4095), 8):
        larger = np.array([e for e in pool if sz[e] > sz[s]], np.int64)
        for m in (1, 2, 3, 5, 9):
            if len(larger) >= m:
                recs.append((int(rng.integers(1, 50)), shuffled(rng, [int(s)] + pick(rng, larger, m))))
    for m in (2, 3, 4, 8, 12, 20):
        recs.append((int(rng.integers(1, 50)), pick(rng, every(env, 1025), m)))
    return recs


def plain_tuples(env, seed=5):
    """smallest set beyond 4096 members (any number of sets), or more than 256 sets with the smallest beyond 16"""
    rng = np.random.default_rng(seed)
    recs, kinds = [], {}

    def add(kind, es):
        recs.append((int(rng.integers(1, 50)), es))
        kinds[kind] = kinds.get(kind, 0) + 1
    huge = [int(e) for e in every(env, 4097)]
    for m in range(2, len(huge) + 1):
        for _ in range(4):
            add("smallest_over_4096", pick(rng, huge, m))
    hub = richest(env, 17, INF, 1)[0]
    pool = hold(env, hub, 17)
    add("over_256_sets", pick(rng, hold(env, hub, 17, 17), 257))              # not empty: the hub group
    add("over_256_sets", pick(rng, pool, 257))
    add("over_256_sets", pick(rng, pool, 300))
    add("over_256_sets", shuffled(rng, pick(rng, pool, 300) + pick(rng, np.setdiff1d(every(env, 17), pool), 300)))   # 600 sets
    add("over_256_sets", pick(rng, every(env, 17), 257))                       # empty
    add("over_256_sets", pick(rng, every(env, 17), 1000))                      # (TUPLE_CAP_BIG is 1024)
    return recs, kinds, huge


# ---- the paths ------------------------------------------------------------------------------------------------------------------------
def test_all_pairs(env):
    recs = all_pairs_tuples(env)
    assert set(paths(env, recs)) == {"all_pairs"}
    ms = {len(es) for _, es in recs}
    assert ms >= set(range(2, 13))
    assert any(smallest(env, es)[1] == 16 for _, es in recs)
    ties = [es for _, es in recs if np.sort(env.sets.sizes[es])[0] == np.sort(env.sets.sizes[es])[1]]
    assert ties and 0 < n_empty(env, recs) < len(recs)
    report("all_pairs (m <= 12, every set <= 16)", len(recs))
    report("all_pairs: tie for the smallest size", len(ties))
    run(env, recs)


def test_chunk_mask_with_a_small_smallest_set(env):
    recs, kinds = chunk_mask_tuples(env)
    assert set(paths(env, recs)) == {"chunk_mask"}
    assert all(kinds.get(k, 0) > 0 for k in ("m13_16_small", "m17_40", "bitmaps_only", "short_only", "both", "disjoint")), kinds
    assert {len(es) for _, es in recs} >= {13, 14, 15, 16, 17, 40}
    assert 0 < n_empty(env, recs) < len(recs)
    for k, n in kinds.items():
        report(f"chunk_mask (smallest <= 16, not all-pairs): {k}", n)
    run(env, recs)


def test_boundary_16_17(env):
    """the same other sets with a smallest set of exactly 16 and of exactly 17 members: k_resolve keeps one, k_resolve_big<1024> takes the other"""
    rng = np.random.default_rng(6)
    hub = richest(env, 17, INF, 1)[0]
    s16, s17 = hold(env, hub, 16, 16), hold(env, hub, 17, 17)
    assert len(s16) and len(s17)
    recs = []
    for r_bm, r_short in ((1, 0), (0, 3), (3, 3), (9, 10)):
        others = pick(rng, hold(env, hub, 129), r_bm) + pick(rng, hold(env, hub, 18, 128), r_short)
        recs.append((3, [int(s16[0])] + others))
        recs.append((5, [int(s17[0])] + others))
        recs.append((7, others + [int(s17[1])]))
    p = paths(env, recs)
    assert p[0::3] == ["chunk_mask"] * 4 and p[1::3] == ["big1024"] * 4 and p[2::3] == ["big1024"] * 4
    report("boundary: smallest of exactly 16 (k_resolve) / exactly 17 (k_resolve_big<1024>), same other sets", len(recs))
    want = run(env, recs)
    assert len(want) >= 2


def test_resolve_big_1024(env):
    recs, kinds = big1024_tuples(env)
    assert set(paths(env, recs)) == {"big1024"}
    assert {n_bitmap_others(env, es) for _, es in recs} >= {0, 1, 2, 3, 4, 5, 9}
    # what each group is for, from the sets' sizes and the host's own intersections
    n256 = sum(1 for _, es in recs if smallest(env, es)[1] > 256 and n_bitmap_others(env, es) >= 1)
    n_tile = n_final = 0
    for _, es in recs:
        b, nb = smallest(env, es)
        bm = [e for j, e in enumerate(es) if j != b and env.sets.sizes[e] > bigsets.BM_MIN_MEMBERS]
        open_ = [e for j, e in enumerate(es) if j != b and env.sets.sizes[e] <= bigsets.BM_MIN_MEMBERS]
        left = len(env.sets.intersect([es[b]] + bm))
        if left > 64 and any(env.sets.sizes[e] >= 65 for e in open_):
            n_tile += 1
        if 0 < left <= 64 and left * len(open_) > 64:
            n_final += 1
    assert n256 >= 3 and n_tile >= 3 and n_final >= 3 and kinds.get("exactly_1024", 0) >= 3 and kinds.get("disjoint", 0) >= 6
    assert 0 < n_empty(env, recs) < len(recs)
    report("k_resolve_big<1024> (smallest 17..1024, m <= 256)", len(recs))
    report("k_resolve_big<1024>: more than 256 survivors enter the bitmap pass", n256)
    report("k_resolve_big<1024>: short lists of 65..128 meet more than 64 survivors (LDS tile loop)", n_tile)
    report("k_resolve_big<1024>: <= 64 survivors, cnt * R > 64 (final all-pairs round)", n_final)
    report("k_resolve_big<1024>: no bitmap sets at all", sum(1 for _, es in recs if n_bitmap_others(env, es) == 0))
    report("k_resolve_big<1024>: smallest of exactly 1024", kinds["exactly_1024"])
    run(env, recs)


def test_resolve_big_4096_beside_1024(env):
    """tuples of both instances of k_resolve_big in one call: both ends of the work list that k_bound_tuples writes are filled"""
    rng = np.random.default_rng(7)
    huge = big4096_tuples(env)
    assert set(paths(env, huge)) == {"big4096"}
    assert {smallest(env, es)[1] for _, es in huge} >= {1025, 4096}
    assert 0 < n_empty(env, huge) < len(huge)
    big = big1024_tuples(env)[0][:40]
    recs = huge + big
    recs = [recs[i] for i in rng.permutation(len(recs))]
    report("k_resolve_big<4096> (smallest 1025..4096, m <= 256)", len(huge))
    report("k_resolve_big<1024> in the same call", len(big))
    run(env, recs)


def test_plain_path(env):
    recs, kinds, huge = plain_tuples(env)
    assert set(paths(env, recs)) == {"plain"}
    over = [es for _, es in recs if len(es) > bigsets.RB_MAXSETS]
    assert {len(es) for es in over} >= {257, 600} and all(smallest(env, es)[1] > bigsets.RES_BIG_MIN for es in over)
    assert any(len(env.sets.intersect(es)) for es in over) and any(len(env.sets.intersect(es)) == 0 for es in over)
    assert sum(1 for _, es in recs if smallest(env, es)[1] > bigsets.RB_CAND_HUGE) >= 10
    assert any(env.sets.sizes[e] == 4097 for e in huge) and len(huge) >= 3
    # both properties at once: more than 256 sets, all beyond 4096 members.  There are only len(huge) such sets: THIS tuple repeats them
    # (the intersection is the same; a record of the library never repeats a set, the kernel does not rely on that)
    both = (11, [huge[i % len(huge)] for i in range(257)])
    assert bigsets.path_of(env.sets, both[1]) == "plain" and smallest(env, both[1])[1] > bigsets.RB_CAND_HUGE
    for k, n in kinds.items():
        report(f"plain path: {k}", n)
    report("plain path: more than 256 sets AND smallest beyond 4096 (repeated set ids)", 1)
    run(env, recs + [both])


def test_empty_intersections_leave_their_neighbours_alone(env):
    """every path in one call, empty and non-empty tuples side by side: an empty one does not appear and the slots next to it are intact"""
    rng = np.random.default_rng(8)
    parts = {"all_pairs": all_pairs_tuples(env, 11), "chunk_mask": chunk_mask_tuples(env, 12)[0], "big1024": big1024_tuples(env, 13)[0],
             "big4096": big4096_tuples(env, 14), "plain": plain_tuples(env, 15)[0]}
    for name, recs in parts.items():
        assert set(paths(env, recs)) == {name}
        assert 0 < n_empty(env, recs) < len(recs), name
        report(f"empty intersections on {name}", n_empty(env, recs))
    recs = [r for p in parts.values() for r in p]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    run(env, recs)


# ---- merging, skipped records, dense singles ------------------------------------------------------------------------------------------
def test_merging(env):
    rng = np.random.default_rng(9)
    hub = richest(env, 17, INF, 1)[0]
    f17 = hold(env, hub, 17, 17)
    g = int(hold(env, hub, 16, 16)[0])
    a, b, c, d = (int(x) for x in f17[:4])
    assert env.sets.intersect([a, b]).tolist() == env.sets.intersect([c, d]).tolist() == env.sets.members(g).tolist()
    huge = [int(e) for e in every(env, 4097)][:2]
    recs = [(3, [a, b]), (4, [c, d]), (5, [b, a]),          # different tuples, the same intersection -- which is also dense set g's
            (2, huge), (6, huge[::-1]),
            (7, [a, c, d]), (7, [a, c, d]), (1, [a, c, d])]  # the same record three times
    want = run(env, recs, {g: 100})
    assert want[tuple(env.sets.members(g).tolist())] == 3 + 4 + 5 + 7 + 7 + 1 + 100
    assert want[tuple(env.sets.intersect(huge).tolist())] == 8 and len(want) == 2


def test_skipped_records(env):
    """records with count 0 and record slots whose offset is ~0 have no effect"""
    base = all_pairs_tuples(env, 21)[:20] + big1024_tuples(env, 22)[0][:20]
    want = run(env, base)
    recs, dead = [], big4096_tuples(env, 23)
    for i, r in enumerate(base):
        recs.append(None)
        recs.append(r)
        recs.append((0, dead[i % 5][1]))       # count 0: not a record
        if i % 3 == 0:
            recs.append((0, r[1]))
    recs += [None, None]
    assert run(env, recs) == want


def test_dense_singles(env):
    rng = np.random.default_rng(10)
    sz = env.sets.sizes
    dense = {}
    for lo, hi in ((1, 1), (16, 16), (64, 64), (65, 65), (129, 129), (1025, 1025), (4097, INF)):
        for e in every(env, lo, hi)[:3]:
            dense[int(e)] = int(rng.integers(1, 1000))
    for e in pick(rng, every(env, 1), 300):
        dense.setdefault(e, int(rng.integers(1, 1000)))
    for e in list(dense):                       # zero counts on the neighbours
        for nb in (e - 1, e + 1):
            if 0 <= nb < len(sz) and nb not in dense:
                dense[nb] = 0
    assert sum(1 for e, c in dense.items() if c and sz[e] > 64) >= 10
    report("k_cand_singles: sets of more than 64 members (wavefront copy)", sum(1 for e, c in dense.items() if c and sz[e] > 64))
    report("k_cand_singles: sets of at most 64 members", sum(1 for e, c in dense.items() if c and sz[e] <= 64))
    want = run(env, [], dense)
    assert len(want) == sum(1 for c in dense.values() if c)
    # beside tuples: a tuple's slot follows what the singles allocated
    run(env, big1024_tuples(env, 24)[0][:30] + plain_tuples(env, 25)[0][:5], dense)


# ---- absorption ------------------------------------------------------------------------------------------------------------------------
def test_table_growth(env):
    """30 000 pairwise distinct records in one call: the table starts at a quarter of the record count (8192 slots), so records land on the fail
    list and the table grows fourfold, twice (32 768 slots cannot seat 30 000 tuples within 64 probes) -- tuples_resize + k_tup_rehash with a
    populated store, then the failed records again through the index list"""
    rng = np.random.default_rng(12)
    special = all_pairs_tuples(env, 31)[:30] + big1024_tuples(env, 32)[0][:30] + big4096_tuples(env, 33)[:10] + plain_tuples(env, 34)[0][:6]
    seen, recs = set(), []
    for r in special:                  # the builders may give the same tuple twice (a tie written for two transcripts): once here
        if tuple(r[1]) not in seen:
            seen.add(tuple(r[1]))
            recs.append(r)
    n = 30000
    ts = rng.integers(0, env.sets.n_targets, 4 * n)
    for t in ts:
        pool = env.holding[int(t)]
        pool = pool[env.sets.sizes[pool] <= 64]
        m = int(rng.integers(2, 5))
        if len(pool) < m:
            continue
        es = tuple(int(x) for x in rng.choice(pool, m, replace=False))
        if es in seen:
            continue
        seen.add(es)
        recs.append((int(rng.integers(1, 9)), list(es)))
        if len(recs) >= n + len(special):      # (at least) n beside the special ones
            break
    assert len(recs) >= n and len(seen) == len(recs)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    ctx = env.ka.Context(0)        # a context of its own: the table of the shared one has whatever size the tests before left it
    try:
        ctx.upload(env.index)
        own = env._replace(ctx=ctx)
        result = resolve(own, recs)
        check(own, recs, None, result)
    finally:
        ctx.close()
    prof = result[1]
    assert prof["n_distinct_tuples"] == len(recs)
    assert prof["tuple_table_slots"] >= 2 * prof["n_distinct_tuples"], prof
    report("absorption with table growth: pairwise distinct records", len(recs))


def test_second_call_replaces_the_first(env):
    first = big1024_tuples(env, 41)[0][:50] + all_pairs_tuples(env, 42)[:50]
    second = big4096_tuples(env, 43)[:10] + chunk_mask_tuples(env, 44)[0][:50]
    dense = {int(every(env, 129, 129)[0]): 9}
    run(env, first, dense)
    install(env, second)                         # no reset in between: the dense counts stay, the tuples of the first call do not
    ecs = env.ctx.finalize()
    check(env, second, dense, (ecs, env.ctx.profile(), int(env.ctx.ec_result.n_ecs), int(env.ctx.ec_result.nnz)))


# ---- the whole flow on the fixture -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads():
    return bigsets.load_reads()


def quant_case(env, reads, variant):
    meta, r1, r2 = reads
    o = common.parse_variant(meta["variants"][variant])
    exp = common.load_expected(bigsets.NAME, variant)
    ctx = env.ctx
    words, lens, max_len = ctx.pack_reads_host(common.interleave(r1, r2 if o["paired"] else None))
    opts = env.ka.QuantOpts(o["paired"], o["fld"], o["sd"], o["single_overhang"], o["strand"], o["no_jump"], o["union"])
    ctx.reset()
    res = env.ka.quant(ctx, opts, [(words, lens, len(r1), max_len)])
    assert np.array_equal(env.index.target_lens, exp["lens"])
    assert res.n_processed == exp["nproc"]
    assert res.ecs.multiset() == exp["ecs"]
    assert np.array_equal(res.flens, exp["flens"])
    assert np.array_equal(res.eff_lens, exp["eff"])
    common.assert_abundance_close(res.est_counts, exp["alpha"], "est_counts")
    return res


@pytest.mark.parametrize("variant", ["pe", "se"])
def test_quant_matches_reference_on_large_sets(variant, env, reads):
    quant_case(env, reads, variant)
    assert env.ctx.profile()["n_distinct_tuples"] > 0


@pytest.mark.parametrize("second_pass", [1, 2, 3])
def test_quant_with_each_overflow_form(second_pass, env, reads):
    env.ctx.tune(overflow_second_pass=second_pass)
    try:
        quant_case(env, reads, "pe")
    finally:
        env.ctx.tune(overflow_second_pass=True)


def test_quant_in_four_batches(env, reads):
    meta, r1, r2 = reads
    exp = common.load_expected(bigsets.NAME, "pe")
    ctx = env.ctx
    opts = env.ka.QuantOpts(1, 0.0, 0.0, 0, 0)
    n = len(r1)
    cuts = [0, 1, 257, 1000, n]
    ctx.reset()
    for a, b in zip(cuts[:-1], cuts[1:]):
        words, lens, max_len = ctx.pack_reads_host(common.interleave(r1[a:b], r2[a:b]), 75)
        ctx.pseudoalign(opts, words, lens, b - a, max_len)
    assert ctx.finalize().multiset() == exp["ecs"]
    assert ctx.stats()["n_processed"] == n
