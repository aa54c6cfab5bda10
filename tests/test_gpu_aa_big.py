"""Translated search on the GPU beyond the sizes of tests/test_gpu_aa.py: wavefronts of k_aa_match that take several groups of eight reads, calls of more than
one chunk, reads long enough that the class-list scratch bounds the grid, frames of up to 65 535 bases.  The workloads are those of tests/aa_big.py; every
expected value is the CPU emulation's of the distinct reads (aa_big.expected_for), every comparison is exact, and which path a call took is read from
kamd_aa_stats (last_chunks, last_match_blocks, last_list_cap), not recomputed here."""
import random

import numpy as np
import pytest

from tests import aa_big as B
from tests import aa_common as A

pytestmark = pytest.mark.gpu
STATS = ("n_processed", "n_winner", "n_all_empty", "n_rejected_offlist", "n_frame_clashes")


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    return kallisto_amd


@pytest.fixture(scope="module")
def contexts(ka):
    """one context per fixture index, and the fixture's reads packed once on each as rows of one record"""
    fx = A.fixture()
    out = {}
    for v in A.VARIANTS:
        ctx = ka.Context(0)
        ctx.upload(ka.Index(fx[v]["index"]))
        words, lens, max_len = ctx.pack_reads_host(fx["reads"])
        out[v] = (ctx, words.view(len(fx["reads"]), -1), lens, max_len)
    return out


def _take(ctx, rows, lens, order):
    """the batch `order` of the packed reads, built on the device by row-indexing"""
    idx = ctx.torch.as_tensor(np.asarray(order, np.int64), device=rows.device)
    return rows[idx].contiguous().view(-1), lens[idx].contiguous()


def _run(ctx, words, lens, n, max_len, calls=None):
    """reset, the n reads in calls of the given sizes (one call by default), finalize -> (multiset without zero counts, stats, last_* of every call)"""
    rec = words.numel() // n
    ctx.reset()
    a, paths = 0, []
    for m in calls or [n]:
        ctx.pseudoalign_aa(words[a * rec:(a + m) * rec], lens[a:a + m], m, max_len)
        st = ctx.aa_stats()
        paths.append((st["last_chunks"], st["last_match_blocks"], st["last_list_cap"]))
        a += m
    assert a == n
    ecs = ctx.finalize()
    return {k: c for k, c in ecs.multiset().items() if c}, ctx.aa_stats(), paths


def _assert_expected(ms, st, want):
    assert {k: st[k] for k in STATS} == {k: want[k] for k in STATS}
    assert ms == want["multiset"]
    assert sum(c for s, c in ms.items() if len(s) == 1) == want["n_unique"]


def _several_groups_per_wavefront(n, blocks):
    """every wavefront of the launch (blocks of four) comes round its loop at least twice, and one a third time"""
    return -(-n // 8) >= 2 * blocks * 4 + 1


# ---- the persistent loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", A.VARIANTS)
def test_wavefronts_take_several_groups(contexts, variant):
    ctx, rows, lens, max_len = contexts[variant]
    n = 100003
    order = B.many_reads()[:n]
    want = B.expected_for(B.emulated_fixture(variant), order)
    w, l = _take(ctx, rows, lens, order)
    ms, st, paths = _run(ctx, w, l, n, max_len)
    (chunks, blocks, cap), = paths
    assert chunks == 1
    assert _several_groups_per_wavefront(n, blocks), (n, blocks)   # (a card with so many CUs that this fails needs a larger n here: fail, do not skip)
    _assert_expected(ms, st, want)
    # the same entries in three calls: other groups, other wavefronts, the same answer
    ms3, st3, paths3 = _run(ctx, w, l, n, max_len, [40001, 40001, 20001])
    assert [p[0] for p in paths3] == [1, 1, 1]
    _assert_expected(ms3, st3, want)
    assert ms3 == ms


# ---- the chunk loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", A.VARIANTS)
def test_a_call_of_more_than_one_chunk(contexts, variant):
    fx = A.fixture()
    ctx, rows, lens, max_len = contexts[variant]
    emu = B.emulated_fixture(variant)
    order = B.many_reads()
    w, l = _take(ctx, rows, lens, order)
    rec = rows.shape[1]
    for n, chunks in ((262144, 1), (262145, 2), (len(order), 2)):   # (262 145: the second chunk holds one read)
        ms, st, paths = _run(ctx, w[:n * rec], l[:n], n, max_len)
        assert paths[0][0] == chunks, (n, paths)
        _assert_expected(ms, st, B.expected_for(emu, order[:n]))
    # nothing is left behind: a second finalize after the large call, then the fixture alone
    again = {k: c for k, c in ctx.finalize().multiset().items() if c}
    assert again == ms == B.expected_for(emu, order)["multiset"]
    n0 = len(fx["reads"])
    ms0, st0, paths0 = _run(ctx, rows.view(-1), lens, n0, max_len)
    assert paths0[0][0] == 1
    assert ms0 == fx[variant]["multiset"] and st0["n_processed"] == n0
    _assert_expected(ms0, st0, B.expected_for(emu, np.arange(n0)))


def test_cfc_frames_of_more_than_one_chunk(contexts):
    ctx = contexts["plain"][0]
    torch = ctx.torch
    base = A.frame_test_reads(random.Random(5))
    ow, ol, max_len = A.emu_frames(base)   # the CPU translation of the distinct reads
    nb = len(base)
    rec = len(ow) // (6 * nb)
    n = 262144 + 11
    words, lens, ml = ctx.pack_reads_host(base, max_len)
    assert ml == max_len == 97
    idx = torch.arange(n, device=words.device) % nb
    gw, gl = ctx.cfc_frames(words.view(nb, rec)[idx].contiguous().view(-1), lens[idx].contiguous(), n, max_len)
    reps = -(-n // nb)
    want_w = np.tile(ow[:6 * nb * rec], reps)[:6 * n * rec]
    want_l = np.tile(ol[:6 * nb], reps)[:6 * n]
    assert np.array_equal(gl.cpu().numpy().view(np.uint16), want_l)
    assert np.array_equal(gw.cpu().numpy().view(np.uint32), want_w)


# ---- long reads -----------------------------------------------------------------------------------------------------
def test_cfc_frames_of_long_reads(contexts):
    ctx = contexts["plain"][0]
    for max_len, reads, ow, ol in B.emulated_frames_long():
        rec = len(ow) // (6 * len(reads))
        for n in (1, 9, len(reads)):
            words, lens, ml = ctx.pack_reads_host(reads[:n], max_len)
            assert ml == max_len
            gw, gl = ctx.cfc_frames(words, lens, n, max_len)
            assert np.array_equal(gl.cpu().numpy().view(np.uint16), ol[:6 * n]), (max_len, n)
            assert np.array_equal(gw.cpu().numpy().view(np.uint32), ow[:6 * n * rec]), (max_len, n)


@pytest.fixture(scope="module")
def long_packed(contexts):
    """the distinct long reads packed once on each context"""
    reads = list(B.long_reads())
    out = {}
    for v in A.VARIANTS:
        ctx = contexts[v][0]
        words, lens, max_len = ctx.pack_reads_host(reads)
        assert max_len == B.LONG_LEN
        out[v] = (words.view(len(reads), -1), lens)
    return out


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_long_reads_bound_the_grid_by_scratch(contexts, long_packed, variant):
    ctx = contexts[variant][0]
    rows, lens = long_packed[variant]
    emu = B.emulated_long(variant)
    nd, max_len = rows.shape[0], B.LONG_LEN
    # the batch must give every wavefront two groups and one a third: n >= 2 x (blocks x 4 x 8) + 9, with the blocks a call of that size gets.  A small call
    # gets few blocks, so the size is grown until the grid no longer follows it.
    n = nd
    for _ in range(8):
        w, l = _take(ctx, rows, lens, B.long_batch(nd, n))
        blocks = _run(ctx, w, l, n, max_len)[2][0][1]
        if _several_groups_per_wavefront(n, blocks):
            break
        n = 2 * blocks * 32 + 9
    assert n < 100000, "the grid keeps growing with the batch: the scratch bound never binds"
    order = B.long_batch(nd, n)
    want = B.expected_for(emu, order)
    assert sum(c for s, c in want["multiset"].items()) > 0 and want["n_rejected_offlist"] + want["n_all_empty"] > 0
    w, l = _take(ctx, rows, lens, order)
    ms, st, paths = _run(ctx, w, l, n, max_len)
    (chunks, blocks, cap), = paths
    assert chunks == 1 and cap == 871
    assert blocks < 4 * ctx.torch.cuda.get_device_properties(ctx.device).multi_processor_count   # the scratch bound is the one that bound
    assert _several_groups_per_wavefront(n, blocks), (n, blocks)
    _assert_expected(ms, st, want)
    # calls of 5 003: another grid against the same scratch buffer
    calls = [5003] * (n // 5003) + ([n % 5003] if n % 5003 else [])
    ms2, st2, paths2 = _run(ctx, w, l, n, max_len, calls)
    assert all(p[2] == 871 for p in paths2) and paths2[0][1] != blocks
    _assert_expected(ms2, st2, want)
    assert ms2 == ms
