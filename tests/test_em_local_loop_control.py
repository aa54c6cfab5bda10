"""The loop control of EMAlgorithm::run (src/EMAlgorithm.h:112-223) -- n_iter and min_rounds other than the defaults -- in
kamd_em_local::run on the CPU (the driver of the component-local form over several ranks, through tests/emu), against the oracle; and
what tests/test_gpu_em_loop_control.py shares with it: the cases, what they must exercise, the assertions of one run.  The matrices and
the binding are those of tests/test_em_local.py, which stays as it is."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import common
from tests.test_em_local import _gene_matrix, _run


def loop_cases(R, zero=True):
    """(n_iter, min_rounds) pairs for a matrix whose EM takes R rounds at the defaults (10000, 50), from R alone: the loop that runs out at and
    around the edges of a chunk of 64 rounds, the natural stop and its neighbours, and a stop that min_rounds places at s = B-2 .. B+1 around a
    chunk edge B (the first multiple of 64 that is at least R + 64: the matrix has long converged there, so the first round past min_rounds
    stops) -- with n_iter one short of the final round (s + 1), just enough for it (s + 2) and far beyond.  zero: the loop without rounds."""
    B = -(-(R + 64) // 64) * 64
    cases = [(1, 50), (2, 50), (63, 50), (64, 50), (65, 50), (128, 50), (200, 500)]
    cases += [(R - 1, 50), (R, 50), (R + 1, 50), (10000, 50), (10000, 0)]
    for s in (B - 2, B - 1, B, B + 1):
        cases += [(s + 1, s - 1), (s + 2, s - 1), (10000, s - 1)]
    if zero:
        cases.append((0, 50))
    return cases


def check_loop_inputs(em, R):
    """what the cases are meant to exercise, asserted on the oracle alone (em(n_iter, min_rounds) -> alpha, alpha_before_zeroes, rounds)"""
    B = -(-(R + 64) // 64) * 64
    assert em(10000, 50)[2] == R
    for s in (B - 2, B - 1, B, B + 1):
        assert em(10000, s - 1)[2] == s + 1, s                       # the first round past min_rounds stops, the final round follows
        _, abz, r = em(s + 1, s - 1)
        assert r == s + 1 and abz.any(), s                           # the same stop with no round left for the final one
    _, abz, r = em(R, 50)
    assert r == R and abz.any()                                      # the natural stop in the loop's last round
    assert not em(R - 1, 50)[1].any()                                # one round less: the loop runs out


def check_loop_case(got, want, cnt, n_iter, min_rounds, what):
    """one run against the oracle's: rounds, alpha (1e-9, the EM forms' tolerance; the zero pattern too), alpha_before_zeroes"""
    (alpha, abz, rounds), (alpha_o, abz_o, rounds_o) = got, want
    what = f"{what} (n_iter={n_iter}, min_rounds={min_rounds})"
    tiny = lambda x: np.where(np.abs(x) < 1e-200, 0.0, x)            # where a decaying value underflows to 0 depends on the summation order
    assert rounds == rounds_o, f"{what}: {rounds} rounds, oracle {rounds_o}"
    if abz_o.any():
        common.assert_abundance_close(alpha, alpha_o, f"alpha, {what}", rel=1e-9)
        common.assert_abundance_close(tiny(abz), tiny(abz_o), f"alpha_before_zeroes, {what}", rel=1e-9, floor=1e-12)
    else:                                                            # the loop ran out: nothing was clamped, nothing set
        assert not abz.any(), f"{what}: alpha_before_zeroes set although the loop ran out"
        common.assert_abundance_close(tiny(alpha), tiny(alpha_o), f"alpha, {what}", rel=1e-9)
    if n_iter >= 1:
        assert abs(alpha.sum() - float(cnt.sum())) < 1e-6 * float(cnt.sum()), f"{what}: the counts are not conserved"


@functools.lru_cache(maxsize=None)
def _gene_matrix_cached(n_genes, seed):
    return _gene_matrix(n_genes, seed)


@functools.lru_cache(maxsize=None)
def _gene_oracle(n_genes, seed, n_iter, min_rounds):
    """once per (matrix, case); the arrays are shared: nobody writes to them"""
    off, ids, cnt, eff, T = _gene_matrix_cached(n_genes, seed)
    return O.em_run(off, ids, cnt, eff, T, n_iter=n_iter, min_rounds=min_rounds)


@pytest.mark.parametrize("builder", [0, 2])
@pytest.mark.parametrize("chunk", [64, 16])
@pytest.mark.parametrize("n_genes,seed", [(300, 7), (60, 2)])
def test_loop_control_equals_the_oracle(n_genes, seed, chunk, builder):
    """kamd_em_local::run at every end the reference's loop has: it runs out; the stop rule holds and the clamped final round follows; the
    stop rule holds in the loop's LAST round -- no final round then, the result is that round's with the clamp applied and
    alpha_before_zeroes is set (before the fix: one round too many, alpha off by 3.6e-2 at n_iter = R = 464, by 4.3e-2 at R = 316 on the
    small matrix); no round at all (1/T for every transcript; before the fix 0 or the singleton count outside the groups)."""
    off, ids, cnt, eff, T = _gene_matrix_cached(n_genes, seed)
    em = lambda n_iter, min_rounds: _gene_oracle(n_genes, seed, n_iter, min_rounds)
    R = em(10000, 50)[2]
    check_loop_inputs(em, R)
    # builder 0: greedy packing into groups of a workgroup's LDS; builder 2: the data-parallel steps cut groups of about 400 entries, sliced ELLPACK
    plan = dict(budget=1 << 30, target=400) if builder else {}
    for n_iter, min_rounds in loop_cases(R):
        rc, a, abz, r, _, _ = _run(off, ids, cnt, eff, T, chunk=chunk, n_iter=n_iter, min_rounds=min_rounds, builder=builder, **plan)
        assert rc == 0
        check_loop_case((a, abz, r), em(n_iter, min_rounds), cnt, n_iter, min_rounds, f"chunk {chunk}, builder {builder}")
