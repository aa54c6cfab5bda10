"""The loop control of EMAlgorithm::run (src/EMAlgorithm.h:112-223) in every EM form on the device: kamd_em_run / kamd_em_run_comm with
n_iter and min_rounds other than the defaults, against the oracle's restatement of the loop (ko_em_run) and nothing else.

The rule is written out in four places -- em_next_round + the read-out of em_run_impl (streamed and CSR forms), em_sell_drive_async (component-
local form and hybrid on one rank), kamd_em_local::run (component-local form over several ranks) and the rewind / replay of the partitioned
run -- and every other GPU test stops "somewhere inside a chunk, far below n_iter".  Here the loop runs out at and around the edges of a chunk
of 64 rounds, min_rounds delays the stop onto such an edge, and the stop falls on the loop's last round: no final round runs then, the result is
that round's alpha with the clamp applied (< 1e-8 -> 0), alpha_before_zeroes is set and rounds == n_iter.

Measured on the parent of the commit that added this file (MI355X): all eight single-rank forms and all three two-rank runs, on both ranks,
failed exactly the cases with stop + 1 == n_iter -- (R, 50) and the four (s + 1, s - 1) -- with the right rounds and alpha_before_zeroes but
alpha off by 2.4e-2 .. 3.8e-2 (the streamed and CSR forms returned the vector one round BEFORE the stop, unclamped; the component-local form
and the hybrid ran a final round the reference does not run); every single-rank form failed (0, 50) (0 or the singleton counts instead
of 1/T).  The other 19 cases passed in every form."""
import functools
import os
import sys

import numpy as np
import pytest

from tests.test_em_local import _gene_matrix
from tests.test_em_local_loop_control import check_loop_case, check_loop_inputs, loop_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _matrix(name):
    """G: gene-sized components only; F: one giant component with long rows and hub columns; H: gene-sized components beside one component
    beyond a workgroup's LDS (a smaller cut of the hybrid matrix of test_em_forms_agree_with_oracle; rows distinct, as kamd_ec_upload wants)"""
    from tests.test_gpu_parity import _distinct_rows, _family_csr, _hybrid_csr
    if name == "G":
        return _gene_matrix(300, 7)
    if name == "F":
        return _family_csr(400, 7)
    return _distinct_rows(*_hybrid_csr(600, 11, 100))


@functools.lru_cache(maxsize=None)
def _oracle(name, n_iter, min_rounds):
    """the yardstick, once per (matrix, case); the arrays are shared: nobody writes to them"""
    from oracle import oracle as O
    off, ids, cnt, eff, T = _matrix(name)
    return O.em_run(off, ids, cnt, eff, T, n_iter=n_iter, min_rounds=min_rounds)


@functools.lru_cache(maxsize=None)
def _cases(name, zero):
    """the (n_iter, min_rounds) pairs of a matrix, from the oracle alone, with what they are meant to exercise asserted on the oracle first"""
    em = lambda n_iter, min_rounds: _oracle(name, n_iter, min_rounds)
    R = em(10000, 50)[2]
    check_loop_inputs(em, R)
    return tuple(loop_cases(R, zero=zero))


_HYBRID = lambda p: p["em_k"] == -2 and p["em_grid"] > 1 and p["em_giant_nnz"] > 0
_LOCAL = lambda p: p["em_k"] in (-1, -2) and p["em_grid"] > 1
FORMS = {
    # form: (tuning, matrix, what the profile of a run must show)
    "streamed": (dict(em_form="streamed"), "F", lambda p: p["em_k"] > 0),
    "streamed_k8": (dict(em_form="streamed", em_entries_per_lane=8), "F", lambda p: p["em_k"] == 8),
    "csr": (dict(em_form="csr"), "F", lambda p: p["em_k"] == 0),
    "local": (dict(em_form="local", em_group_div=64), "G", _LOCAL),
    "local_wave": (dict(em_form="local", em_group_div=64, em_small_nnz=40), "G", _LOCAL),
    "hybrid": (dict(em_form="local"), "H", lambda p: _HYBRID(p) and p["em_giant_pieces"] > 0),
    "hybrid_plain": (dict(em_form="local", em_blocked=False), "H", lambda p: _HYBRID(p) and p["em_giant_pieces"] == 0),
    "hybrid_nograph": (dict(em_form="local", em_graph=False), "H", lambda p: _HYBRID(p) and p["em_giant_pieces"] > 0),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_loop_control_on_one_rank(form):
    import torch
    import kallisto_amd as ka
    ka.load_library()
    tune, name, ran = FORMS[form]
    off, ids, cnt, eff, T = _matrix(name)
    cases = _cases(name, True)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
    csr = (d(off, np.int64), d(ids, np.int32), d(cnt, np.int32))
    ctx = ka.Context(0)
    try:
        ctx.tune(**tune)
        for i, (n_iter, min_rounds) in enumerate(cases):
            got = ctx.em_run(eff, n_iter=n_iter, min_rounds=min_rounds, csr=csr)
            if i == 0:
                prof = ctx.profile()
                assert ran(prof), f"{form}: another form ran: {prof}"
            check_loop_case(got, _oracle(name, n_iter, min_rounds), cnt, n_iter, min_rounds, form)
    finally:
        ctx.close()


# the two-rank runs: (matrix, form of the partitioned EM)
RUNS = (("G", "local"), ("G", "streamed"), ("H", "local"))


def _loop_worker(rank, world, port, runs, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kallisto_amd as ka
        out = []
        for name, form, cases in runs:
            off, ids, cnt, eff, T = _matrix(name)
            ctx = ka.Context(0)
            try:
                ctx.tune(em_form=form)
                ctx.ec_upload(off, ids, cnt)
                comm = ka.Comm.over_process_group(ctx)
                res = [ctx.em_run_comm(comm, eff, n_iter, min_rounds) for n_iter, min_rounds in cases]
                out.append((name, form, res, ctx.profile()["em_k"]))
                comm.close()
            finally:
                ctx.close()
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_loop_control_on_two_ranks():
    """kamd_em_run_comm over two ranks on one GPU (collectives over gloo): the component-local form through kamd_em_local::run (G; H: one rank
    owns the oversized component and runs the hybrid on its rows), the streamed form through the rewind / replay of em_run_impl.  Every rank
    returns the oracle's result, and both the same bits."""
    import torch.multiprocessing as mp
    from tests.test_gpu_multirank import _free_port
    runs = tuple((name, form, _cases(name, False)) for name, form in RUNS)
    for name, _, cases in runs:                      # (the oracle before any device run; cached for the assertions below)
        for n_iter, min_rounds in cases:
            _oracle(name, n_iter, min_rounds)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_loop_worker, args=(r, 2, port, runs, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=600) for _ in range(2)]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    res = dict(got)
    for i, (name, form, cases) in enumerate(runs):
        cnt = _matrix(name)[2]
        for r in (0, 1):
            assert res[r][i][:2] == (name, form)
            em_k = res[r][i][3]
            assert (em_k == -2) if form == "local" else (em_k >= 0), f"{name} {form}, rank {r}: another form ran (em_k {em_k})"
            for (n_iter, min_rounds), one in zip(cases, res[r][i][2]):
                check_loop_case(one, _oracle(name, n_iter, min_rounds), cnt, n_iter, min_rounds, f"two ranks, {name} {form}, rank {r}")
        for (n_iter, min_rounds), a, b in zip(cases, res[0][i][2], res[1][i][2]):
            assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), \
                f"two ranks, {name} {form} (n_iter={n_iter}, min_rounds={min_rounds}): the ranks' results differ"
