"""k_em_sell / k_em_sell_wave fetch a group's tables (index streams, slice descriptors, counts, singles, effective lengths, alpha, a) with
one batch of wide loads at the start of a launch.  The rounds must not notice: the same number of rounds and the same abundances as the
oracle's EMAlgorithm::run, and -- at split length 8, where the register form and the LDS form add in the same order -- the same bits
whether the slices of a wavefront live in registers or in LDS.

The inputs (tests/em_group_load_inputs.py) are held to what they are chosen for by tests/test_em_group_load_inputs.py, on the CPU, on the
plan the device's set-up steps build; here the device's plan must have the number of groups that check saw:
  * nine hundred gene-sized components cut into some forty groups (em_group_div=64: a group takes about 1 024 entries), so that every
    group has other bases in every table; with em_small_nnz=40 also 160 groups of about 40 entries, one wavefront each;
  * dense components (12 / 34 transcripts, ~200 distinct rows, one row with all transcripts): far more rows than transcripts and, at every
    split length, a split row, so the first row slice carries lane metadata whose segment ids exceed the number of transcripts -- the load
    must turn only the padding entries (0xFFFF) into the zero slot and leave such halves alone;
  * a hub transcript that sits in 300 two-transcript rows: a column split over many lanes (metadata and padding in the column stream);
  * a group of ONE row and two transcripts -- the smallest tables a group can have: a group holds whole components of rows with two or
    more transcripts, so a group with a single transcript cannot exist -- once as a workgroup's group, once as a wavefront's; one long row
    alone in a group; with two size classes, groups without any component (empty tables);
  * workgroups of 256 / 512 / 1024 lanes: one, two or more batches per table.
By the layout (kamd_em_sell.h) a slice occupies a multiple of 128 stream entries, so every group's stream starts and ends on a 16-byte
boundary of its array: there is no stream shorter than eight indices and no unaligned head or tail to exercise."""
import functools

import numpy as np
import pytest

from tests import common, em_group_load_inputs as I

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    kallisto_amd.load_library()
    return kallisto_amd


@functools.lru_cache(maxsize=None)
def _matrix():
    from oracle import oracle as O
    off, ids, cnt, eff, T = I.matrix()
    return off, ids, cnt, eff, T, O.em_run(off, ids, cnt, eff, T)


def _run(ka, **tune):
    import torch
    off, ids, cnt, eff, T, _ = _matrix()
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
    ctx = ka.Context(0)
    try:
        ctx.tune(em_form="local", em_group_div=64, **tune)
        out = ctx.em_run(eff, csr=(d(off, np.int64), d(ids, np.int32), d(cnt, np.int32)))
        prof = ctx.profile()
    finally:
        ctx.close()
    assert prof["em_k"] in (-1, -2)                               # the component-local form ...
    # ... on the groups whose tables tests/test_em_group_load_inputs.py looked at
    assert prof["em_grid"] == len(I.plan_stats(tune["em_split_len"], "em_small_nnz" in tune)[0]["rows"])
    return out


def _check_against_oracle(out):
    off, ids, cnt, eff, T, (alpha_o, abz_o, rounds_o) = _matrix()
    alpha, abz, rounds = out
    assert rounds == rounds_o
    assert abs(alpha.sum() - cnt.sum()) < 1e-6 * cnt.sum()
    common.assert_abundance_close(alpha, alpha_o, "alpha", rel=1e-9)
    tiny = lambda x: np.where(np.abs(x) < 1e-200, 0.0, x)      # (as test_em_forms_agree_with_oracle: where a value underflows depends on the order of the sums)
    common.assert_abundance_close(tiny(abz), tiny(abz_o), "alpha_before_zeroes", rel=1e-9, floor=1e-12)


@pytest.mark.parametrize("split", [8, 16, 32])
@pytest.mark.parametrize("block", [256, 512, 1024])
def test_group_tables_loaded_wide_agree_with_oracle(block, split, ka):
    _check_against_oracle(_run(ka, em_local_block=block, em_split_len=split))


@pytest.mark.parametrize("split", [8, 16, 32])
def test_wavefront_form_agrees_with_oracle(split, ka):
    """components of up to 40 entries one wavefront each (k_em_sell_wave), the others in workgroups, side by side"""
    _check_against_oracle(_run(ka, em_local_block=1024, em_split_len=split, em_small_nnz=40))


@pytest.mark.parametrize("block", [256, 512, 1024])
def test_register_and_lds_forms_give_the_same_bits_at_split_length_8(block, ka):
    a_r, z_r, r_r = _run(ka, em_local_block=block, em_split_len=8, em_reg_slices=True)
    a_l, z_l, r_l = _run(ka, em_local_block=block, em_split_len=8, em_reg_slices=False)
    assert r_r == r_l
    assert np.array_equal(a_r.view(np.uint64), a_l.view(np.uint64))
    assert np.array_equal(z_r.view(np.uint64), z_l.view(np.uint64))
