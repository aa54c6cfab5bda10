"""The inputs of tests/test_gpu_em_group_load.py have the properties those tests are there for -- checked on the CPU, on the plan the
device's set-up steps build (kamd_em_local.h build_plan_steps_host + kamd_em_sell.h from_csr_plan through tests/emu_sell), for every
split length and both ways the groups are cut (one size class; components of up to 40 entries one wavefront each).

A group with a single TRANSCRIPT cannot exist: a group holds whole connected components of the rows with two or more transcripts
(singleton rows are the constant `single`, not rows of the plan), so every component, and with it every non-empty group, has at least
one row and two transcripts.  The smallest group is one row with two transcripts, and the matrix has one."""
import numpy as np
import pytest

from tests import em_group_load_inputs as I


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("split", [8, 16, 32])
def test_plan_of_the_group_load_matrix(split, small):
    s, n_small = I.plan_stats(split, small)
    ng = len(s["rows"])
    assert ng > 24 and (n_small > 24) == small                      # dozens of groups, every one with bases of its own
    live = s["rows"] > 0
    # no group with a single transcript (see above); groups without any component exist (a component longer than a group's window of
    # the running entry count leaves the next window empty): the kernel must take a group of empty tables
    assert np.all(s["tr"][live] >= 2) and np.all((s["tr"] == 0) == ~live)
    assert small == bool(np.any(~live))
    # the smallest group there is: one row of two transcripts, alone in its group -- as a workgroup's group and as a wavefront's
    tiny = np.nonzero((s["rows"] == 1) & (s["tr"] == 2))[0]
    assert len(tiny) == 1 and (tiny[0] < n_small) == small
    assert s["row_slices"][tiny[0]] == 1 and s["col_slices"][tiny[0]] == 1 and s["row_u16"][tiny[0]] == 256
    # one class: one long row alone in its group, split over the lanes of a slice (with two classes it shares a group with the hub)
    if not small:
        assert np.any((s["rows"] == 1) & (s["tr"] == I.FILLER) & (s["row_meta_slices"] == 1))
    # every stream is whole 16-byte words (a slice is a multiple of 128 entries): no head, no tail, none shorter than eight indices
    assert np.all(s["row_u16"] % 128 == 0) and np.all(s["col_u16"] % 128 == 0) and np.all(s["row_u16"][live] >= 128)
    # padding entries in both streams of every group
    assert np.all(s["row_pads"][live] > 0) and np.all(s["col_pads"][live] > 0)
    # lane metadata in both directions, and in a row stream segment ids ABOVE the group's number of transcripts: a packed minimum against
    # the zero slot's index (instead of the equality test on 0xFFFF) would change them
    assert np.any(s["col_meta_slices"] > 0)
    assert np.any((s["row_meta_slices"] > 0) & (s["row_meta_max_seg"] > s["tr"]))
    # batches: at 256 lanes the largest table needs more than the two trips a first batch holds (ems_stage_rest runs in every form), at
    # 1 024 lanes more than the one trip of the forms held to 64 registers
    longest = max(int(np.max(s[k])) for k in ("rows", "tr")) if not small else 0
    words = max(int(s["row_u16"].max()), int(s["col_u16"].max())) // 8
    assert max(words, longest) > 2 * 256 and max(words, longest) > 1024
    # ... and at split length 32 a wavefront's group (64 lanes, two trips a batch) more than one batch: an unsplit row of 30 entries is a
    # slice of 32 trips (at the shorter split lengths every group of the small class fits its first batch)
    if small and split == 32:
        assert int(s["row_u16"][:n_small].max()) // 8 > 2 * 64
