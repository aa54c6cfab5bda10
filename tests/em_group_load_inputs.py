"""The EC matrix of tests/test_gpu_em_group_load.py and the shape of the plan the device builds from it, computed on the CPU
(tests/emu_sell: the steps of kamd_em_local.h and the layout of kamd_em_sell.h).  tests/test_em_group_load_inputs.py holds the matrix to
the properties the GPU tests rely on."""
import ctypes as C
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_WORDS = 12
COLS = ("rows", "tr", "nnz", "row_slices", "col_slices", "row_u16", "col_u16", "row_pads", "col_pads", "row_meta_slices", "row_meta_max_seg",
        "col_meta_slices")
# what the device's plan search uses for this matrix (em_sell_plan_search): groups of max(1024, nnz / (CUs * em_group_div)) entries, and with
# em_small_nnz = 40 components of up to 40 entries in groups of about 40
TARGET, SMALL = 1024, 40
# The one-row components have the highest transcript ids, so they are the last components of their class, and a group holds the components
# whose first entry falls into its window of the class's running entry count.  FILLER (the length of one long row in front of them) and
# ONE_ROW (how many there are) put the LAST of them at the start of a window, with one size class and with two: it is a group of its own.
FILLER, ONE_ROW = 1855, 17


@functools.lru_cache(maxsize=None)
def matrix(filler=None, one_row=None):
    from tests.test_em_local import _gene_matrix
    filler = FILLER if filler is None else filler
    one_row = ONE_ROW if one_row is None else one_row
    off, ids, cnt, eff, T = _gene_matrix(900, 23)
    rng = np.random.default_rng(5)
    rows, counts = [], []
    t = T
    for n in (12, 34, 12):                                # dense components: n transcripts, ~200 rows of 2 .. 8, one row with all of them
        seen = {tuple(range(n))}
        while len(seen) < 200:
            seen.add(tuple(sorted(rng.choice(n, int(rng.integers(2, 9)), replace=False).tolist())))
        for r in sorted(seen):
            rows.append(np.array(r) + t); counts.append(int(rng.integers(0, 30)))
        t += n
    hub = t                                               # hub: one transcript in 300 rows of two
    for i in range(300):
        rows.append(np.array([hub, hub + 1 + i])); counts.append(int(rng.integers(1, 9)))
    t += 301
    rows.append(np.arange(t, t + filler)); counts.append(7)   # one long row (a component of its own)
    t += filler
    rows.append(np.arange(t, t + 30)); counts.append(11)      # a row of 30: a small component whose slice is 32 trips wide at split length 32
    t += 30
    for i in range(one_row):                              # one row, two transcripts
        rows.append(np.array([t, t + 1])); counts.append(3 + 5 * i)
        t += 2
    for s in rng.choice(t - T, 40, replace=False):        # singleton rows: the constant term of some of the new transcripts
        rows.append(np.array([T + int(s)])); counts.append(int(rng.integers(1, 20)))
    order = rng.permutation(len(rows))
    ids2 = np.concatenate([ids] + [rows[i].astype(np.uint32) for i in order])
    off2 = np.concatenate([off, off[-1] + np.cumsum([len(rows[i]) for i in order]).astype(np.uint64)])
    cnt2 = np.concatenate([cnt, np.array([counts[i] for i in order], np.uint32)])
    eff2 = np.concatenate([eff, rng.uniform(150, 3000, t - T)])
    return off2, ids2, cnt2, eff2, t


def plan_stats(split, small, filler=None, one_row=None):
    """-> (one dict of arrays over the groups, number of groups of the small class)"""
    lib = C.CDLL(os.path.join(ROOT, "tests", "emu_sell", "libkamd_sell_emu.so"))
    off, ids, cnt, eff, T = matrix(filler, one_row)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    off = np.ascontiguousarray(off, np.uint64); ids = np.ascontiguousarray(ids, np.uint32); cnt = np.ascontiguousarray(cnt, np.uint32)
    stats = np.zeros((4096, STAT_WORDS), np.uint32)
    n_small = C.c_uint32(0)
    ng = lib.emu_sell_plan_stats(p(off), p(ids), p(cnt), C.c_uint64(len(cnt)), p(np.ascontiguousarray(eff)), C.c_uint64(T), C.c_uint64(1 << 30),
                                 C.c_uint64(TARGET), C.c_uint32(SMALL if small else 0), C.c_uint64(SMALL), C.c_uint32(split), p(stats), 4096,
                                 C.byref(n_small))
    assert ng > 0, ng
    return {k: stats[:ng, i].astype(np.int64) for i, k in enumerate(COLS)}, n_small.value
