"""Per-read equivalence classes without a GPU: the table and the look-up of kamd_readec.h (CPU build, tests/emu_readec) against a Python dict of
tuples; the reference's `bus -n` output (tests/golden/bus_num) against the oracle read by read; the option checks of `bus -n`."""
import collections
import os
import subprocess

import numpy as np
import pytest

from tests import read_ecs_common as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
IDX = os.path.join(ROOT, "tests", "golden", "ref_test_pe", "index.idx")


def _distinct_sets(n, seed, max_len=300, universe=5000):
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < n:
        k = int(rng.integers(1, max_len + 1))
        s = tuple(sorted(rng.choice(universe, size=k, replace=False).tolist()))
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def _check(sets, queries, cap=None, tag_mask=2 ** 64 - 1):
    slots, cap, failed = R.emu_table(sets, cap, tag_mask)
    assert failed == 0
    assert cap & (cap - 1) == 0 and cap >= 2 * len(sets)
    # every row sits in exactly one slot, every other slot is empty
    rows = slots[1::2][slots[0::2] != 0]
    assert sorted(rows.tolist()) == list(range(len(sets)))
    want = {s: i for i, s in enumerate(sets)}
    got = R.emu_lookup(sets, slots, cap, queries, tag_mask)
    for q, g in zip(queries, got.tolist()):
        assert g == (R.NONE if len(q) == 0 else want.get(tuple(q), R.FOREIGN)), (q, g)


@pytest.mark.parametrize("n", [1, 2, 1000, 5000])
def test_table_against_a_dict(n):
    sets = _distinct_sets(n, seed=n)
    absent = [s for s in _distinct_sets(50, seed=n + 1) if s not in set(sets)]
    assert absent
    # the minimum capacity is the library's own: the smallest power of two >= 2 n (probe sequences that start in the last slots wrap)
    assert R.emu().rec_emu_capacity(n) == max(2, 1 << (2 * n - 1).bit_length())
    _check(sets, sets + absent + [()])


@pytest.mark.parametrize("n", [2, 1000])
def test_degenerate_hash_every_tag_equal(n):
    """tag_mask = 0: all tags are 1 and all probes start in one slot -- the member compare and the continued probe decide alone, and the probes of
    the last rows walk n slots"""
    sets = _distinct_sets(n, seed=7 * n, max_len=40)
    absent = [s for s in _distinct_sets(20, seed=7 * n + 1, max_len=40) if s not in set(sets)]
    _check(sets, sets + absent + [()], tag_mask=0)


def test_full_table_wraps_and_ends():
    """a capacity below the library's minimum, exactly the number of rows, with every tag equal: the table is full, every probe wraps around its end, and
    a probe for an absent set ends after one round (no empty slot stops it)"""
    sets = _distinct_sets(64, seed=3, max_len=20)
    slots, cap, failed = R.emu_table(sets, cap=64, tag_mask=0)
    assert failed == 0 and np.all(slots[0::2] == 1)
    got = R.emu_lookup(sets, slots, cap, sets + [(1, 2, 3, 4999)], tag_mask=0)
    assert got.tolist() == list(range(64)) + [R.FOREIGN]
    # one row more than slots: the build reports it instead of spinning
    assert R.emu_table(sets + [(4998, 4999)], cap=64, tag_mask=0)[2] == 1


def test_strict_prefix_and_neighbours():
    sets = [(1, 2, 3), (1, 2), (1, 2, 3, 4), (2,), (1,), (0, 1, 2, 3)]
    queries = sets + [(1, 2, 3, 5), (3,), (1, 3), (), (2, 3)]
    _check(sets, queries)
    _check(sets, queries, tag_mask=0)


def test_empty_result():
    slots, cap, failed = R.emu_table([])
    assert cap == 2 and failed == 0 and not slots.any()
    assert R.emu_lookup([], slots, cap, [(1,), ()]).tolist() == [R.FOREIGN, R.NONE]


@pytest.mark.parametrize("case", R.BUS_CASES)
def test_golden_is_consistent_with_the_oracle(case):
    """every read of the case: the oracle's set is what the reference wrote under the read's number and barcode, and the reads without a line are exactly
    the ones the oracle leaves unmapped.  (A barcode shared by two lines of the batch file holds two reads per number: compared as multisets per key.)"""
    meta, lines = R.load_bus_case(case)
    assert meta["numbering"] == "entry" and meta["oracle_disagrees_on_reads"] == []
    assert len(lines) == meta["n_records"] and len({l[2] for l in lines}) == meta["n_classes"]
    sets = R.oracle_sets(meta["fixture"], R.opts_key(R.bus_oracle_opts(meta)))
    assert len(sets) == meta["n_reads"]
    want = collections.Counter(lines)
    got = collections.Counter()
    n_unmapped = 0
    for bc, a, b in R.samples_of(meta):
        for i in range(a, b):
            if sets[i]:
                got[(i - a, bc, sets[i])] += 1
            else:
                n_unmapped += 1
    assert n_unmapped == meta["n_reads_without_record"]
    assert got == want, sorted((got - want).items())[:5] + sorted((want - got).items())[:5]


def _bus_errors(args, cwd):
    p = subprocess.run([EXE, "bus", *args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, [l for l in p.stderr.decode().split("\n") if l.startswith("Error:")], p.stdout.decode()


def test_bus_num_refuses_aa(tmp_path):
    open(tmp_path / "a.fq", "w").close()
    rc, errs, _ = _bus_errors(["-x", "bulk", "-i", IDX, "-o", "o", "-n", "--aa", "a.fq"], str(tmp_path))
    assert rc == 1 and len(errs) == 1 and "--aa" in errs[0] and "--num" in errs[0]


def test_bus_num_refuses_a_fifo(tmp_path):
    os.mkfifo(tmp_path / "pipe.fq")
    rc, errs, _ = _bus_errors(["-x", "bulk", "-i", IDX, "-o", "o", "--num", "pipe.fq"], str(tmp_path))
    assert rc == 1 and len(errs) == 1 and "pipe.fq is not a regular file" in errs[0]


def test_bus_help_lists_num(tmp_path):
    rc, _, out = _bus_errors(["--help"], str(tmp_path))
    assert "-n, --num" in out
    p = subprocess.run([EXE, "bus"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and "-n, --num" in p.stdout.decode()
