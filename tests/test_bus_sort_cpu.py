"""The rules of kamd_bus_sort / kamd_bus_count without a GPU: kamd_bussort.h compiled for the CPU (tests/emu_bussort, TEST INFRASTRUCTURE) against
numpy's lexsort and run-length sums and against a dict restatement of `bustools count` (tests/bus_sort_common.py).  Integers only: every comparison
is exact."""
import numpy as np
import pytest

from tests import bus_sc_common as B
from tests import bus_sort_common as S

INT32_MIN = -2 ** 31
ALL_DIGITS = (1 << S.KEY_DIGITS) - 1


def _random_records(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, S.REC)
    r["barcode"] = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    r["umi"] = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    r["ec"] = rng.integers(INT32_MIN, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    r["flags"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    r["count"] = rng.integers(1, 100, n)
    return r


def _one_byte_pairs():
    """for each of the 24 key bytes a pair of records whose keys differ in that byte alone, the larger key first"""
    base = S.make_records([0x1122334455667788], 0x99AABBCCDDEEFF00, 0x12345678, 0x0A0B0C0D)[0]
    out = []
    for d in range(S.KEY_DIGITS):
        hi, lo = base.copy(), base.copy()
        field, shift = (("flags", d), ("ec", d - 4), ("umi", d - 8), ("barcode", d - 16))[(d >= 4) + (d >= 8) + (d >= 16)]
        for rec, bit in ((hi, 0x80), (lo, 0x00)):   # bit 7 of the byte set / cleared (in the top byte of ec that is the sign: set means negative, the SMALLER key)
            v = int(rec[field]) & 0xFFFFFFFFFFFFFFFF if field != "ec" else int(rec[field]) & 0xFFFFFFFF
            v = (v & ~(0xFF << (8 * shift))) | ((0x11 | bit) << (8 * shift))
            rec[field] = v - 2 ** 32 if field == "ec" and v >= 2 ** 31 else v
        out += [hi, lo]
    return np.array(out, S.REC)


def test_digits_are_the_key_bytes():
    r = _random_records(50, 1)
    key = S.np_key_bytes(r)
    assert key[0, 0] == int(r["flags"][0]) & 0xFF and key[0, 7] == ((int(r["ec"][0]) >> 24) & 0xFF) ^ 0x80 and key[0, 23] == int(r["barcode"][0]) >> 56
    lib = S.emu()
    for i in range(len(r)):
        one = np.ascontiguousarray(r[i:i + 1])
        assert [lib.bussort_emu_digit(one.ctypes.data, d) for d in range(S.KEY_DIGITS)] == key[i].tolist()


def test_lsd_sort_over_the_digits_is_numpys_lexsort():
    r = _random_records(5000, 2)
    r["ec"][:40] = np.tile(np.array([-1, INT32_MIN, 0, 1, 2 ** 31 - 1, -2, 7, 1000], np.int32), 5)   # the sign flip: negative classes sort before positive ones
    pairs = _one_byte_pairs()
    r = np.concatenate([r, pairs, r[:300]])   # (repeated keys: stability)
    r["pad"] = np.arange(len(r))
    got, plan = S.emu_sort(r)
    want = S.np_sort(r)
    assert got.tobytes() == want.tobytes()
    assert plan == ALL_DIGITS
    # each pair on its own: one pass, over exactly the byte that differs, and the two records change places
    for d in range(S.KEY_DIGITS):
        p = pairs[2 * d:2 * d + 2].copy()
        p["pad"] = [0, 1]
        got, plan = S.emu_sort(p)
        assert plan == 1 << d, d
        assert got.tobytes() == S.np_sort(p).tobytes()
        if d == 7:   # the byte with ec's sign: the record with the bit set is negative and stays first
            assert got["pad"].tolist() == [0, 1] and int(p["ec"][0]) < 0 <= int(p["ec"][1])
        else:
            assert got["pad"].tolist() == [1, 0], d


def test_sort_plan():
    same = S.make_records([5] * 100, 7, 3, 1)
    assert S.emu_plan(same) == 0 and S.np_plan(same) == 0
    low = same.copy()
    low["flags"][::2] ^= 1
    assert S.emu_plan(low) == 1 << 0
    top = same.copy()
    top["barcode"][::3] |= np.uint64(1 << 63)
    assert S.emu_plan(top) == 1 << 23
    rnd = _random_records(5000, 3)
    assert S.emu_plan(rnd) == ALL_DIGITS == S.np_plan(rnd)
    # the plan function itself: a digit counts when its OR byte differs from its AND byte
    o, a = np.zeros(S.KEY_DIGITS, np.uint8), np.zeros(S.KEY_DIGITS, np.uint8)
    o[[2, 9, 23]], a[[2, 9, 23]] = [0xFF, 0x10, 0x81], [0xFF, 0x00, 0x80]
    assert S.emu().bussort_emu_plan(o.ctypes.data, a.ctypes.data) == (1 << 9) | (1 << 23)
    tenx = _tenx_like(3000, 4)
    assert S.emu_plan(tenx) == S.np_plan(tenx)


def _tenx_like(n, seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 2 ** 32, 50, dtype=np.uint64)
    return S.make_records(pool[rng.integers(0, 50, n)], rng.integers(0, 2 ** 24, n, dtype=np.uint64), rng.integers(0, 1000, n).astype(np.int32),
                          np.array([0, 1, 5], np.uint32)[rng.integers(0, 3, n)], rng.integers(1, 4, n))


NO_UMI = 2 ** 64 - 1


def _corner_records():
    """(barcode, umi, ec, flags, count): every corner of the collapse and of the group rule; the first and the last group are multi-class"""
    rows = [
        (1, 5, 3, 0, 1), (1, 5, 9, 0, 2),                       # first group of all: two classes
        (1, 6, 4, 0, 1),                                         # a group of one record
        (1, 7, 4, 0, 1), (1, 7, 4, 1, 2), (1, 7, 4, 5, 1),       # one class, three flags: not multi, three records after the collapse
        (1, 8, 4, 0, 1), (1, 8, 4, 0, 5), (1, 8, 4, 0, 1),       # equal keys: collapse to count 7
        (2, 5, 1, 0, 1), (2, 5, 2, 0, 1), (2, 5, 7, 0, 1),       # three classes
        (2, NO_UMI, 4, 0, 3), (2, NO_UMI, 4, 0, 1),              # a UMI of ~0
        (3, 1, 2, 0, 1), (3, 1, 5, 1, 1),                        # a barcode whose only group is multi: it still has a row
        (4, 2, 4, 0, 1), (4, 3, 4, 0, 1), (4, 4, 6, 0, 1),       # (row, class 4) from two UMIs, not adjacent once class 6 lies between ... in another barcode too
        (1, 9, 6, 0, 1),
        (9, 9, -1, 0, 1), (9, 9, 0, 0, 1),                       # last group of all: two classes, one of them negative
    ]
    a = np.array(rows, dtype=object)
    return S.make_records(a[:, 0].astype(np.uint64), a[:, 1].astype(np.uint64), a[:, 2].astype(np.int32), a[:, 3].astype(np.uint32), a[:, 4].astype(np.uint32))


def _check_count(rec_sorted, mode):
    bc, en, mu, st, over = S.emu_count(rec_sorted, mode)
    assert over == 0
    return S.assert_count_is_the_restatement(rec_sorted, mode, bc, en, mu, st), st


@pytest.mark.parametrize("collapsed", [False, True])
def test_collapse_and_group_rule_equal_the_dict_restatement(collapsed):
    rec = _corner_records()
    rec["pad"] = np.arange(len(rec))
    rng = np.random.default_rng(5)
    srt, _ = S.emu_sort(rec[rng.permutation(len(rec))])
    assert srt[["barcode", "umi", "ec", "flags"]].tolist() == S.np_sort(rec)[["barcode", "umi", "ec", "flags"]].tolist()
    srt = S.np_sort(rec)
    col, over = S.emu_collapse(srt)
    want_col, sums = S.np_collapse(srt)
    assert over == 0 and col.tobytes() == want_col.tobytes()
    assert len(col) == len(rec) - 3                                    # only (1, 8, 4, 0) x 3 and (2, ~0, 4, 0) x 2 merge
    assert int(col[(col["barcode"] == 1) & (col["umi"] == 8)]["count"][0]) == 7
    data = col if collapsed else srt
    want, st = _check_count(data, S.UMIS)
    assert set(want["multi"]) == {(1, 5), (2, 5), (3, 1), (9, 9)}
    assert want["barcodes"] == [1, 2, 3, 4, 9] and not any(r == 2 for r, _ in want["entries"])   # barcode 3: a row, no entry
    assert want["entries"][(0, 4)] == 3 and want["entries"][(3, 4)] == 2                        # flags ignored for grouping; two UMIs, one (row, class)
    assert (int(data[0]["barcode"]), int(data[0]["umi"])) in want["multi"] and (int(data[-1]["barcode"]), int(data[-1]["umi"])) in want["multi"]
    want_r, st_r = _check_count(data, S.READS)
    assert st_r["n_multi_groups"] == 0 and sum(want_r["entries"].values()) == int(rec["count"].astype(np.int64).sum())
    assert S.emu().bussort_emu_unsorted(np.ascontiguousarray(data).ctypes.data, len(data)) == 0
    assert S.emu().bussort_emu_unsorted(np.ascontiguousarray(data[::-1]).ctypes.data, len(data)) == len(col) - 1   # (equal neighbours are in order)


def test_collapse_sum_is_held_in_64_bits():
    r = S.make_records([1, 1, 2, 2], 1, 1, 0, [0xFFFFFFFE, 1, 0xFFFFFFFF, 1])
    col, over = S.emu_collapse(r)
    assert over == 1 and len(col) == 2 and int(col[0]["count"]) == 0xFFFFFFFF
    _, sums = S.np_collapse(r)
    assert sums.tolist() == [0xFFFFFFFF, 0x100000000]


def test_count_on_random_groups_equals_the_dict_restatement():
    rec = _tenx_like(4000, 6)
    rec["umi"] &= np.uint64(0x3F)     # 50 barcodes x 64 UMIs: groups of several records, many of them multi-class
    rec["ec"] %= 7
    srt = S.np_sort(rec)
    for data in (srt, S.np_collapse(srt)[0]):
        for mode in (S.UMIS, S.READS):
            want, st = _check_count(data, mode)
        assert len(S.py_count(S.rec_tuples(data), S.UMIS)["multi"]) > 100


def test_goldens_hold_the_corners_of_the_count():
    """the reference's own records (tests/golden/bus_sc), classes as transcript sets: at least one case has a multi-class group, and at least one has
    a multi-class group whose transcript sets do not intersect (the group `bustools count` drops)"""
    n_multi, n_empty = {}, {}
    for name in B.golden_cases():
        _, lines = B.load_golden(name)
        recs = [(bc, umi, s, 1) for _, bc, umi, s in lines]
        m, n_multi[name], n_empty[name] = S.py_matrix(recs, S.UMIS, lambda s: s)
        c = S.py_count(recs, S.UMIS)
        # every group lands in the matrix once, but for the dropped ones
        assert sum(m.values()) == c["n_umis"] - n_empty[name]
        assert {b for b, _ in m} <= set(c["barcodes"])
    assert max(n_multi.values()) >= 1, n_multi
    assert max(n_empty.values()) >= 1, n_empty
