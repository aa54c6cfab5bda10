"""What the tests of the BUS records' sort, collapse and count (kamd_bus_sort, kamd_bus_count, `bus_sc --count`) share:

  * the ctypes binding of tests/emu_bussort/libkamd_bussort_emu.so (TEST INFRASTRUCTURE: kamd_bussort.h compiled for the CPU);
  * numpy's answer for sort and collapse (np.lexsort, run-length sums);
  * a restatement of `bustools count` over Python dicts (py_count, py_resolve, py_matrix): no sorting, no adjacency -- the yardstick of the count."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REC = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
ENTRY = np.dtype([("row", "<u4"), ("ec", "<i4"), ("value", "<u4")])
assert REC.itemsize == 32 and ENTRY.itemsize == 12
KEY_DIGITS = 24   # 8 + 8 + 4 + 4 key bytes
UMIS, READS = 0, 1


class CountStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_barcodes", C.c_uint64), ("n_entries", C.c_uint64), ("n_umis", C.c_uint64), ("n_multi_groups", C.c_uint64),
                ("n_multi_records", C.c_uint64), ("last_ms", C.c_float)]


_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_bussort")], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(HERE, "emu_bussort", "libkamd_bussort_emu.so"))
        L.bussort_emu_digit.restype = C.c_uint32
        L.bussort_emu_digit.argtypes = [C.c_void_p, C.c_int]
        L.bussort_emu_plan.restype = C.c_uint32
        L.bussort_emu_plan.argtypes = [C.c_void_p, C.c_void_p]
        L.bussort_emu_reduce.restype = C.c_uint32
        L.bussort_emu_reduce.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.bussort_emu_sort.restype = C.c_uint32
        L.bussort_emu_sort.argtypes = [C.c_void_p, C.c_uint64]
        L.bussort_emu_collapse.restype = C.c_uint64
        L.bussort_emu_collapse.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.bussort_emu_unsorted.restype = C.c_uint64
        L.bussort_emu_unsorted.argtypes = [C.c_void_p, C.c_uint64]
        L.bussort_emu_count.restype = C.c_uint64
        L.bussort_emu_count.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CountStats)]
        _lib = L
    return _lib


def emu_plan(rec):
    """bus_sort_plan of the OR / AND of the records' keys -> bit mask of the digits that need a pass"""
    rec = np.ascontiguousarray(rec, REC)
    o, a = np.zeros(KEY_DIGITS, np.uint8), np.zeros(KEY_DIGITS, np.uint8)
    return int(emu().bussort_emu_reduce(rec.ctypes.data, len(rec), o.ctypes.data, a.ctypes.data))


def emu_sort(rec):
    """-> (sorted copy, plan)"""
    out = np.ascontiguousarray(rec, REC).copy()
    plan = int(emu().bussort_emu_sort(out.ctypes.data, len(out)))
    return out, plan


def emu_collapse(rec):
    """records in key order -> (collapsed copy, runs whose sum exceeds 32 bits)"""
    out = np.ascontiguousarray(rec, REC).copy()
    over = C.c_uint64(0)
    n = int(emu().bussort_emu_collapse(out.ctypes.data, len(out), C.byref(over)))
    return out[:n], int(over.value)


def emu_count(rec, mode):
    """records in key order -> (barcodes, entries ENTRY, multi REC, stats dict, sums above 32 bits)"""
    rec = np.ascontiguousarray(rec, REC)
    n = max(len(rec), 1)
    bc, en, mu, st = np.zeros(n, np.uint64), np.zeros(n, ENTRY), np.zeros(n, REC), CountStats()
    over = int(emu().bussort_emu_count(rec.ctypes.data, len(rec), mode, bc.ctypes.data, en.ctypes.data, mu.ctypes.data, C.byref(st)))
    stats = {k: int(getattr(st, k)) for k, _ in CountStats._fields_ if k != "last_ms"}
    return bc[:stats["n_barcodes"]], en[:stats["n_entries"]], mu[:stats["n_multi_records"]], stats, over


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# numpy: sort and collapse
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def np_sort(rec):
    """the driver's order: np.lexsort((flags, ec, umi, barcode)), stable"""
    return rec[np.lexsort((rec["flags"], rec["ec"], rec["umi"], rec["barcode"]))]


def np_collapse(rec):
    """records in key order -> (one record per run of equal keys: count = the run's sum, everything else of the first; the sums as uint64)"""
    if len(rec) == 0:
        return rec.copy(), np.zeros(0, np.uint64)
    first = np.ones(len(rec), bool)
    first[1:] = (rec["barcode"][1:] != rec["barcode"][:-1]) | (rec["umi"][1:] != rec["umi"][:-1]) | (rec["ec"][1:] != rec["ec"][:-1]) | (rec["flags"][1:] != rec["flags"][:-1])
    starts = np.flatnonzero(first)
    sums = np.add.reduceat(rec["count"].astype(np.uint64), starts)
    out = rec[starts].copy()
    out["count"] = (sums & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out, sums


def np_key_bytes(rec):
    """[n, 24] uint8: the key bytes, digit 0 = low byte of flags .. digit 23 = high byte of barcode; ec with its top bit flipped"""
    key = np.zeros((len(rec), KEY_DIGITS), np.uint8)
    key[:, 0:4] = rec["flags"].astype("<u4").view(np.uint8).reshape(-1, 4)
    key[:, 4:8] = (rec["ec"].astype("<i4").view("<u4") ^ np.uint32(0x80000000)).view(np.uint8).reshape(-1, 4)
    key[:, 8:16] = rec["umi"].astype("<u8").view(np.uint8).reshape(-1, 8)
    key[:, 16:24] = rec["barcode"].astype("<u8").view(np.uint8).reshape(-1, 8)
    return key


def np_plan(rec):
    """the digits in which two keys differ, from the key bytes themselves"""
    if len(rec) == 0:
        return 0
    key = np_key_bytes(rec)
    diff = np.bitwise_or.reduce(key, axis=0) != np.bitwise_and.reduce(key, axis=0)
    return int(sum(1 << d for d in range(KEY_DIGITS) if diff[d]))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# `bustools count`, restated over dicts
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def py_count(recs, mode):
    """recs: iterable of (barcode, umi, class, count), any order; a class is anything hashable.
    -> dict(barcodes = the rows, ascending; entries = {(row, class): value}; multi = {(barcode, umi): set of classes} of the groups that name several
    classes (UMIS mode: they add nothing to entries); n_umis = distinct (barcode, umi))"""
    recs = list(recs)
    barcodes = sorted({r[0] for r in recs})
    row = {b: i for i, b in enumerate(barcodes)}
    entries, multi, groups = {}, {}, {}
    for b, u, c, n in recs:
        groups.setdefault((b, u), set()).add(c)
        if mode == READS:
            entries[(row[b], c)] = entries.get((row[b], c), 0) + n
    if mode == UMIS:
        for (b, u), cs in groups.items():
            if len(cs) == 1:
                k = (row[b], next(iter(cs)))
                entries[k] = entries.get(k, 0) + 1
            else:
                multi[(b, u)] = cs
    return {"barcodes": barcodes, "entries": entries, "multi": multi, "n_umis": len(groups)}


def py_resolve(multi, set_of):
    """the multi-class groups of py_count, set_of(class) -> transcript ids: the intersection of a group's sets -> ({(barcode, umi): sorted tuple}, the
    groups with an empty intersection (dropped))"""
    kept, dropped = {}, []
    for g, cs in multi.items():
        inter = None
        for c in cs:
            s = set(set_of(c))
            inter = s if inter is None else inter & s
        if inter:
            kept[g] = tuple(sorted(inter))
        else:
            dropped.append(g)
    return kept, dropped


def py_matrix(recs, mode, set_of):
    """the whole count with its host resolution -> ({(barcode, transcript set as sorted tuple): value}, n multi groups, n dropped groups)"""
    c = py_count(recs, mode)
    m = {}
    for (r, cls), v in c["entries"].items():
        k = (c["barcodes"][r], tuple(sorted(set_of(cls))))
        m[k] = m.get(k, 0) + v
    kept, dropped = py_resolve(c["multi"], set_of)
    for (b, u), s in kept.items():
        m[(b, s)] = m.get((b, s), 0) + 1
    return m, len(c["multi"]), len(dropped)


def assert_count_is_the_restatement(rec_sorted, mode, barcodes, entries, multi, stats):
    """what a count (the CPU build's or the device's) made of records in key order, against py_count of the same records: the rows, every entry, the
    entries' order, the statistics, and the multi records -- exactly the multi-class groups' records, in input order, pad = their row.  -> py_count's dict"""
    want = py_count(rec_tuples(rec_sorted), mode)
    assert np.asarray(barcodes).astype(np.uint64).tolist() == want["barcodes"]
    keys = list(zip(entries["row"].tolist(), entries["ec"].tolist()))
    assert dict(zip(keys, entries["value"].tolist())) == want["entries"]
    assert all(a < b for a, b in zip(keys, keys[1:]))                 # strictly increasing in (row, class)
    assert stats["n_records"] == len(rec_sorted) and stats["n_umis"] == want["n_umis"] and stats["n_barcodes"] == len(want["barcodes"])
    assert stats["n_entries"] == len(want["entries"]) and stats["n_multi_groups"] == len(want["multi"])
    in_multi = np.array([g in want["multi"] for g in zip(rec_sorted["barcode"].tolist(), rec_sorted["umi"].tolist())], bool)
    exp = np.ascontiguousarray(rec_sorted[in_multi]).copy()
    exp["pad"] = np.searchsorted(np.array(want["barcodes"], np.uint64), exp["barcode"])
    assert stats["n_multi_records"] == len(exp)
    assert np.ascontiguousarray(multi).tobytes() == exp.tobytes()
    return want


def rec_tuples(rec):
    """REC array -> the (barcode, umi, ec, count) tuples py_count takes"""
    return list(zip(rec["barcode"].tolist(), rec["umi"].tolist(), rec["ec"].tolist(), rec["count"].tolist()))


def make_records(barcode, umi, ec, flags=0, count=1, pad=0):
    barcode = np.asarray(barcode, np.uint64)
    r = np.zeros(len(barcode), REC)
    r["barcode"], r["umi"], r["ec"], r["flags"], r["count"], r["pad"] = barcode, umi, ec, flags, count, pad
    return r
