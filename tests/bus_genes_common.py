"""What the tests of the gene-level count of BUS records (kamd_bus_genes_create, kamd_bus_count_genes, `bus_sc --genecounts`) share:

  * a restatement of the gene lists and of `bustools count --genecounts` over Python dicts and sets (py_gene_lists, py_gene_count): no sorting of
    records, no adjacency -- the yardstick;
  * the ctypes binding of tests/emu_busgenes/libkamd_busgenes_emu.so (TEST INFRASTRUCTURE: kamd_busgenes.h compiled for the CPU);
  * the class grid, the gene maps of the golden cases and the outcome of every group of a set of records."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests.bus_sort_common import ENTRY, REC, READS, UMIS, make_records, np_sort, rec_tuples  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
NONE, MULTI = -1, -2
OUTCOMES = ("single_one", "single_none", "single_multi", "multi_one", "multi_none", "multi_multi")   # classes of the group x genes left


class GeneCountStats(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_barcodes", C.c_uint64), ("n_entries", C.c_uint64), ("n_umis", C.c_uint64), ("n_counted", C.c_uint64),
                ("n_no_gene", C.c_uint64), ("n_multi_gene", C.c_uint64), ("n_wave_groups", C.c_uint64), ("last_ms", C.c_float), ("resolve_ms", C.c_float)]


COUNTERS = ("n_records", "n_barcodes", "n_entries", "n_umis", "n_counted", "n_no_gene", "n_multi_gene")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def py_gene_lists(tr_gene, sets):
    """tr_gene: gene id per transcript, -1 = none; sets: a sequence of transcript-id sequences -> the sorted distinct gene ids (>= 0) of every set"""
    return [sorted({int(tr_gene[t]) for t in s} - {-1}) for s in sets]


def py_group_gene(lists, classes):
    """the gene of a group that names `classes` (any iterable): the one gene all their lists share, else NONE / MULTI"""
    inter = None
    for c in classes:
        g = set(lists[c])
        inter = g if inter is None else inter & g
    return next(iter(inter)) if len(inter) == 1 else (NONE if not inter else MULTI)


def py_gene_count(recs, mode, lists):
    """recs: iterable of (barcode, umi, class, count), any order; lists: py_gene_lists' result
    -> dict(barcodes = the rows, ascending; entries = {(row, gene): value}; n_umis, n_counted, n_no_gene, n_multi_gene; groups = {key: gene / NONE /
    MULTI} with key = (barcode, umi) in UMIS mode)"""
    recs = list(recs)
    barcodes = sorted({r[0] for r in recs})
    row = {b: i for i, b in enumerate(barcodes)}
    entries, genes = {}, {}
    if mode == READS:
        for i, (b, u, c, n) in enumerate(recs):
            g = genes[i] = py_group_gene(lists, [c])
            if g >= 0:
                entries[(row[b], g)] = entries.get((row[b], g), 0) + n
    else:
        groups = {}
        for b, u, c, n in recs:
            groups.setdefault((b, u), set()).add(c)
        for (b, u), cs in groups.items():
            g = genes[(b, u)] = py_group_gene(lists, cs)
            if g >= 0:
                entries[(row[b], g)] = entries.get((row[b], g), 0) + 1
    vals = list(genes.values())
    return {"barcodes": barcodes, "entries": entries, "n_umis": len(vals), "n_counted": sum(1 for g in vals if g >= 0), "n_no_gene": vals.count(NONE),
            "n_multi_gene": vals.count(MULTI), "groups": genes}


def py_wave_groups(recs, lists, max_records, max_list):
    """the (barcode, umi) groups of recs that the thresholds hand to a wavefront: more than one record, and more than max_records records or a smallest
    list of more than max_list genes.  recs: (barcode, umi, class, count) as the device gets them (duplicates count as records)"""
    groups = {}
    for b, u, c, n in recs:
        groups.setdefault((b, u), []).append(c)
    return sum(1 for cs in groups.values() if len(cs) > 1 and (len(cs) > max_records or min(len(lists[c]) for c in cs) > max_list))


def py_outcomes(recs, lists):
    """UMIS mode: how many groups of recs end in each of OUTCOMES"""
    groups = {}
    for b, u, c, n in recs:
        groups.setdefault((b, u), set()).add(c)
    out = dict.fromkeys(OUTCOMES, 0)
    for cs in groups.values():
        g = py_group_gene(lists, cs)
        out[("single_" if len(cs) == 1 else "multi_") + ("one" if g >= 0 else ("none" if g == NONE else "multi"))] += 1
    return out


def assert_gene_count_is_the_restatement(rec_sorted, mode, lists, barcodes, entries, stats):
    """what a gene count (the CPU build's or the device's) made of records in key order, against py_gene_count of the same records: the rows, every
    entry, the entries' strict (row, gene) order, every counter.  -> py_gene_count's dict"""
    want = py_gene_count(rec_tuples(rec_sorted), mode, lists)
    assert np.asarray(barcodes).astype(np.uint64).tolist() == want["barcodes"]
    keys = list(zip(entries["row"].tolist(), entries["ec"].tolist()))
    assert dict(zip(keys, entries["value"].tolist())) == want["entries"]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    assert stats["n_records"] == len(rec_sorted) and stats["n_barcodes"] == len(want["barcodes"]) and stats["n_entries"] == len(want["entries"])
    for k in ("n_umis", "n_counted", "n_no_gene", "n_multi_gene"):
        assert stats[k] == want[k], k
    return want


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the class grid of the list tests, the gene maps of the golden cases
# ---------------------------------------------------------------------------------------------------------------------------------------------------
GRID_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 5000)
GRID_TARGETS = 6000
GRID_MAPS = ("zero", "identity", "mod7", "none", "zero_holes", "identity_holes", "mod7_holes")


def grid_sets():
    """classes of GRID_SIZES transcripts each, twice: a run of consecutive ids, and ids spread over the targets; and an empty class between them"""
    sets = []
    for k, n in enumerate(GRID_SIZES):
        sets.append(list(range(k, k + n)))
    sets.append([])
    for k, n in enumerate(GRID_SIZES):
        step = max(GRID_TARGETS // n - 1, 1)
        sets.append([(7 * k + j * step) % GRID_TARGETS for j in range(n)] if step > 1 else list(range(GRID_TARGETS - n, GRID_TARGETS)))
    return [sorted(set(s)) for s in sets]


def grid_map(name):
    """-> (tr_gene int32 [GRID_TARGETS], n_genes)"""
    t = np.arange(GRID_TARGETS, dtype=np.int64)
    base = name.split("_")[0]
    g = {"zero": np.zeros_like(t), "identity": t, "mod7": t % 7, "none": np.full_like(t, -1)}[base]
    if name.endswith("_holes"):
        g = np.where(t % 7 == 3, -1, g)
    return g.astype(np.int32), {"zero": 1, "identity": GRID_TARGETS, "mod7": 7, "none": 1}[base]


def golden_map(n_targets, holes):
    """gene(t) = t // 3, with holes: -1 where t % 7 == 3 -> (tr_gene int32, n_genes)"""
    t = np.arange(n_targets, dtype=np.int64)
    g = t // 3
    if holes:
        g = np.where(t % 7 == 3, -1, g)
    return g.astype(np.int32), (n_targets + 2) // 3


def csr_of(sets):
    off = np.zeros(len(sets) + 1, np.uint64)
    if len(sets):
        off[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
    ids = np.array([t for s in sets for t in s], np.uint32)
    return off, ids


def lists_of_csr(off, ids):
    return [ids[int(off[c]):int(off[c + 1])].tolist() for c in range(len(off) - 1)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# emu binding
# ---------------------------------------------------------------------------------------------------------------------------------------------------
_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_busgenes")], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(HERE, "emu_busgenes", "libkamd_busgenes_emu.so"))
        L.busgenes_emu_thresholds.restype = None
        L.busgenes_emu_thresholds.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.busgenes_emu_lists.restype = C.c_uint64
        L.busgenes_emu_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
        L.busgenes_emu_group.restype = C.c_int32
        L.busgenes_emu_group.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        L.busgenes_emu_count.restype = C.c_int
        L.busgenes_emu_count.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(GeneCountStats)]
        _lib = L
    return _lib


def thresholds():
    """-> (GENES_THREAD_MAX_RECORDS, GENES_THREAD_MAX_LIST) of kamd_busgenes.h"""
    a, b = C.c_uint32(0), C.c_uint32(0)
    emu().busgenes_emu_thresholds(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def emu_lists(tr_gene, sets):
    """-> (off uint64 [n_classes + 1], ids int32 [n_pairs]) as the CPU build makes them"""
    tr_gene = np.ascontiguousarray(tr_gene, np.int32)
    off, ids = csr_of(sets)
    out_off, out_ids = np.zeros(len(sets) + 1, np.uint64), np.zeros(max(len(ids), 1), np.int32)
    n = int(emu().busgenes_emu_lists(tr_gene.ctypes.data, off.ctypes.data, ids.ctypes.data, len(sets), out_off.ctypes.data, out_ids.ctypes.data, len(out_ids)))
    return out_off, out_ids[:n]


def table_of(lists):
    """gene lists -> the CSR (off uint64, ids int32) the emu's rule takes"""
    off = np.zeros(len(lists) + 1, np.uint64)
    if len(lists):
        off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    ids = np.array([g for x in lists for g in x] + [0], np.int32)
    return off, ids


def emu_group(lists, classes):
    off, ids = table_of(lists)
    cl = np.ascontiguousarray(classes, np.int32)
    return int(emu().busgenes_emu_group(off.ctypes.data, ids.ctypes.data, len(lists), cl.ctypes.data, len(cl)))


def emu_count(lists, rec, mode):
    """records in key order -> (rc, barcodes, entries ENTRY, stats dict with n_wave_groups); rc 0, or 1 class outside the table / 2 unsorted / 3 overflow"""
    off, ids = table_of(lists)
    rec = np.ascontiguousarray(rec, REC)
    n = max(len(rec), 1)
    bc, en, st = np.zeros(n, np.uint64), np.zeros(n, ENTRY), GeneCountStats()
    rc = int(emu().busgenes_emu_count(off.ctypes.data, ids.ctypes.data, len(lists), rec.ctypes.data, len(rec), mode, bc.ctypes.data, en.ctypes.data, C.byref(st)))
    stats = {k: int(getattr(st, k)) for k, _ in GeneCountStats._fields_ if k not in ("last_ms", "resolve_ms")}
    return rc, bc[:stats["n_barcodes"]], en[:stats["n_entries"]], stats
