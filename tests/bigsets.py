"""The bigsets_pe fixture (tests/golden/make_bigsets.py: transcript sets of 129 to 4400 members) and the host reference of EC
resolution over it: plain set algebra on a boolean membership matrix.  Shared by the CPU tests (through oracle.Index) and the GPU
tests (through kallisto_amd.Index), so that both look at the same sets with the same code."""
from __future__ import annotations

import ctypes as C
import gzip
import json
import os
import shutil
from dataclasses import dataclass

import numpy as np

from tests import common

NAME = "bigsets_pe"
BOUNDARY_SIZES = (16, 17, 64, 65, 128, 129, 1024, 1025, 4096, 4097)
# the thresholds of kallisto_amd/csrc/kamd_ec.hip and kamd_dev.h
RES_BIG_MIN, TUPLE_CAP, CAND_SINGLE_WAVE, BM_MIN_MEMBERS, RB_CAND_BIG, RB_CAND_HUGE, RB_MAXSETS, TUPLE_CAP_BIG = 16, 12, 64, 128, 1024, 4096, 256, 1024
SIZE_CLASSES = ((1, 16), (17, 64), (65, 128), (129, 1024), (1025, 4096), (4097, 1 << 30))


def unpack_index(tmp_dir) -> str:
    """gunzip the committed index.idx.gz into tmp_dir; the path of index.idx"""
    out = os.path.join(str(tmp_dir), "index.idx")
    with gzip.open(os.path.join(common.case_dir(NAME), "index.idx.gz"), "rb") as fi, open(out, "wb") as fo:
        shutil.copyfileobj(fi, fo)
    return out


def load_reads():
    """(case.json, mate 1 reads, mate 2 reads)"""
    d = common.case_dir(NAME)
    with open(os.path.join(d, "case.json")) as f:
        meta = json.load(f)

    def lines(p):
        with gzip.open(p, "rb") as f:
            return [x.rstrip(b"\n") for x in f]
    return meta, lines(os.path.join(d, "reads_1.txt.gz")), lines(os.path.join(d, "reads_2.txt.gz"))


@dataclass
class Sets:
    """the de-duplicated transcript sets of an index as CSR, and which targets are on-listed"""
    off: np.ndarray       # int64 [n_sets + 1]
    ids: np.ndarray       # int64 [nnz], ascending inside a set
    onlist: np.ndarray    # bool [n_targets]
    n_targets: int

    def __post_init__(self):
        self.sizes = np.diff(self.off)
        self._matrix = None

    def members(self, e):
        return self.ids[self.off[e]:self.off[e + 1]]

    @property
    def matrix(self):
        """bool [n_sets, n_targets]: set e holds target t, and t is on-listed"""
        if self._matrix is None:
            m = np.zeros((len(self.sizes), self.n_targets), bool)
            m[np.repeat(np.arange(len(self.sizes)), self.sizes), self.ids] = True
            self._matrix = m & self.onlist[None, :]
        return self._matrix

    def intersect(self, set_ids):
        """the on-listed targets that every one of the sets holds, ascending"""
        return np.flatnonzero(self.matrix[np.asarray(set_ids, np.int64)].all(axis=0))


def sets_of_oracle_index(oix) -> Sets:
    from oracle import oracle as O
    L = O.lib()
    off, parts = [0], []
    for e in range(oix.num_ecs):
        p = C.POINTER(C.c_uint32)()
        n = int(L.ko_index_ec(oix.h, e, C.byref(p)))
        if n:
            parts.append(np.ctypeslib.as_array(p, shape=(n,)).astype(np.int64))
        off.append(off[-1] + n)
    ids = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return Sets(np.array(off, np.int64), ids, np.ones(oix.num_targets, bool), int(oix.num_targets))


def sets_of_device_index(index) -> Sets:
    """from kallisto_amd.Index: the host tables that kamd_index_upload copies to the device (view.ec_off / ec_ids / onlist_bits)"""
    from kallisto_amd import api
    off, ids = index.ec_sets()
    v = index.view
    bits = api._np(v.onlist_bits, v.onlist_words, np.uint32)
    t = np.arange(int(v.n_targets))
    onlist = ((bits[t >> 5] >> (t & 31).astype(np.uint32)) & 1).astype(bool)
    return Sets(off.astype(np.int64), ids.astype(np.int64), onlist, int(v.n_targets))


def size_histogram(sizes) -> dict:
    sizes = np.asarray(sizes)
    return {f"{lo}..{hi}" if hi < (1 << 30) else f"{lo}..": int(((sizes >= lo) & (sizes <= hi)).sum()) for lo, hi in SIZE_CLASSES}


def expected_ecs(sets: Sets, records, dense=None) -> dict:
    """What kamd_ec_finalize must produce for tuple records [(count, [set ids])] and dense counts {set id: count}: the multiset
    {ascending transcript tuple: count} -- a tuple's EC is the intersection of its sets, a dense entry's EC the set itself (on-listed
    members only), equal member lists are merged and their counts summed, empty results and zero counts are dropped."""
    out = {}
    for cnt, es in records:
        if cnt == 0:
            continue
        key = tuple(sets.intersect(es).tolist())
        if key:
            out[key] = out.get(key, 0) + int(cnt)
    for e, cnt in (dense or {}).items():
        if cnt == 0:
            continue
        key = tuple(sets.intersect([e]).tolist())
        if key:
            out[key] = out.get(key, 0) + int(cnt)
    return out


def path_of(sets: Sets, es) -> str:
    """Which kernel path resolves the tuple, from the sizes of its sets alone (kamd_ec.hip: k_bound_tuples, k_resolve, k_resolve_big):
    "all_pairs" | "chunk_mask" | "big1024" | "big4096" | "plain" """
    sz = sets.sizes[np.asarray(es, np.int64)]
    m, nb = len(es), int(sz.min())
    if nb <= RES_BIG_MIN:
        return "all_pairs" if m <= TUPLE_CAP and int(sz.max()) <= RES_BIG_MIN else "chunk_mask"
    if m > RB_MAXSETS or nb > RB_CAND_HUGE:
        return "plain"
    return "big1024" if nb <= RB_CAND_BIG else "big4096"
