"""The manyclass_pe fixture (tests/golden/make_manyclass.py: items that meet 2 to several hundred (unitig, set) classes) and the per-item
figures the tests of kernel A's long class lists select by, computed with the CPU emulation of the stepper (tests/emu).  Shared by the
generator, the CPU tests and the GPU tests, so that all three count the same way.

Per item:  D  distinct classes (what the first pass's eight-entry list would have to hold),
           A  classes the second pass appends (duplicates stay unless they are neighbours),
           S  distinct non-empty transcript sets the classes map to (the sets of the item's tuple record)."""
from __future__ import annotations

import ctypes as C
import gzip
import json
import os
import shutil
import subprocess
from dataclasses import dataclass, field

import numpy as np

from tests import common

NAME = "manyclass_pe"
# kallisto_amd/csrc/kamd_match.hip: entries of the first pass's list, of the second pass's; kamd_dev.h: sets of the straight-line kernel's list
FIRST_CAP, LONG_CAP, TUPLE_CAP_BIG = 8, 192, 1024
FLAGS_FIRST, FLAGS_APPEND, FLAG_NO_JUMP = 1 | 4, 1 | 4 | 8, 2
MATE1, MATE2, ID_MASK = 0x40000000, 0x80000000, 0x3FFFFFFF
LANE_SLOT_A = (63, 64, 65, 127, 128, 129, 191, 192)
MIN_ITEMS = 4


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


# ---- tests/emu_classlist (TEST INFRASTRUCTURE): the stepper's class lists and the straight-line matcher with options, on an emu_binding.EmuIndex ----
_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu_classlist")], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(_HERE, "emu_classlist", "libkamd_classlist_emu.so"))
        L.emu_class_list.restype = C.c_int64
        L.emu_ec_state_opts.restype = C.c_int64
        _lib = L
    return _lib


def class_list(ix, words, l16, item, paired, max_len, flags, cap=1024):
    """The class list of one item as kernel A's stepper builds it (uint32 entries: class | mate 1 in bit 30 | mate 2 in bit 31);
    flags as emu_binding.tuples' use_stepper: FLAGS_FIRST the first pass (distinct classes), FLAGS_APPEND the second pass's append-only list,
    + FLAG_NO_JUMP."""
    out = np.zeros(cap, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = lib().emu_class_list(C.byref(ix.view), p(words), p(l16), C.c_uint64(item), int(paired), C.c_int32(max_len), int(flags), p(out), C.c_uint64(cap))
    if n < 0:
        raise RuntimeError(f"emu_class_list: more than {cap} classes")
    return out[:n].copy()


def ec_state_opts(ix, words, l16, n_items, paired, max_len, no_jump=0, union=0, item_ids=None):
    """emu_binding.ec_state with --no-jump / --union (the records' sets then carry the mate flags) and set lists of up to 1024 entries, over the
    items `item_ids` of the packed reads (None: all n_items): (dense, stream, rec_off)"""
    ids = None if item_ids is None else np.ascontiguousarray(item_ids, np.uint64)
    n = n_items if ids is None else len(ids)
    dense = np.zeros(max(ix.view.n_ecs, 1), np.uint32)
    cap = max(n * (TUPLE_CAP_BIG + 2), 1024)
    stream = np.zeros(cap, np.uint32)
    rec_off = np.zeros(max(n, 1), np.uint64)
    nr = C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nw = lib().emu_ec_state_opts(C.byref(ix.view), p(words), p(l16), None if ids is None else p(ids), C.c_uint64(n), int(paired), C.c_int32(max_len),
                                 int(no_jump) | (int(union) << 1), p(dense), p(stream), C.c_uint64(cap), p(rec_off), C.byref(nr))
    if nw < 0:
        raise RuntimeError(f"emu_ec_state_opts failed {nw}")
    return dense, stream[:nw].copy(), rec_off[:nr.value].copy()


@dataclass
class Item:
    D: int
    A: int
    S: int
    both_mates: bool         # both mates contribute classes
    mate_merge: bool         # mate 2's first class is mate 1's last: one appended entry carries both flags
    mate2_revisit: bool      # mate 2 appends a class that mate 1 appended before its last
    cross_slice_dup: bool    # a set's first and a later entry lie in different 64-entry slices of the appended list
    appended: np.ndarray = field(repr=False, default=None)


def class_tables(ix):
    """(class -> set id, set is non-empty) of an EmuIndex"""
    from kallisto_amd import api
    v = ix.view
    uec_ec = api._np(v.uec_ec, v.n_uec, np.uint32)
    ec_off = api._np(v.ec_off, v.n_ecs + 1, np.uint64)
    return uec_ec, np.diff(ec_off.astype(np.int64)) > 0


def item_figures(ix, words, l16, n_items, paired, max_len, no_jump=0, tables=None) -> list:
    """D, A, S and the properties above of every item, item by item through class_list"""
    uec_ec, nonempty = tables or class_tables(ix)
    nj = FLAG_NO_JUMP if no_jump else 0
    out = []
    for i in range(n_items):
        first = class_list(ix, words, l16, i, paired, max_len, FLAGS_FIRST | nj)
        app = class_list(ix, words, l16, i, paired, max_len, FLAGS_APPEND | nj)
        cls = (app & ID_MASK).astype(np.int64)
        sets = uec_ec[cls].astype(np.int64)
        keep = nonempty[sets]
        assert set(cls.tolist()) == set((first & ID_MASK).tolist()), "the append-only list holds other classes than the first pass's"
        m1, m2 = (app & MATE1) != 0, (app & MATE2) != 0
        last1 = int(np.flatnonzero(m1).max()) if m1.any() else -1
        revisit = bool(m2.any() and last1 > 0 and np.isin(cls[m2 & ~m1], cls[:last1]).any())
        kept = sets[keep]     # k_classify_long's compacted list: the non-empty sets in the order of the appended classes
        cross = False
        seen = {}
        for j, e in enumerate(kept.tolist()):
            if e in seen and seen[e] // 64 != j // 64:
                cross = True
                break
            seen.setdefault(e, j)
        out.append(Item(len(first), len(app), len(set(kept.tolist())), bool(m1.any() and m2.any()), bool((m1 & m2).any()), revisit, cross, app))
    return out


def route(it: Item) -> str:
    """"first": the first pass finishes the item; "long": k_classify_long; "straight": the second pass's list overflows again"""
    if it.D <= FIRST_CAP:
        return "first"
    return "long" if it.A <= LONG_CAP else "straight"


def groups(figs, oc=None) -> dict:
    """the item numbers of every count section 1 of the fixture's description asks for; oc: per item the strand filter's outcome (0 / 1 / 2)"""
    g = {}
    sel = lambda f: [i for i, it in enumerate(figs) if f(it)]
    for d in (7, 8, 9):
        g[f"D={d}"] = sel(lambda it: it.D == d)
    g["D=8,A>=40"] = sel(lambda it: it.D == 8 and it.A >= 40)
    g["D>=2,S=1"] = sel(lambda it: it.D >= 2 and it.S == 1)
    g["D=8,S<8"] = sel(lambda it: it.D == 8 and 0 < it.S < 8)
    for a in LANE_SLOT_A:
        g[f"A={a}"] = sel(lambda it: it.D > FIRST_CAP and it.A == a)
    g["long,S<=8,A>=150"] = sel(lambda it: route(it) == "long" and it.S <= 8 and it.A >= 150)
    g["long,cross_slice_dup"] = sel(lambda it: route(it) == "long" and it.cross_slice_dup)
    g["long,S>64"] = sel(lambda it: route(it) == "long" and it.S > 64)
    g["long,S>128"] = sel(lambda it: route(it) == "long" and it.S > 128)
    g["A=193"] = sel(lambda it: it.D > FIRST_CAP and it.A == 193)
    g["A=194"] = sel(lambda it: it.D > FIRST_CAP and it.A == 194)
    g["A>=300"] = sel(lambda it: it.D > FIRST_CAP and it.A >= 300)
    g["D=9,A>=193"] = sel(lambda it: it.D == 9 and it.A >= 193)
    g["S>256"] = sel(lambda it: it.S > 256)
    g["long,both_mates"] = sel(lambda it: route(it) == "long" and it.both_mates)
    g["long,mate_merge"] = sel(lambda it: route(it) == "long" and it.mate_merge)
    g["long,mate2_revisit"] = sel(lambda it: route(it) == "long" and it.mate2_revisit)
    if oc is not None:
        for k, name in ((1, "removed"), (2, "changed"), (0, "unchanged")):
            g[f"long,filter_{name}"] = [i for i, it in enumerate(figs) if route(it) == "long" and it.S > 0 and oc[i] == k]
    return g


# groups that need one item only
SINGLE = {"A>=300": 1, "S>256": 1}


def filter_outcomes(ix, words, l16, n_items, max_len, strand) -> np.ndarray:
    """per paired item what the strand filter does to its transcript set: 0 nothing (or the set is empty anyway), 1 removes everything,
    2 changes it -- the straight-line emulation with and without the filter"""
    from tests import emu_binding as E
    o0, i0 = E.pseudoalign_opts(ix, words, l16, n_items, 1, max_len, 0, 0, 0, 0)
    o1, i1 = E.pseudoalign_opts(ix, words, l16, n_items, 1, max_len, 0, strand, 0, 0)
    oc = np.zeros(n_items, np.int64)
    for i in range(n_items):
        a, b = i0[o0[i]:o0[i + 1]], i1[o1[i]:o1[i + 1]]
        oc[i] = 0 if np.array_equal(a, b) else (1 if len(b) == 0 else 2)
    return oc
