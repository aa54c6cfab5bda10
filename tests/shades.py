"""The shades_pe fixture (tests/golden/make_shades.py: an index with shades, targets named <base>_shade_<variant>), the class rule of such an
index restated on Python sets, and the binding of tests/emu_shade (the per-item logic of kamd_core.h on the CPU).  Shared by the CPU tests
and the GPU tests, so that both look at the same sets with the same code."""
from __future__ import annotations

import ctypes as C
import gzip
import json
import os
import shutil
import subprocess

import numpy as np

from tests import common

NAME = "shades_pe"
TAG = "_shade_"
NOT_A_SHADE = 0xFFFFFFFF
EC_MATE1, EC_MATE2, EC_ID_MASK = 0x40000000, 0x80000000, 0x3FFFFFFF
TUPLE_CAP = 12
HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu_shade", "libkamd_shade_emu.so")
DUMP_VARIANTS = ("pe", "pe_fr", "pe_rf", "pe_union", "pe_nojump", "se_so")


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


def load_expected(variant):
    return common.load_expected(NAME, variant)


def colours_of_names(names):
    """The load rule on the names alone: colour[i] = first earlier target named by the text before "_shade_", NOT_A_SHADE for a target that is
    no shade; raises ValueError for a shade without such a target."""
    first, out = {}, np.full(len(names), NOT_A_SHADE, np.uint32)
    for i, n in enumerate(names):
        at = n.find(TAG)
        if at > 0:
            if n[:at] not in first:
                raise ValueError(f"shade {n} has no base target before it")
            out[i] = first[n[:at]]
        first.setdefault(n, i)
    return out


class ShadeRule:
    """The class of an item on an index with shades, on Python sets.  set_members(e) -> the members of index set e; colour[t] as above.
    Cores are intersected (per mate united first with `union`; a mate without sets imposes nothing), then every shade of any of the
    item's sets whose colour survived is united back in."""

    def __init__(self, set_members, colour):
        self.set_members, self.colour, self._split = set_members, np.asarray(colour), {}
        self.is_shade = self.colour != NOT_A_SHADE

    def split(self, e):
        """(membership row of the core, shades) of index set e"""
        if e not in self._split:
            m = np.asarray(self.set_members(e), np.int64)
            row = np.zeros(len(self.colour), bool)
            row[m[~self.is_shade[m]]] = True
            self._split[e] = (row, m[self.is_shade[m]])
        return self._split[e]

    def __call__(self, sets, union=False):
        """sets = the ids of the distinct non-empty sets the item's hits carried (with `union` a list of (id, in mate 1, in mate 2));
        returns an ascending tuple"""
        none = np.zeros(len(self.colour), bool)
        if not union:
            ids = list(sets)
            core = np.logical_and.reduce([self.split(e)[0] for e in ids]) if ids else none
        else:
            ids = [e for e, _, _ in sets]
            mates = [[e for e, a, b in sets if a], [e for e, a, b in sets if b]]
            parts = [np.logical_or.reduce([self.split(e)[0] for e in m]) for m in mates if m]
            core = np.logical_and.reduce(parts) if parts else none
        if not core.any():
            return ()
        out = core.copy()
        for e in ids:
            sh = self.split(e)[1]
            out[sh[core[self.colour[sh]]]] = True
        return tuple(np.flatnonzero(out).tolist())


def shaded_class(set_members, colour, sets, union=False):
    return ShadeRule(set_members, colour)(sets, union)


# ---- tests/emu_shade ----------------------------------------------------------------------------------------------------------
_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_shade")], stdout=subprocess.DEVNULL)
        L = C.CDLL(EMU)
        L.kamd_last_error.restype = C.c_char_p
        L.kamd_packed_record_words.restype = C.c_uint64
        L.kamd_index_target_name.restype = C.c_char_p
        L.emu_shade_quant.restype = C.c_int64
        _lib = L
    return _lib


class EmuIndex:
    """the product's index loader, compiled into the emulation library"""

    def __init__(self, path):
        from kallisto_amd.api import _View, _np
        L = emu()
        self.h = C.c_void_p()
        rc = L.kamd_index_load(os.fsencode(path), 2, C.byref(self.h))
        if rc != 0:
            raise RuntimeError(L.kamd_last_error().decode())
        self.view = v = _View()
        L.kamd_index_get_view(self.h, C.byref(v))
        self.n_targets, self.n_shades = int(v.n_targets), int(v.n_shades)
        self.names = [L.kamd_index_target_name(self.h, C.c_uint64(i)).decode() for i in range(self.n_targets)]
        self.colour = _np(v.shade_colour, v.n_targets, np.uint32).copy() if self.n_shades else np.full(self.n_targets, NOT_A_SHADE, np.uint32)
        self.ec_off = _np(v.ec_off, v.n_ecs + 1, np.uint64).astype(np.int64)
        self.ec_ids = _np(v.ec_ids, v.ec_nnz, np.uint32).astype(np.int64)
        if self.n_shades:
            self.core_off = _np(v.core_off, v.n_ecs + 1, np.uint64).astype(np.int64)
            self.core_ids = _np(v.core_ids, v.core_nnz, np.uint32).astype(np.int64)
            self.shade_off = _np(v.shade_off, v.n_ecs + 1, np.uint64).astype(np.int64)
            self.shade_ids = _np(v.shade_ids, v.shade_nnz, np.uint32).astype(np.int64)

    def members(self, e):
        return self.ec_ids[self.ec_off[e]:self.ec_off[e + 1]].tolist()

    def save(self, path):
        rc = emu().kamd_index_save(self.h, os.fsencode(path))
        if rc != 0:
            raise RuntimeError(emu().kamd_last_error().decode())

    def close(self):
        if self.h:
            emu().kamd_index_free(self.h)
            self.h = None


def pack(seqs):
    L = emu()
    n = len(seqs)
    lens = np.array([len(s) for s in seqs], np.int32)
    max_len = max(int(lens.max(initial=1)), 1)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    words = np.zeros(max(n * L.kamd_packed_record_words(max_len), 1), np.uint32)
    l16 = np.zeros(max(n, 1), np.uint16)
    rc = L.kamd_pack_reads_host(b"".join(seqs), off.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), C.c_uint64(n),
                                C.c_int32(max_len), words.ctypes.data_as(C.c_void_p), l16.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError(L.kamd_last_error().decode())
    return words, l16, max_len


def emu_quant(ix: EmuIndex, r1, r2, opts, sets_stride=0):
    """The per-item logic over all items.  opts = common.parse_variant(...).  Returns dict(ecs = the EC multiset, nproc, flens = the
    fragment-length sample (first 10 000 pairs with a class of one target and 0 < length < 1000), n_sets, n_shade_union, sets)."""
    paired = bool(opts["paired"])
    reads = common.interleave(r1, r2 if paired else None)
    words, l16, max_len = pack(reads)
    n = len(r1)
    out_off = np.zeros(n + 1, np.uint64)
    cap = n * min(ix.n_targets, 4096)   # (a --union class can hold most targets)
    out_ids = np.zeros(cap, np.uint32)
    tl = np.zeros(n, np.int32)
    n_sets, n_su = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    sets = np.zeros((n, sets_stride), np.uint32) if sets_stride else None
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    r = emu().emu_shade_quant(C.byref(ix.view), p(words), p(l16), C.c_uint64(n), int(paired), C.c_int32(max_len), int(opts["strand"]),
                              int(opts["no_jump"]) | (int(opts["union"]) << 1), p(out_off), p(out_ids), C.c_uint64(cap), p(tl), p(n_sets), p(n_su),
                              p(sets) if sets_stride else None, C.c_uint64(sets_stride))
    if r < 0:
        raise RuntimeError(f"emu_shade_quant failed {r}")
    raw, flens, used = {}, np.zeros(common.MAX_FRAG_LEN, np.uint32), 0
    off = out_off.astype(np.int64)
    for i in range(n):
        if off[i + 1] == off[i]:
            continue
        key = out_ids[off[i]:off[i + 1]].tobytes()      # (a --union class holds a thousand targets: tuples only of the distinct ones)
        raw[key] = raw.get(key, 0) + 1
        if paired and opts["fld"] == 0.0 and used < 10000 and off[i + 1] - off[i] == 1 and 0 < tl[i] < common.MAX_FRAG_LEN:
            flens[tl[i]] += 1
            used += 1
    ecs = {tuple(np.frombuffer(k, np.uint32).tolist()): c for k, c in raw.items()}
    return dict(ecs=ecs, nproc=n, flens=flens, n_sets=n_sets, n_shade_union=n_su, sets=sets)


def stats_of_fixture(idx_path, r1, r2):
    """what make_shades.py records in case.json beside the reference's own numbers"""
    ix = EmuIndex(idx_path)
    res = emu_quant(ix, r1, r2, common.parse_variant([]))
    out = dict(shade_ids=np.flatnonzero(ix.colour != NOT_A_SHADE), core_sizes=np.diff(ix.core_off),
               more_than_12_sets=int((res["n_sets"] > TUPLE_CAP).sum()), largest_shade_union=int(res["n_shade_union"].max()))
    ix.close()
    return out
