"""What the per-read class tests share: the fixtures of tests/golden/bus_num (the reference's `bus -n` output), the cut of an existing fixture's
reads into the samples of a case, the oracle's per-read transcript sets, and the ctypes binding of tests/emu_readec/libkamd_readec_emu.so
(TEST INFRASTRUCTURE: kamd_readec.h compiled for the CPU)."""
from __future__ import annotations

import ctypes as C
import functools
import gzip
import json
import os
import subprocess

import numpy as np

from tests import common

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(common.GOLDEN, "bus_num")
BUS_CASES = ["ref_test_pe", "yeast_se", "mosaic_pe"]
NONE, FOREIGN = -1, -2

_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_readec")], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(HERE, "emu_readec", "libkamd_readec_emu.so"))
        L.rec_emu_capacity.restype = C.c_uint64
        L.rec_emu_capacity.argtypes = [C.c_uint64]
        L.rec_emu_build.restype = C.c_uint64
        L.rec_emu_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]
        L.rec_emu_lookup.restype = None
        L.rec_emu_lookup.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        _lib = L
    return _lib


def csr(sets):
    off = np.zeros(len(sets) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
    ids = np.array([x for s in sets for x in s] + [0], np.uint32)   # (one spare word: never an empty buffer)
    return off, ids


def emu_table(sets, cap=None, tag_mask=2 ** 64 - 1):
    """the table of the CSR `sets` at capacity `cap` (None: the library's own) -> (slots, cap, failed rows)"""
    L = emu()
    off, ids = csr(sets)
    cap = int(L.rec_emu_capacity(len(sets))) if cap is None else cap
    slots = np.full(2 * cap, 0xAB, np.uint64)
    failed = L.rec_emu_build(off.ctypes.data, ids.ctypes.data, len(sets), slots.ctypes.data, cap, tag_mask)
    return slots, cap, int(failed)


def emu_lookup(sets, slots, cap, queries, tag_mask=2 ** 64 - 1):
    off, ids = csr(sets)
    qoff, qids = csr(queries)
    out = np.full(len(queries), -7, np.int32)
    emu().rec_emu_lookup(slots.ctypes.data, cap, tag_mask, off.ctypes.data, ids.ctypes.data, qoff.ctypes.data, qids.ctypes.data, len(queries), out.ctypes.data)
    return out


def load_bus_case(name):
    d = os.path.join(GOLD, name)
    meta = json.load(open(os.path.join(d, "case.json")))
    lines = []
    with gzip.open(os.path.join(d, "expected.txt.gz"), "rt") as f:
        for l in f:
            fl, bc, s = l.rstrip("\n").split("\t")
            lines.append((int(fl), int(bc), tuple(int(x) for x in s.split(","))))
    return meta, lines


def samples_of(meta):
    """[(barcode, first read, end read)] of the case's samples, in the order of the command line / batch file"""
    _, _, r1, _ = common.load_case(meta["fixture"])
    n, cuts = len(r1), meta["cuts"]
    ranges = [(int(round(cuts[s] * n)), int(round(cuts[s + 1] * n))) for s in range(len(cuts) - 1)]
    ids = meta["batch_ids"]
    if ids is None:
        bcs = list(range(len(ranges)))
    else:
        seen = {}
        bcs = [seen.setdefault(i, len(seen)) for i in ids]
    return [(bc, a, b) for bc, (a, b) in zip(bcs, ranges)]


def bus_oracle_opts(meta):
    """`bus -x bulk`: no positional filter (single_overhang), single-end reads with partial matches (src/main.cpp:762)"""
    from oracle import oracle as O
    flags = meta["bus_flags"]
    paired = "--paired" in flags
    strand = 1 if "--fr-stranded" in flags else (2 if "--rf-stranded" in flags else 0)
    return O.Opts(1 if paired else 0, 0.0 if paired else 200.0, 0.0 if paired else 20.0, 1, strand, int("--no-jump" in flags), int("--union" in flags))


@functools.lru_cache(maxsize=None)
def oracle_sets(fixture, opts_key):
    """the oracle's transcript set of every read (pair) of a fixture under the options (paired, fld, sd, single_overhang, strand, no_jump, union):
    a tuple of tuples, () = not pseudoaligned.  Computed once per (fixture, options) and shared."""
    from oracle import oracle as O
    _, idx, r1, r2 = common.load_case(fixture)
    paired, fld, sd, so, strand, nj, un = opts_key
    opts = O.Opts(paired, fld, sd, so, strand, nj, un)
    ix = O.Index(idx)
    out = []
    for i in range(len(r1)):
        s, _, _ = ix.pseudoalign(opts, r1[i], r2[i] if paired else None, mean_fl=fld, has_mean_fl=fld != 0.0)
        out.append(tuple(s))
    ix.close()
    return tuple(out)


def opts_key(o):
    return (int(o.paired), float(o.fld), float(o.sd), int(o.single_overhang), int(o.strand), int(o.no_jump), int(o.do_union))
