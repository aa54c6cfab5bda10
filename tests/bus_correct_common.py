"""What the tests of the barcode whitelists (kamd_bus_whitelist_parse, kamd_bus_whitelist_create, kamd_bus_correct, `bus_sc -w`) share:

  * a brute-force restatement of the rule (py_status, py_correct): a Python `set` for the whitelist and a loop over the 3 L neighbours of a barcode
    -- the yardstick everywhere, never the code under test;
  * the ctypes binding of tests/emu_buscorrect/libkamd_buscorrect_emu.so (TEST INFRASTRUCTURE: kamd_buscorrect.h compiled for the CPU, with a plain
    host build of the table);
  * the inputs: whitelists and record mixtures by a seeded generator, keys that share a home bucket, the golden cases' whitelists."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from tests import bus_sc_common as B
from tests.bus_sort_common import REC, make_records

HERE = os.path.dirname(os.path.abspath(__file__))
EXACT, CORRECTED, AMBIGUOUS, UNCORRECTABLE = 0, 1, 2, 3
STAT_KEYS = ("n_exact", "n_corrected", "n_ambiguous", "n_uncorrectable")
LENGTHS = [1, 2, 8, 16, 21, 22, 31, 32]
SIZES = [1, 2, 7, 8, 9, 1000]
ALL_ONES = 2 ** 64 - 1


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def py_neighbours(b, L):
    """the 3 L barcodes that differ from b in exactly one base position"""
    return [b ^ (x << (2 * p)) for p in range(L) for x in (1, 2, 3)]


def py_status(W, L, b):
    """W: a set of ints -> (status, the barcode the record keeps or None)"""
    if b >> (2 * L):
        return UNCORRECTABLE, None
    if b in W:
        return EXACT, b
    near = [w for w in py_neighbours(b, L) if w in W]
    if len(near) == 1:
        return CORRECTED, near[0]
    return (AMBIGUOUS if near else UNCORRECTABLE), None


def py_correct(W, L, rec):
    """REC array -> (the survivors in input order with their barcodes corrected, status uint8 [n], counters dict)"""
    W = set(int(w) for w in W)
    memo, status, fixed = {}, np.zeros(len(rec), np.uint8), rec["barcode"].copy()
    for i, b in enumerate(rec["barcode"].tolist()):
        if b not in memo:
            memo[b] = py_status(W, L, b)
        status[i] = memo[b][0]
        if memo[b][1] is not None:
            fixed[i] = memo[b][1]
    out = rec.copy()
    out["barcode"] = fixed
    out = np.ascontiguousarray(out[status <= CORRECTED])
    stats = {k: int((status == s).sum()) for s, k in enumerate(STAT_KEYS)}
    stats.update(n_in=len(rec), n_out=len(out))
    return out, status, stats


def encode(s):
    r = 0
    for ch in s.upper():
        r = (r << 2) | "ACGT".index(ch)
    return r


def decode(b, L):
    return "".join("ACGT"[(b >> (2 * (L - 1 - i))) & 3] for i in range(L))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# emu binding
# ---------------------------------------------------------------------------------------------------------------------------------------------------
_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_buscorrect")], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(HERE, "emu_buscorrect", "libkamd_buscorrect_emu.so"))
        L.buscorrect_emu_n_buckets.restype = C.c_uint64
        L.buscorrect_emu_n_buckets.argtypes = [C.c_uint64]
        L.buscorrect_emu_home.restype = C.c_uint64
        L.buscorrect_emu_home.argtypes = [C.c_uint64, C.c_uint64]
        L.buscorrect_emu_neighbour.restype = C.c_uint64
        L.buscorrect_emu_neighbour.argtypes = [C.c_uint64, C.c_int, C.c_int]
        L.buscorrect_emu_build.restype = C.c_void_p
        L.buscorrect_emu_build.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_uint64]
        L.buscorrect_emu_free.restype = None
        L.buscorrect_emu_free.argtypes = [C.c_void_p]
        L.buscorrect_emu_distinct.restype = C.c_uint64
        L.buscorrect_emu_distinct.argtypes = [C.c_void_p]
        L.buscorrect_emu_max_chain.restype = C.c_uint32
        L.buscorrect_emu_max_chain.argtypes = [C.c_void_p]
        L.buscorrect_emu_table_buckets.restype = C.c_uint64
        L.buscorrect_emu_table_buckets.argtypes = [C.c_void_p]
        L.buscorrect_emu_lookup.restype = C.c_int
        L.buscorrect_emu_lookup.argtypes = [C.c_void_p, C.c_uint64]
        L.buscorrect_emu_correct.restype = C.c_uint64
        L.buscorrect_emu_correct.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


class EmuWhitelist:
    """the CPU build's table of a list of codes; n_buckets = 0: the capacity rule's"""

    def __init__(self, codes, L, n_buckets=0):
        codes = np.ascontiguousarray(codes, np.uint64)
        self.h = emu().buscorrect_emu_build(codes.ctypes.data, len(codes), L, n_buckets)
        if not self.h:
            raise ValueError("the CPU build refuses the whitelist")
        self.n_distinct = int(emu().buscorrect_emu_distinct(self.h))
        self.max_chain = int(emu().buscorrect_emu_max_chain(self.h))
        self.n_buckets = int(emu().buscorrect_emu_table_buckets(self.h))

    def __contains__(self, key):
        return bool(emu().buscorrect_emu_lookup(self.h, int(key)))

    def correct(self, rec):
        """-> (survivors REC, status uint8 [n], counters dict) in the shape of py_correct"""
        rec = np.ascontiguousarray(rec, REC)
        out, status, counts = np.zeros(max(len(rec), 1), REC), np.zeros(max(len(rec), 1), np.uint8), np.zeros(4, np.uint64)
        m = int(emu().buscorrect_emu_correct(self.h, rec.ctypes.data, len(rec), out.ctypes.data, status.ctypes.data, counts.ctypes.data))
        stats = {k: int(counts[s]) for s, k in enumerate(STAT_KEYS)}
        stats.update(n_in=len(rec), n_out=m)
        return out[:m], status[:len(rec)], stats

    def close(self):
        if self.h:
            emu().buscorrect_emu_free(self.h)
            self.h = None


def home(key, n_buckets):
    return int(emu().buscorrect_emu_home(int(key), n_buckets))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def rand_barcodes(rng, L, n):
    return rng.integers(0, 2 ** 64, n, dtype=np.uint64) & np.uint64(4 ** L - 1)


def random_codes(L, n, seed):
    """n distinct barcodes of L bases (all 4^L where that is fewer), in random order"""
    rng = np.random.default_rng(seed)
    space = 4 ** L
    if space <= 4 * n:
        return rng.permutation(space)[:min(n, space)].astype(np.uint64)
    out = np.unique(rand_barcodes(rng, L, 2 * n + 16))
    assert len(out) >= n
    return out[rng.permutation(len(out))[:n]]


def substitute(rng, b, L, k=1):
    """b with k distinct base positions changed"""
    for p in rng.choice(L, size=k, replace=False).tolist():
        b ^= int(rng.integers(1, 4)) << (2 * p)
    return b


def mixture(W, L, n, seed, p_sub1=0.2, p_sub2=0.1, p_random=0.1):
    """n records: barcodes of W, some with one or two substituted bases, some random; umi, ec, count, flags arbitrary, pad = the input index"""
    rng = np.random.default_rng(seed)
    W = np.asarray(W, np.uint64)
    bc = W[rng.integers(0, len(W), n)].copy()
    kind = rng.random(n)
    p1 = rng.integers(0, L, n)
    p2 = (p1 + rng.integers(1, max(L, 2), n)) % L                      # another position (L = 1: the same one, and no second substitution below)
    x1, x2 = rng.integers(1, 4, n).astype(np.uint64), rng.integers(1, 4, n).astype(np.uint64)
    sub1 = kind < p_sub1 + (p_sub2 if L >= 2 else 0.0)
    sub2 = (kind >= p_sub1) & sub1
    bc[sub1] ^= x1[sub1] << (2 * p1[sub1]).astype(np.uint64)
    bc[sub2] ^= x2[sub2] << (2 * p2[sub2]).astype(np.uint64)
    rnd = (kind >= p_sub1 + p_sub2) & (kind < p_sub1 + p_sub2 + p_random)
    bc[rnd] = rand_barcodes(rng, L, int(rnd.sum()))
    return with_fields(bc, rng)


def with_fields(barcodes, rng):
    n = len(barcodes)
    r = make_records(barcodes, rng.integers(0, 2 ** 63, n, dtype=np.uint64), rng.integers(-5, 1000, n).astype(np.int32),
                     rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
    r["pad"] = np.arange(n)
    return r


def colliding_keys(L, n_keys, n_buckets, bucket, seed):
    """n_keys distinct barcodes of L bases whose home bucket in a table of n_buckets is `bucket`: random keys, kept where the CPU build's hash says so"""
    rng = np.random.default_rng(seed)
    out = []
    seen = set()
    while len(out) < n_keys:
        for k in rand_barcodes(rng, L, 4096).tolist():
            if k not in seen and home(k, n_buckets) == bucket:
                seen.add(k)
                out.append(k)
                if len(out) == n_keys:
                    break
    return np.array(out, np.uint64)


def golden_bc_cases():
    """the cases of tests/golden/bus_sc whose layout has a barcode"""
    return [n for n in B.golden_cases() if B.parse(B.CASES[n]["tech"])[0].parts("bc")[0][0] >= 0]


def golden_whitelist(name):
    """-> (W sorted list, L, the case's golden lines): W = the barcodes of the reference's records without an N in the barcode (flags & 3 == 0)"""
    meta, lines = B.load_golden(name)
    L = int(meta["bus_header"][1])
    return sorted({bc for fl, bc, _, _ in lines if fl & 3 == 0}), L, lines


def whitelist_text(W, L, newline="\n"):
    return "".join(decode(int(w), L) + newline for w in W).encode()
