"""What the translated-search tests share: the fixture of tests/golden/aa_bulk, a plain Python translation to check the
frames against, and the ctypes binding of tests/emu_aa/libkamd_aa_emu.so (TEST INFRASTRUCTURE: kamd_aa.h compiled for the CPU)."""
from __future__ import annotations

import collections
import ctypes as C
import functools
import gzip
import json
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "aa_bulk")
VARIANTS = ("plain", "dlist")
# the standard genetic code, codons in the order AAA, AAC, AAG, AAT, ACA, ... TTT
CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
# amino acid -> comma-free triplet
CFC = {"F": "ACC", "L": "ACA", "I": "ATA", "M": "ATC", "V": "ATT", "S": "CTA", "P": "CTC", "T": "CTT", "A": "AGA", "Y": "AGC",
       "H": "AGT", "Q": "AGG", "N": "CGA", "K": "CGC", "D": "CGT", "E": "CGG", "C": "TGA", "W": "TGC", "R": "TGT", "G": "TGG"}
# the lengths at which the packed layout turns a corner (16 bases per sequence word, 32 per mask word), every l mod 3
FRAME_LENGTHS = list(range(0, 41)) + [47, 48, 49, 95, 96, 97]


def codon_index(c):
    return sum("ACGT".index(b) << (2 * (2 - i)) for i, b in enumerate(c))


def codon_of(i):
    return "".join("ACGT"[(i >> (2 * (2 - j))) & 3] for j in range(3))


def py_frames(read: bytes):
    """the six translated frames of a read, masked bases as N"""
    s = read.decode().upper()
    rc = "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(b, "N") for b in reversed(s))
    out = []
    for f in range(6):
        u = (s if f < 3 else rc)[f % 3:]
        t = ""
        for i in range(0, len(u) - 2, 3):
            c = u[i:i + 3]
            aa = CODE[codon_index(c)] if all(b in "ACGT" for b in c) else "*"
            t += CFC.get(aa, "NNN")
        out.append(t.encode())
    return out


def frame_test_reads(rng):
    """reads of every length of FRAME_LENGTHS: plain, lower case, and with an N in each codon position"""
    reads = []
    for ln in FRAME_LENGTHS:
        s = "".join(rng.choice("ACGT") for _ in range(ln))
        reads.append(s)
        reads.append(s.lower())
        for pos in range(min(ln, 3)):
            i = min(ln - 1, 3 * rng.randrange(0, ln // 3 + 1) + pos)
            reads.append(s[:i] + rng.choice("Nn") + s[i + 1:])
    return [r.encode() for r in reads]


def write_fastq(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def read_ec(path):
    ecs = []
    for i, line in enumerate(gzip.open(path, "rt") if path.endswith(".gz") else open(path)):
        e, trs = line.split()
        assert int(e) == i
        ecs.append(tuple(sorted(int(x) for x in trs.split(","))))
    return ecs


@functools.lru_cache(maxsize=None)
def fixture():
    """reads, and per variant: index path, the reference's EC multiset {set: reads}, its run_info numbers, case.json's entry"""
    case = json.load(open(os.path.join(GOLD, "case.json")))
    reads = gzip.open(os.path.join(GOLD, "reads.txt.gz")).read().split()
    assert len(reads) == case["n_reads"]
    out = {"reads": reads, "case": case}
    for v in VARIANTS:
        ms = collections.Counter()
        for line in gzip.open(os.path.join(GOLD, v, "bus_expected.txt.gz"), "rt"):
            bc, n, s = line.split()
            ms[tuple(int(x) for x in s.split(","))] += int(n)
        out[v] = {"index": os.path.join(GOLD, "index_%s.idx" % v), "multiset": dict(ms),
                  "run_info": json.load(open(os.path.join(GOLD, v, "run_info.json"))), "case": case["variants"][v]}
    return out


# ---- the CPU emulation ----------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_aa")], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(HERE, "emu_aa", "libkamd_aa_emu.so"))
        L.kamd_last_error.restype = C.c_char_p
        L.kamd_packed_record_words.restype = C.c_uint64
        L.aa_emu_pseudoalign.restype = C.c_int64
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack(seqs, max_len=None):
    L = lib()
    n = len(seqs)
    lens = np.array([len(s) for s in seqs], np.int32)
    max_len = max_len or max(int(lens.max(initial=1)), 1)
    off = np.zeros(max(n, 1), np.uint64)
    if n:
        off[1:n] = np.cumsum(lens[:-1].astype(np.uint64))
    rec = int(L.kamd_packed_record_words(max_len))
    words = np.zeros(max(n * rec, 1), np.uint32)
    l16 = np.zeros(max(n, 1), np.uint16)
    rc = L.kamd_pack_reads_host(b"".join(seqs), _p(off), _p(lens), C.c_uint64(n), C.c_int32(max_len), _p(words), _p(l16))
    if rc != 0:
        raise RuntimeError(L.kamd_last_error().decode())
    return words, l16, max_len


def unpack_frames(words, lens, n_frames, max_len):
    """packed records -> byte strings (masked bases as N)"""
    sw = (max_len + 15) // 16 + 1
    rec = sw + (max_len + 31) // 32 + 1
    out = []
    for r in range(n_frames):
        w = words[r * rec:(r + 1) * rec]
        s = bytearray()
        for i in range(int(lens[r])):
            if (int(w[sw + (i >> 5)]) >> (i & 31)) & 1:
                s += b"N"
            else:
                s += b"ACGT"[(int(w[i >> 4]) >> (2 * (i & 15))) & 3:][:1]
        out.append(bytes(s))
    return out


def emu_frames(seqs, max_len=None):
    words, l16, max_len = pack(seqs, max_len)
    n = len(seqs)
    rec = int(lib().kamd_packed_record_words(max_len))
    ow = np.zeros(max(6 * n * rec, 1), np.uint32)
    ol = np.zeros(max(6 * n, 1), np.uint16)
    lib().aa_emu_frames(_p(words), _p(l16), C.c_uint64(n), C.c_int32(max_len), _p(ow), _p(ol))
    return ow, ol, max_len


def emu_codon_table():
    t = np.zeros(64, np.uint8)
    lib().aa_emu_codon_table(_p(t))
    return t


def emu_pseudoalign(index_path, seqs, diag=False):
    from kallisto_amd.api import _View
    L = lib()
    h = C.c_void_p()
    if L.kamd_index_load(index_path.encode(), 2, C.byref(h)) != 0:
        raise RuntimeError(L.kamd_last_error().decode())
    try:
        view = _View()
        L.kamd_index_get_view(h, C.byref(view))
        words, l16, max_len = pack(seqs)
        n = len(seqs)
        outcome = np.zeros(max(n, 1), np.int32)
        clashes = np.zeros(max(n, 1), np.uint32)
        off = np.zeros(n + 1, np.uint64)
        cap = max(n * 64, 1024)
        ids = np.zeros(cap, np.uint32)
        dg = np.zeros(3, np.uint64)
        r = L.aa_emu_pseudoalign(C.byref(view), _p(words), _p(l16), C.c_uint64(n), C.c_int32(max_len), _p(outcome), _p(clashes), _p(off), _p(ids),
                                 C.c_uint64(cap), _p(dg) if diag else None)
        if r < 0:
            raise RuntimeError("aa_emu_pseudoalign failed %d" % r)
    finally:
        L.kamd_index_free(h)
    ms = collections.Counter()
    for i in range(n):
        if outcome[i] >= 0:
            ms[tuple(ids[int(off[i]):int(off[i + 1])].tolist())] += 1
    return {"outcome": outcome[:n], "clashes": clashes[:n], "multiset": dict(ms), "diag": dg}
