"""Workloads that take the translated search beyond what tests/golden/aa_bulk alone reaches: more reads in a call than one pass of the persistent
wavefronts of k_aa_match takes, more than one chunk of a call, reads long enough that the class-list scratch bounds the grid, and frames of up to
65 535 bases.  No GPU: every expected value is the CPU emulation's (tests/emu_aa, pinned to the reference by tests/test_aa_cpu.py; tests/emu_aa_big adds the depth of
the class lists) of the DISTINCT reads, carried to a batch by expected_for; the frames are also checked against aa_common.py_frames."""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np

from tests import aa_common as A

COPIES = 49          # many_reads: 49 x 5 589 = 273 861 entries, more than one chunk of a call
LONG_LEN = 900       # long_reads: a whole protein of the fixture, back-translated
N_FIXTURE_IN_LONG = 2000
# frame lengths in groups of one max_len each (the record stride is the group's): around the fixture's longest read, around the length at which a frame's
# class list outgrows 256 entries, around 66 sequence words / 33 mask words, around 4096, and the longest a record can hold
FRAME_LENGTHS_LONG = [[150, 151, 152, 153], [286, 287, 288, 289], [1053, 1054, 1055, 1056, 1057, 1058], [4095, 4096, 4097, 4098], [65533, 65534, 65535]]
_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(r: bytes) -> bytes:
    return r[::-1].translate(_RC)


def proteins():
    out = []
    for line in open(os.path.join(A.GOLD, "proteins.fa")):
        if line.startswith(">"):
            out.append("")
        else:
            out[-1] += line.strip()
    return out


def many_reads(copies=COPIES, seed=11):
    """an index array into the fixture's reads: every read `copies` times, shuffled, so that a read's neighbours in its group of eight and its place modulo
    the wavefront count differ from copy to copy"""
    n = len(A.fixture()["reads"])
    return np.random.default_rng(seed).permutation(np.tile(np.arange(n, dtype=np.int64), copies))


@functools.lru_cache(maxsize=None)
def long_reads(seed=23):
    """the distinct reads of the long-read workload: per protein the whole protein back-translated with random synonymous codons, its reverse complement,
    the same behind one base, the reverse complement of the same behind two bases (each cut to LONG_LEN: winners in frames 0, 3, 1, 5); a copy of each with
    one substitution and one with an N; then N_FIXTURE_IN_LONG reads of the fixture for the tuple records, the rejected and the empty reads"""
    rng = random.Random(seed)
    synonyms = {aa: [A.codon_of(i) for i in range(64) if A.CODE[i] == aa] for aa in set(A.CODE) - {"*"}}
    whole = []
    for p in proteins():
        nt = "".join(rng.choice(synonyms[a]) for a in p).encode()
        one = rng.choice("ACGT").encode() + nt
        two = (rng.choice("ACGT") + rng.choice("ACGT")).encode() + nt
        whole += [nt[:LONG_LEN], revcomp(nt[:LONG_LEN]), one[:LONG_LEN], revcomp(two[:LONG_LEN])]
    changed = []
    for r in whole:
        i = rng.randrange(len(r))
        changed.append(r[:i] + rng.choice([b for b in "ACGT" if b != chr(r[i])]).encode() + r[i + 1:])
    for r in whole:
        i = rng.randrange(len(r))
        changed.append(r[:i] + b"N" + r[i + 1:])
    fx = A.fixture()["reads"]
    return tuple(whole + changed + [fx[i] for i in sorted(rng.sample(range(len(fx)), N_FIXTURE_IN_LONG))])


def n_whole_long_reads():
    return 4 * len(proteins())


def long_batch(n_distinct, n_entries, seed=29):
    """an index array of n_entries >= n_distinct entries over the distinct reads: each at least once, the rest drawn at random, shuffled"""
    assert n_entries >= n_distinct
    rng = np.random.default_rng(seed)
    return rng.permutation(np.concatenate([np.arange(n_distinct, dtype=np.int64), rng.integers(0, n_distinct, n_entries - n_distinct)]))


@functools.lru_cache(maxsize=None)
def frame_reads_long(seed=31):
    """[(max_len, reads)]: per length of a group of FRAME_LENGTHS_LONG a random read, the same in lower case and one with an N in each codon position (the
    scheme of aa_common.frame_test_reads)"""
    rng = random.Random(seed)
    groups = []
    for lengths in FRAME_LENGTHS_LONG:
        reads = []
        for ln in lengths:
            s = "".join(rng.choices("ACGT", k=ln))
            reads += [s, s.lower()]
            for pos in range(3):
                i = min(ln - 1, 3 * rng.randrange(0, ln // 3 + 1) + pos)
                reads.append(s[:i] + rng.choice("Nn") + s[i + 1:])
        groups.append((max(lengths), [r.encode() for r in reads]))
    return groups


def unpack_frames_np(words, lens, n_frames, max_len):
    """aa_common.unpack_frames without a Python loop over the bases"""
    sw = (max_len + 15) // 16 + 1
    rec = sw + (max_len + 31) // 32 + 1
    w = np.asarray(words[:n_frames * rec], np.uint32).reshape(n_frames, rec)
    out = []
    for r in range(n_frames):
        tl = int(lens[r])
        base = ((w[r, :sw - 1, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).ravel()[:tl]
        masked = ((w[r, sw:, None] >> np.arange(32, dtype=np.uint32)) & 1).ravel()[:tl].astype(bool)
        out.append(np.where(masked, ord("N"), np.frombuffer(b"ACGT", np.uint8)[base]).astype(np.uint8).tobytes())
    return out


# ---- per-read answers of the emulation ------------------------------------------------------------------------------
_depth_lib = None


def depth_lib():
    global _depth_lib
    if _depth_lib is None:
        d = os.path.join(A.HERE, "emu_aa_big")
        subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL)
        _depth_lib = C.CDLL(os.path.join(d, "libkamd_aa_depth_emu.so"))
        _depth_lib.aa_emu_list_depth.restype = C.c_int64
    return _depth_lib


def emu_pseudoalign(index_path, seqs):
    """aa_common.emu_pseudoalign read by read: outcome and clashes as there, and sets (per read, the winner's transcript set; None: not aligned), list_len (per
    read, its longest class list), max_list_len (the longest met), win_sets (per read, the distinct index sets of the winning frame: more than one and the
    kernel writes a tuple record)"""
    from kallisto_amd.api import _View
    L, p = A.lib(), A._p
    h = C.c_void_p()
    if L.kamd_index_load(index_path.encode(), 2, C.byref(h)) != 0:
        raise RuntimeError(L.kamd_last_error().decode())
    try:
        view = _View()
        L.kamd_index_get_view(h, C.byref(view))
        words, l16, max_len = A.pack(seqs)
        n = len(seqs)
        outcome, clashes = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32)
        off = np.zeros(n + 1, np.uint64)
        cap = max(n * 64, 1024)
        ids = np.zeros(cap, np.uint32)
        r = L.aa_emu_pseudoalign(C.byref(view), p(words), p(l16), C.c_uint64(n), C.c_int32(max_len), p(outcome), p(clashes), p(off), p(ids), C.c_uint64(cap), None)
        if r < 0:
            raise RuntimeError("aa_emu_pseudoalign failed %d" % r)
        depth, wsets = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        longest = depth_lib().aa_emu_list_depth(C.byref(view), p(words), p(l16), C.c_uint64(n), C.c_int32(max_len), p(depth), p(wsets))
        if longest < 0:
            raise RuntimeError("aa_emu_list_depth failed %d" % longest)
    finally:
        L.kamd_index_free(h)
    sets = [tuple(ids[int(off[i]):int(off[i + 1])].tolist()) if outcome[i] >= 0 else None for i in range(n)]
    assert np.array_equal(wsets[:n] > 0, outcome[:n] >= 0)   # (the two emulations decide alike)
    return {"outcome": outcome[:n], "clashes": clashes[:n], "multiset": dict(collections.Counter(s for s in sets if s is not None)), "sets": sets,
            "list_len": depth[:n], "max_list_len": int(longest), "win_sets": wsets[:n]}


def expected_for(emu, order):
    """What a run over the reads emu was made from, taken in `order` (an index array, repeats allowed), must give: the EC multiset without zero counts and
    the counters of kamd_aa_stats, plus n_unique.  Exact for any tiling or permutation, and only the distinct reads were emulated."""
    outcome, clashes = emu["outcome"], emu["clashes"]
    times = np.bincount(np.asarray(order, np.int64), minlength=len(outcome))
    assert len(times) == len(outcome), "order points beyond the emulated reads"
    ms = collections.Counter()
    for i in np.flatnonzero(times):
        if outcome[i] >= 0:
            ms[emu["sets"][i]] += int(times[i])
    aligned = outcome >= 0
    return {"multiset": dict(ms), "n_processed": int(times.sum()), "n_winner": [int(times[outcome == f].sum()) for f in range(6)],
            "n_all_empty": int(times[outcome == -2].sum()), "n_rejected_offlist": int(times[outcome == -1].sum()),
            "n_frame_clashes": int((times[aligned] * clashes[aligned].astype(np.int64)).sum()),   # (clashes of aligned reads only, as test_aa_cpu sums them)
            "n_unique": sum(c for s, c in ms.items() if len(s) == 1)}


# ---- emulations, once per process ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def emulated_fixture(variant):
    fx = A.fixture()
    return emu_pseudoalign(fx[variant]["index"], fx["reads"])


@functools.lru_cache(maxsize=None)
def emulated_long(variant):
    return emu_pseudoalign(A.fixture()[variant]["index"], list(long_reads()))


@functools.lru_cache(maxsize=None)
def emulated_frames_long():
    """[(max_len, reads, words, lens)] of frame_reads_long"""
    return [(ml, reads) + A.emu_frames(reads, ml)[:2] for ml, reads in frame_reads_long()]
