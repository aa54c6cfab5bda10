"""What the tests of the barcode / UMI technologies (`bus -x <technology>`: kamd_bus_split, kamd_bus_records, kallisto_amd.bus_sc) share, and what
tests/golden/make_bus_sc.py generates its inputs with:

  * the cases of tests/golden/bus_sc (CASES) and their reads: the cDNA reads of existing fixtures, tag reads by a small deterministic generator over
    an integer LCG of its own (no numpy stream whose values could change between versions) -- no read file is committed;
  * a short Python restatement of the per-item rules (py_item), the yardstick of the per-item tests;
  * the ctypes binding of tests/emu_bustag/libkamd_bustag_emu.so (TEST INFRASTRUCTURE: kamd_bustag.h and kamd_bus.cpp compiled for the CPU);
  * the oracle's per-read transcript set of the cut sequences, the fixtures' loaders, and the rule for the BUS header's lengths."""
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
GOLD = os.path.join(common.GOLDEN, "bus_sc")
MAX_PARTS = 8
STRAND_FLAG = {0: "--unstranded", 1: "--fr-stranded", 2: "--rf-stranded"}

# name: technology string as the reference is given it, the fixture whose mate-1 reads are the cDNA and the slice of them, extra flags of the
# command line, seed of the tag generator
SEQ_WINDOW_STARTS = (1, 15, 16, 17, 33)
CASES = {
    "10xv3": dict(tech="10XV3", fixture="ref_test_pe", reads=(0, 5000), flags=[], seed=11),
    "10xv3_unstranded": dict(tech="10XV3", fixture="ref_test_pe", reads=(0, 5000), flags=["--unstranded"], seed=11),
    "surecell": dict(tech="SURECELL", fixture="yeast_se", reads=(0, 6000), flags=[], seed=12),
    "indropsv2": dict(tech="INDROPSV2", fixture="k21_pe", reads=(0, 3000), flags=[], seed=13),
    "vasa": dict(tech="VASA-SEQ", fixture="yeast_se", reads=(0, 3000), flags=[], seed=14),
    **{"seq_window_%d" % s: dict(tech="0,0,8:0,8,16:1,%d,100" % s, fixture="yeast_se", reads=(2000, 4000), flags=[], seed=15) for s in SEQ_WINDOW_STARTS},
    # (tag reads of 7 .. 44 bases: 12 .. 40 as the common ones, 41 .. 44 so that a UMI beyond 32 bases -- the truncation -- occurs, 7 .. 9 for the drops)
    "open_umi": dict(tech="0,0,8:0,8,0:1,0,0", fixture="ref_test_pe", reads=(5000, 8000), flags=[], seed=16),
    "no_umi": dict(tech="0,0,8:-1,-1,-1:1,0,0", fixture="ref_test_pe", reads=(8000, 10000), flags=[], seed=17),
    "no_bc": dict(tech="-1,-1,-1:0,0,10:1,0,0", fixture="yeast_se", reads=(3000, 6000), flags=[], seed=18),
}
DRIVER_CASES = ["10xv3", "indropsv2", "vasa"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# emu binding
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Substr(C.Structure):
    _fields_ = [("file", C.c_int32), ("start", C.c_int32), ("stop", C.c_int32)]


class Layout(C.Structure):
    _fields_ = [("n_files", C.c_int32), ("n_bc", C.c_int32), ("n_umi", C.c_int32), ("reserved", C.c_int32),
                ("bc", Substr * MAX_PARTS), ("umi", Substr * MAX_PARTS), ("seq", Substr)]

    def parts(self, which):
        a, n = (self.bc, self.n_bc) if which == "bc" else (self.umi, self.n_umi)
        return [(a[i].file, a[i].start, a[i].stop) for i in range(n)]

    def as_dict(self):
        return {"n_files": self.n_files, "bc": self.parts("bc"), "umi": self.parts("umi"), "seq": (self.seq.file, self.seq.start, self.seq.stop)}


class SplitStats(C.Structure):
    _fields_ = [("n_items", C.c_uint64), ("n_valid", C.c_uint64), ("n_dropped_umi", C.c_uint64), ("n_dropped_bc", C.c_uint64),
                ("bc_len_hist", C.c_uint64 * 33), ("umi_len_hist", C.c_uint64 * 33), ("max_seq_len", C.c_int32), ("last_ms", C.c_float)]


TAG_DTYPE = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("flags", "<u4"), ("bc_len", "<u2"), ("umi_len", "<u2")])
assert TAG_DTYPE.itemsize == 24

_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_bustag")], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(HERE, "emu_bustag", "libkamd_bustag_emu.so"))
        L.bus_emu_parse.restype = C.c_int
        L.bus_emu_parse.argtypes = [C.c_char_p, C.POINTER(Layout), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
        L.bus_emu_check.restype = C.c_int
        L.bus_emu_check.argtypes = [C.POINTER(Layout), C.c_char_p, C.c_size_t]
        L.bus_emu_seq_max_len.restype = C.c_int32
        L.bus_emu_seq_max_len.argtypes = [C.POINTER(Layout), C.c_int32]
        L.bus_emu_record_words.restype = C.c_uint64
        L.bus_emu_record_words.argtypes = [C.c_int32]
        L.bus_emu_split.restype = C.c_uint64
        L.bus_emu_split.argtypes = [C.POINTER(Layout), C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.POINTER(SplitStats)]
        _lib = L
    return _lib


def parse(tech):
    """-> (Layout, default strand) or raises ValueError with the parser's text"""
    L, strand, err = Layout(), C.c_int32(-1), C.create_string_buffer(512)
    if emu().bus_emu_parse(tech.encode(), C.byref(L), C.byref(strand), err, len(err)) != 0:
        raise ValueError(err.value.decode())
    return L, int(strand.value)


def record_words(max_len):
    return (max_len + 15) // 16 + 1 + (max_len + 31) // 32 + 1


def stats_dict(st):
    return {"n_items": int(st.n_items), "n_valid": int(st.n_valid), "n_dropped_umi": int(st.n_dropped_umi), "n_dropped_bc": int(st.n_dropped_bc),
            "bc_len_hist": [int(x) for x in st.bc_len_hist], "umi_len_hist": [int(x) for x in st.umi_len_hist], "max_seq_len": int(st.max_seq_len)}


def emu_split(L, words, lens, n_items, max_len, seq_max_len=None):
    """-> (tags [n_valid] TAG_DTYPE, src [n_valid], seq_words [n_valid * record_words(seq_max_len)], seq_len [n_valid], stats dict, seq_max_len)"""
    lib = emu()
    if seq_max_len is None:
        seq_max_len = int(lib.bus_emu_seq_max_len(C.byref(L), max_len))
    rw = record_words(seq_max_len)
    tags = np.zeros(max(n_items, 1), TAG_DTYPE)
    src = np.zeros(max(n_items, 1), np.uint32)
    sw = np.zeros(max(n_items, 1) * rw, np.uint32)
    sl = np.zeros(max(n_items, 1), np.uint16)
    st = SplitStats()
    words = np.ascontiguousarray(words, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint16)
    nv = int(lib.bus_emu_split(C.byref(L), words.ctypes.data, lens.ctypes.data, n_items, max_len, tags.ctypes.data, src.ctypes.data, sw.ctypes.data, sl.ctypes.data,
                               seq_max_len, C.byref(st)))
    return tags[:nv], src[:nv], sw[:nv * rw], sl[:nv], stats_dict(st), seq_max_len


def pack_host(seqs, max_len=None):
    """kamd_pack_reads_host of the product library (host code: no GPU needed) -> (words uint32, lens uint16, max_len)"""
    import kallisto_amd.api as A
    lib = A.load_library()
    n = len(seqs)
    ln = np.array([len(s) for s in seqs], np.int32)
    max_len = max_len or max(int(ln.max(initial=1)), 1)
    off = np.zeros(max(n, 1), np.uint64)
    if n:
        off[1:n] = np.cumsum(ln[:-1].astype(np.uint64))
    buf = b"".join(seqs) + b"\0"
    words = np.zeros(max(n, 1) * record_words(max_len), np.uint32)
    l16 = np.zeros(max(n, 1), np.uint16)
    rc = lib.kamd_pack_reads_host(buf, off.ctypes.data, ln.ctypes.data, n, max_len, words.ctypes.data, l16.ctypes.data)
    assert rc == 0, lib.kamd_last_error()
    return words[:n * record_words(max_len)], l16[:n], max_len


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the rules once more, in Python
# ---------------------------------------------------------------------------------------------------------------------------------------------------
_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("a"): 0, ord("c"): 1, ord("g"): 2, ord("t"): 3}


def py_encode(s):
    """a field's string -> (value, flag): the first 32 bases, anything but ACGT is code 2 and an N"""
    r, n_n, pos = 0, 0, 0
    for i, ch in enumerate(s[:32]):
        c = _CODE.get(ch)
        if c is None:
            c = 2
            if n_n == 0:
                pos = i
            n_n += 1
        r = (r << 2) | c
    return r, (min(n_n, 3) | (pos & 31) << 2) if n_n else 0


def _py_field(parts, reads):
    if parts[0][0] < 0:
        return None
    out = b""
    for f, a, b in parts:
        l = len(reads[f])
        n = (b - a) if b else (l - a)
        if l < a + n or n <= 0:
            return False
        out += reads[f][a:a + n]
    return out


def py_item(layout, reads):
    """layout: Layout.as_dict(); reads: the item's reads (bytes) per file -> ("umi" | "bc", None) for a dropped item, else
    ("ok", dict(barcode, umi, flags, bc_len, umi_len, seq))"""
    umi = _py_field(layout["umi"], reads)
    if umi is False:
        return "umi", None
    bc = _py_field(layout["bc"], reads)
    if bc is False:
        return "bc", None
    b, fb = (0, 0) if bc is None else py_encode(bc)
    u, fu = (2 ** 64 - 1, fb) if umi is None else py_encode(umi)   # (absent UMI: the flag repeats the barcode's, see kamd_bustag.h)
    f, a, e = layout["seq"]
    r = reads[f]
    seq = r[a:(min(e, len(r)) if e else len(r))] if len(r) > a else b""
    return "ok", dict(barcode=b, umi=u, flags=fb | fu << 8, bc_len=16 if bc is None else len(bc), umi_len=1 if umi is None else len(umi), seq=seq)


def py_split(layout, items):
    """items: list of per-file read tuples -> (list of (input item, dict) of the survivors, stats dict without max_seq_len's device detail)"""
    st = {"n_items": len(items), "n_valid": 0, "n_dropped_umi": 0, "n_dropped_bc": 0, "bc_len_hist": [0] * 33, "umi_len_hist": [0] * 33, "max_seq_len": 0}
    out = []
    for i, reads in enumerate(items):
        if layout["umi"][0][0] >= 0:   # the UMI bin comes before the barcode is looked at
            u = _py_field(layout["umi"], reads)
            if u is not False and len(u) <= 32:
                st["umi_len_hist"][len(u)] += 1
        else:                          # (no UMI: length 1, and also before the barcode is looked at)
            st["umi_len_hist"][1] += 1
        what, d = py_item(layout, reads)
        if what != "ok":
            st["n_dropped_" + what] += 1
            continue
        if d["bc_len"] <= 32:
            st["bc_len_hist"][d["bc_len"]] += 1
        st["n_valid"] += 1
        st["max_seq_len"] = max(st["max_seq_len"], len(d["seq"]))
        out.append((i, d))
    return out, st


def header_lens(layout, stats):
    """the BUS header's (bclen, umilen): the layout's fixed sums, or where a part is open-ended or the field absent the modes of the length histograms
    (the first of equal bins, src/main.cpp:2472-2496)"""
    out = []
    for parts, hist in ((layout["bc"], stats["bc_len_hist"]), (layout["umi"], stats["umi_len_hist"])):
        if parts[0][0] >= 0 and parts[0][1] >= 0 and all(b != 0 for _, _, b in parts):
            out.append(sum(b - a for _, a, b in parts))
        else:
            out.append(int(np.argmax(np.asarray(hist))))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the reads of a case
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def lcg(seed):
    x = seed & (2 ** 64 - 1)
    while True:
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        yield x >> 33


CORNERS = ["plain", "n1", "n2", "n3", "n5", "n_first", "n_last", "n_umi_first", "n_umi_last", "n_both", "lower", "short_bc", "short_umi", "exact"]
CORNER_PERIOD = 37   # corners 1 .. 13 on reads i % 37 == 1 .. 13: 2 of 37 reads (5.4 %) are short enough to be dropped


def gen_tags(layout, n, seed):
    """tag reads for `n` read sets of the layout (its dict) -> (list of bytes, list of corner names).  Barcodes from a pool of 50, UMIs from a pool
    of 120, so (barcode, UMI) pairs repeat; the bases between and behind the parts are random; on top of that the corners of CORNERS.  A corner
    that needs a field the layout lacks falls on the other field, or is a plain read."""
    rnd = lcg(seed)
    nxt = lambda m: next(rnd) % m
    rs = lambda k: bytearray(b"ACGT"[nxt(4)] for _ in range(k))
    bc_parts = [p for p in layout["bc"] if p[0] >= 0]
    umi_parts = [p for p in layout["umi"] if p[0] >= 0]
    open_umi = any(b == 0 for _, _, b in umi_parts)
    bc_pos = [i for _, a, b in bc_parts for i in range(a, b)]
    umi_pos = [] if open_umi else [i for _, a, b in umi_parts for i in range(a, b)]
    bc_end = max([b for _, _, b in bc_parts], default=0)
    umi_end = max([b for _, _, b in umi_parts], default=0)
    umi_start = umi_parts[0][1] if umi_parts else 0
    fixed_end = max(bc_end, umi_end)
    pool = [rs(len(bc_pos)) for _ in range(50)]
    upool = [rs(40 if open_umi else len(umi_pos)) for _ in range(120)]
    tags, names = [], []
    for i in range(n):
        c = i % CORNER_PERIOD
        name = CORNERS[c] if c < len(CORNERS) else "plain"
        if open_umi:   # half of the reads carry a UMI of 12 (the mode); the rest 4 .. 36
            length = umi_start + (12 if nxt(2) else 4 + nxt(33))
        else:
            length = fixed_end + 2
        t = rs(length)
        b, u = pool[nxt(50)], upool[nxt(120)]
        for k, p in enumerate(bc_pos):
            t[p] = b[k]
        if open_umi:
            t[umi_start:] = u[:length - umi_start]
            upos = list(range(umi_start, length))
        else:
            for k, p in enumerate(umi_pos):
                t[p] = u[k]
            upos = umi_pos
        first, second = (bc_pos, upos) if bc_pos else (upos, bc_pos)   # "the barcode", or the only field there is
        other = second if second else first

        def put_n(pos_list, k):
            for p in sorted(set(pos_list[nxt(len(pos_list))] for _ in range(8 * k)))[:k]:
                t[p] = ord("N")
        if name == "n1":
            put_n(first, 1)
        elif name == "n2":
            put_n(first, 2)
        elif name == "n3":
            put_n(other, 3)
        elif name == "n5":
            put_n(first, 5)
        elif name == "n_first":
            t[first[0]] = ord("N")
        elif name == "n_last":
            t[first[-1]] = ord("n")   # (lower case: an N all the same)
        elif name == "n_umi_first":
            t[other[0]] = ord("N")
        elif name == "n_umi_last":
            t[other[-1]] = ord("N")
        elif name == "n_both":
            put_n(first, 1)
            put_n(other, 1)
        elif name == "lower":
            t = bytearray(bytes(t).lower())
        elif name == "short_bc":
            t = t[:(bc_end if bc_end else umi_end) - 1]
        elif name == "short_umi":
            t = t[:(umi_start if open_umi else (umi_end if umi_end else bc_end) - 1)]
        elif name == "exact":
            t = t[:(umi_start + 1 if open_umi else fixed_end)]
        tags.append(bytes(t))
        names.append(name)
    return tags, names


@functools.lru_cache(maxsize=None)
def case_reads(name):
    """-> (Layout, default strand, list of per-file read tuples, corner names).  Two files: the tag read in the file the barcode names (or the UMI),
    the cDNA read in the other.  One file (VASA-SEQ): tag and cDNA in one read; the short corners are the whole read."""
    c = CASES[name]
    L, strand = parse(c["tech"])
    lay = L.as_dict()
    _, _, r1, r2 = common.load_case(c["fixture"])
    a, b = c["reads"]
    cdna = r1[a:b]
    tags, names = gen_tags(lay, len(cdna), c["seed"])
    if lay["n_files"] == 1:
        cut = lay["seq"][1]
        # (a tag cut short is a short read without cDNA; "exact" ends where the cDNA would begin: an empty sequence)
        items = [((t[:cut] + s,) if n not in ("short_bc", "short_umi", "exact") else (t[:cut],)) for (t, s, n) in zip(tags, cdna, names)]
    else:
        sf = lay["seq"][0]
        items = [((s, t) if sf == 0 else (t, s)) for t, s in zip(tags, cdna)]
    return L, strand, items, names


def case_strand(name):
    c = CASES[name]
    _, strand = parse(c["tech"])
    for s, f in STRAND_FLAG.items():
        if f in c["flags"]:
            strand = s
    return strand


def case_batch(name):
    """the case's items packed as one batch at a common max_len -> (words, lens, n_items, max_len)"""
    L, _, items, _ = case_reads(name)
    flat = [r for it in items for r in it]
    w, l, max_len = pack_host(flat)
    return w, l, len(items), max_len


def load_golden(name):
    d = os.path.join(GOLD, name)
    meta = json.load(open(os.path.join(d, "case.json")))
    lines = []
    with gzip.open(os.path.join(d, "expected.txt.gz"), "rt") as f:
        for l in f:
            fl, bc, umi, s = l.rstrip("\n").split("\t")
            lines.append((int(fl), int(bc), int(umi), tuple(int(x) for x in s.split(","))))
    return meta, lines


def golden_cases():
    """the cases that have a fixture (a case the reference could not run is recorded in tests/golden/bus_sc/dropped.json and has none)"""
    return [n for n in CASES if os.path.exists(os.path.join(GOLD, n, "expected.txt.gz"))]


def oracle_opts(strand, no_jump=0, union=0):
    """what `bus` runs single-end reads with: no positional filter (single_overhang), partial matches"""
    from oracle import oracle as O
    return O.Opts(0, 200.0, 20.0, 1, strand, no_jump, union)


@functools.lru_cache(maxsize=None)
def oracle_sets(name):
    """the oracle's transcript set of the cut sequence of every surviving item of a case: tuple of (input item, tuple of ids); () = not pseudoaligned"""
    from oracle import oracle as O
    c = CASES[name]
    L, _, items, _ = case_reads(name)
    surv, _ = py_split(L.as_dict(), items)
    _, idx, _, _ = common.load_case(c["fixture"])
    ix = O.Index(idx)
    opts = oracle_opts(case_strand(name))
    out = []
    for i, d in surv:
        s = ix.pseudoalign(opts, d["seq"], None, mean_fl=200.0, has_mean_fl=True)[0] if len(d["seq"]) else []
        out.append((i, tuple(s)))
    ix.close()
    return tuple(out)
