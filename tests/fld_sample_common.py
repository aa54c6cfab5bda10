"""Inputs and expectations of the fragment-length sample's tests (test_fld_sample_cpu.py, test_gpu_fld_sample.py).  No GPU here.

The sample is the first 10 000 qualifying pairs of the input in input order (src/ProcessReads.cpp:981-1017, oracle/kallisto_oracle.c
`tlencount < 10000`): a pair qualifies when exactly one transcript remains, both mates hit and 0 < tl < 1000.  While the sample is
being estimated no pair's result depends on another pair, so what the oracle says about each pair of ONE tile of a fixture
(pair_flags) gives the expectation of any input put together from slices of that tile and junk pairs (expected_flens) -- inputs of
millions of pairs, far beyond what the oracle would walk in a test's time.  test_fld_sample_cpu.py holds that shortcut against the
oracle's own process_reads on inputs it can walk.

An input is an Input: a list of segments, each `times` copies of the tile's pairs [a, b) or of junk pairs (both mates all N: no
k-mer, never pseudoaligned).  The same list yields the reads the oracle walks (reads), the per-item index into the tile's flags
(order) and the packed records on the device (device: slices of one packed tile, Tensor.repeat and one cat -- records have a fixed
size, so a concatenation of records is a valid input; nothing beyond one tile is packed on the host)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import common

WANT = 10000            # pairs in the sample
RANK_PER_THREAD, RANK_PER_WAVE, RANK_PER_BLOCK = 8, 512, 8192   # items per thread / wavefront / block of k_fld_count, k_fld_emit
FIRST_CHUNK = 1048576   # items of the first prefix kamd_fld_from_batch looks at (kamd_tuning.fld_first_chunk's default)
STRANDS = {"pe": 0, "pe_fr": 1, "pe_rf": 2}

_cases, _indices, _flags = {}, {}, {}


def case_reads(case):
    """(index path, r1, r2) of a fixture, loaded once"""
    if case not in _cases:
        _, idx_path, r1, r2 = common.load_case(case)
        _cases[case] = (idx_path, r1, r2)
    return _cases[case]


def oracle_index(case):
    from oracle import oracle as O
    if case not in _indices:
        _indices[case] = O.Index(case_reads(case)[0])
    return _indices[case]


def oracle_opts(strand=0, single_overhang=0, no_jump=0, union=0):
    from oracle import oracle as O
    return O.Opts(1, 0.0, 0.0, single_overhang, strand, no_jump, union)


def pair_flags(case, strand=0, single_overhang=0, no_jump=0, union=0):
    """per pair of the fixture: (qualifies, tl) by the oracle's per-pair entry points -- the condition of ko_process_reads, pair by pair"""
    key = (case, strand, single_overhang, no_jump, union)
    if key not in _flags:
        ix = oracle_index(case)
        opts = oracle_opts(strand, single_overhang, no_jump, union)
        _, r1, r2 = case_reads(case)
        q = np.zeros(len(r1), bool)
        tls = np.full(len(r1), -1, np.int64)
        for i, (a, b) in enumerate(zip(r1, r2)):
            u, n1, n2 = ix.pseudoalign(opts, a, b)
            if len(u) == 1 and n1 > 0 and n2 > 0:
                tl = ix.map_pair(a, b)
                if 0 < tl < common.MAX_FRAG_LEN:
                    q[i], tls[i] = True, tl
        q.setflags(write=False); tls.setflags(write=False)
        _flags[key] = (q, tls)
    return _flags[key]


def expected_flens(flags, tls, order, start_used=0):
    """"the first 10 000 qualifying pairs in input order", restated: `order` holds per item of the input its pair in the tile (-1 = junk);
    -> (flens histogram of the pairs this input adds to a sample that already holds start_used, used afterwards)"""
    order = np.asarray(order, np.int64)
    real = order >= 0
    q = np.zeros(len(order), bool)
    q[real] = flags[order[real]]
    take = np.flatnonzero(q)[:max(0, WANT - start_used)]
    flens = np.bincount(tls[order[take]], minlength=common.MAX_FRAG_LEN).astype(np.uint32)
    assert len(flens) == common.MAX_FRAG_LEN
    return flens, start_used + len(take)


def qualifying_positions(flags, order):
    """items of the input that qualify, ascending"""
    order = np.asarray(order, np.int64)
    q = np.zeros(len(order), bool)
    q[order >= 0] = flags[order[order >= 0]]
    return np.flatnonzero(q)


@dataclass
class Input:
    case: str
    segments: list = field(default_factory=list)   # ("tile", a, b, times) | ("junk", 0, count, 1)

    @property
    def n_items(self):
        return sum((b - a) * t for _, a, b, t in self.segments)

    def order(self):
        parts = [np.tile(np.arange(a, b, dtype=np.int64), t) if kind == "tile" else np.full((b - a) * t, -1, np.int64) for kind, a, b, t in self.segments]
        return np.concatenate(parts) if parts else np.zeros(0, np.int64)

    def prefix(self, n):
        """the first n items of this input"""
        assert 0 <= n <= self.n_items
        out, left = [], n
        for kind, a, b, t in self.segments:
            per = b - a
            whole = min(t, left // per) if per else 0
            if whole:
                out.append((kind, a, b, whole)); left -= whole * per
            if whole < t and left:
                out.append((kind, a, a + left, 1)); left = 0
            if not left:
                break
        res = Input(self.case, out)
        assert res.n_items == n
        return res

    def window(self, lo, hi):
        """items [lo, hi) of this input"""
        o = self.order()[lo:hi]
        # (runs of consecutive pairs of the tile / of junk: what a ragged batch of the same reads is)
        segs, i = [], 0
        while i < len(o):
            j = i + 1
            if o[i] < 0:
                while j < len(o) and o[j] < 0:
                    j += 1
                segs.append(("junk", 0, j - i, 1))
            else:
                while j < len(o) and o[j] == o[j - 1] + 1:
                    j += 1
                segs.append(("tile", int(o[i]), int(o[i]) + j - i, 1))
            i = j
        return Input(self.case, segs)

    def junk_read(self):
        _, r1, r2 = case_reads(self.case)
        return b"N" * len(r1[0]), b"N" * len(r2[0])

    def reads(self):
        """the interleaved reads, for the oracle (only for inputs small enough to walk)"""
        _, r1, r2 = case_reads(self.case)
        j1, j2 = self.junk_read()
        out = []
        for kind, a, b, t in self.segments:
            one = [x for p in zip(r1[a:b], r2[a:b]) for x in p] if kind == "tile" else [j1, j2] * (b - a)
            out.extend(one * t)
        return out

    def device(self, ka, ctx, max_len=None):
        """(words, lens, n_items, max_len) on the device: one tile and one junk pair packed by the host packer, the rest by slicing,
        Tensor.repeat and cat"""
        import torch
        _, r1, r2 = case_reads(self.case)
        max_len = max_len or max(max(map(len, r1)), max(map(len, r2)))
        key = (self.case, max_len, id(ctx))
        if key not in _packed:
            words, lens, ml = ctx.pack_reads_host(common.interleave(r1, r2), max_len)
            jw, jl, _ = ctx.pack_reads_host(list(self.junk_read()), max_len)
            assert ml == max_len
            _packed[key] = (words, lens, jw, jl)
        words, lens, jw, jl = _packed[key]
        rec = 2 * ka.packed_record_words(max_len)   # words per pair
        assert words.numel() == len(r1) * rec and jw.numel() == rec
        ws, ls = [], []
        for kind, a, b, t in self.segments:
            if kind == "tile":
                ws.append(words[a * rec:b * rec].repeat(t)); ls.append(lens[2 * a:2 * b].repeat(t))
            else:
                ws.append(jw.repeat((b - a) * t)); ls.append(jl.repeat((b - a) * t))
        if not ws:
            return words[:0].clone(), lens[:0].clone(), 0, max_len
        return torch.cat(ws), torch.cat(ls), self.n_items, max_len


_packed = {}


def forget_packed(ctx):
    """drop the packed tiles of a context that is being closed"""
    for k in [k for k in _packed if k[2] == id(ctx)]:
        del _packed[k]


# ---- the named inputs ---------------------------------------------------------------------------------------------------------------

def tiled(case, tiles):
    n = len(case_reads(case)[1])
    return Input(case, [("tile", 0, n, tiles)])


JUNK_AT = 4321   # cut_at puts its junk pairs inside the first tile, not at a block boundary


def cut_at(item, strand=0):
    """two tiles of ref_test_pe with as many junk pairs inserted behind pair JUNK_AT as it takes for the 10 000th qualifying pair to be
    exactly item `item` of the input"""
    q, _ = pair_flags("ref_test_pe", strand)
    plain = tiled("ref_test_pe", 2)
    natural = int(qualifying_positions(q, plain.order())[WANT - 1])
    assert item >= natural and natural > JUNK_AT, (item, natural)
    n = len(q)
    return Input("ref_test_pe", [("tile", 0, JUNK_AT, 1), ("junk", 0, item - natural, 1), ("tile", JUNK_AT, n, 1), ("tile", 0, n, 1)])


def prefix_with(n_qualifying, strand=0):
    """the shortest prefix of tiled ref_test_pe that holds exactly n_qualifying qualifying pairs: its last item is the n_qualifying-th"""
    q, _ = pair_flags("ref_test_pe", strand)
    per_tile = int(q.sum())
    tiles = n_qualifying // per_tile + 1
    full = tiled("ref_test_pe", tiles)
    pos = qualifying_positions(q, full.order())
    return full.prefix(int(pos[n_qualifying - 1]) + 1)


def dense_sparse_dense():
    """ref_test_pe[:8192] (dense), 70 000 junk pairs (nothing), one whole tile (dense): with a first prefix of 8192 items the second
    prefix finds nothing and the third is sized from a rate that the second has diluted"""
    n = len(case_reads("ref_test_pe")[1])
    return Input("ref_test_pe", [("tile", 0, RANK_PER_BLOCK, 1), ("junk", 0, 70000, 1), ("tile", 0, n, 1)])


def prefixes_that_run(n_items, qualifying_pos, first_chunk=FIRST_CHUNK, start_used=0):
    """kamd_fld_from_batch's loop over prefixes, restated from its documentation (the first prefix has first_chunk items, the next ones
    1.5 x what the rate so far asks for, between 65 536 and 2 097 152 items): -> list of (first item, items) per prefix"""
    out, done, found = [], 0, start_used
    chunk = first_chunk
    pos = np.asarray(qualifying_pos)
    while done < n_items and found < WANT:
        n = min(chunk, n_items - done)
        out.append((done, n))
        found = min(WANT, found + int(np.count_nonzero((pos >= done) & (pos < done + n))))
        done += n
        rate = max((found - start_used) / done, 1e-4)
        chunk = min(max(int((WANT - min(found, WANT)) / rate * 1.5), 65536), 2097152)
    return out
