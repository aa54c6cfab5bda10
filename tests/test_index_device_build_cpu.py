"""The device builder of the k-mer table (kamd_index_load_deferred + kamd_index_upload, kallisto_amd/csrc/kamd_ixbuild.hip) without a GPU:
its per-item steps (kamd_ixbuild.h) are driven serially by tests/emu_ixbuild -- count, scan, place, order, fill -- and must give, byte for
byte, the tables the host builder produces with ONE thread (the keys of a home bucket in ascending text position).  The driver makes the
order awkward on purpose: the scan combines its maps over chunks of 7 buckets, the placement runs over the items in reversed order.

The fixtures never reach the growth of a compact table nor its fall-back to the wide one, so the shared geometry functions and the scan are
also checked on synthetic histograms against a brute-force serial loop and against the rules restated here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kallisto_amd.api import _View
from tests import common

HERE = os.path.dirname(os.path.abspath(__file__))
WIDE, COMPACT, AUTO = 0, 1, 2
LAYOUTS = [("wide", WIDE, 0.0), ("auto", AUTO, 0.0), ("compact09", COMPACT, 0.9)]


class _Out(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in ("n_buckets", "pad_buckets", "n_dbuckets", "dpad_buckets", "dummy_slot")] +
                [(n, C.c_uint32) for n in ("layout", "slots", "tag_q", "tag_dsh", "tag_w", "dummy_uec", "dummy_strand")] +
                [("rounds", C.c_int32), ("table", C.c_void_p), ("slot_block", C.c_void_p), ("slot_dist", C.c_void_p), ("dtable", C.c_void_p)])


@pytest.fixture(scope="module")
def L():
    d = os.path.join(HERE, "emu_ixbuild")
    subprocess.check_call(["make", "-C", d], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(d, "libkamd_ixbuild_emu.so"))
    lib.kamd_last_error.restype = C.c_char_p
    lib.kamd_index_load_layout.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]
    lib.kamd_index_load_deferred.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]
    lib.kamd_index_get_view.argtypes = [C.c_void_p, C.POINTER(_View)]
    lib.kamd_index_save.argtypes = [C.c_void_p, C.c_char_p]
    lib.kamd_index_free.argtypes = [C.c_void_p]
    lib.ixb_emu_build.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(_Out)]
    lib.ixb_emu_free.argtypes = [C.POINTER(_Out)]
    lib.ixb_emu_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.ixb_emu_geo_new.restype = C.c_void_p
    lib.ixb_emu_geo_new.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_double, C.POINTER(C.c_int), C.c_void_p]
    lib.ixb_emu_geo_fit.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.ixb_emu_geo_after_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.ixb_emu_geo_free.argtypes = [C.c_void_p]
    lib.ixb_emu_total_buckets.restype = C.c_uint64
    lib.ixb_emu_total_buckets.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    return lib


def _arr(ptr, n, dtype):
    if not ptr or n == 0:
        return np.zeros(0, dtype)
    return np.frombuffer((C.c_char * (int(n) * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype, count=int(n)).copy()


def _load(L, fn, path, threads, layout, load):
    h = C.c_void_p()
    rc = fn(path.encode(), threads, layout, load, C.byref(h))
    assert rc == 0, L.kamd_last_error()
    v = _View()
    assert L.kamd_index_get_view(h, C.byref(v)) == 0
    return h, v


_POINTERS = {"uec_ec": ("n_uec", np.uint32), "ec_off": (lambda v: v.n_ecs + 1, np.uint64), "ec_ids": ("ec_nnz", np.uint32),
             "unitig_blk_off": (lambda v: v.n_unitigs + 1, np.uint64), "unitig_len": ("n_unitigs", np.uint32), "blk_unitig": ("n_blocks", np.uint32),
             "blk_lb": ("n_blocks", np.uint32), "blk_ub": ("n_blocks", np.uint32), "blk_ec": ("n_blocks", np.uint32),
             "blk_pos_off": (lambda v: v.n_blocks + 1, np.uint64), "target_lens": (lambda v: v.n_targets + v.dlist_size, np.int32),
             "onlist_bits": ("onlist_words", np.uint32), "utext": ("utext_words", np.uint32), "unitig_gpos": (lambda v: v.n_unitigs + 1, np.uint64)}


@pytest.mark.parametrize("lname,layout,load", LAYOUTS, ids=[x[0] for x in LAYOUTS])
@pytest.mark.parametrize("case", common.CASES)
def test_device_steps_equal_the_one_thread_host_table(case, lname, layout, load, L, tmp_path):
    path = common.load_case(case)[1]
    hh, hv = _load(L, L.kamd_index_load_layout, path, 1, layout, load)
    dh, dv = _load(L, L.kamd_index_load_deferred, path, 2, layout, load)
    try:
        # the deferred view: no tables, everything else as the host loader gives it
        assert not dv.table and not dv.slot_block and not dv.slot_dist and not dv.dtable
        assert dv.n_buckets == 0 and dv.pad_buckets == 0 and dv.n_dbuckets == 0
        for n in ("k", "n_kmers", "n_unitigs", "n_blocks", "n_uec", "n_ecs", "ec_nnz", "n_targets", "dlist_size", "onlist_words", "utext_words", "text_bases"):
            assert getattr(dv, n) == getattr(hv, n), n
        for n, (cnt, dt) in _POINTERS.items():
            c_h = cnt(hv) if callable(cnt) else getattr(hv, cnt)
            assert np.array_equal(_arr(getattr(dv, n), c_h, dt), _arr(getattr(hv, n), c_h, dt)), n
        npos = int(_arr(hv.blk_pos_off, hv.n_blocks + 1, np.uint64)[-1])
        assert np.array_equal(_arr(dv.blk_posw, npos, np.uint32), _arr(hv.blk_posw, npos, np.uint32))
        assert np.array_equal(_arr(dv.blk_sense, npos, np.uint8), _arr(hv.blk_sense, npos, np.uint8))
        # kamd_index_save refuses an index without tables, with a message
        assert L.kamd_index_save(dh, str(tmp_path / "x.kamd").encode()) == -1 and b"kamd_index_save" in L.kamd_last_error()
        o = _Out()
        assert L.ixb_emu_build(dh, 7, 1, C.byref(o)) == 0
        try:
            # geometry
            assert (o.n_buckets, o.pad_buckets, o.layout, o.slots, o.tag_q, o.tag_dsh, o.tag_w) == \
                   (hv.n_buckets, hv.pad_buckets, hv.table_layout, hv.slots_per_bucket, hv.tag_q, hv.tag_dsh, hv.tag_w)
            assert (o.n_dbuckets, o.dpad_buckets, o.dummy_slot, o.dummy_uec, o.dummy_strand) == (hv.n_dbuckets, hv.dpad_buckets, hv.dummy_slot, hv.dummy_uec, hv.dummy_strand)
            assert o.rounds == 1   # (the fixtures never grow the table: see the synthetic tests below)
            lines = hv.n_buckets + hv.pad_buckets
            slots = lines * hv.slots_per_bucket
            assert _arr(o.table, lines * 8, np.uint64).tobytes() == _arr(hv.table, lines * 8, np.uint64).tobytes()
            assert _arr(o.slot_block, slots, np.uint32).tobytes() == _arr(hv.slot_block, slots, np.uint32).tobytes()
            assert _arr(o.slot_dist, slots, np.uint32).tobytes() == _arr(hv.slot_dist, slots, np.uint32).tobytes()
            dl = (hv.n_dbuckets + hv.dpad_buckets) * 8
            assert (case == "dlist_pe") == (dl > 0)
            assert _arr(o.dtable, dl, np.uint64).tobytes() == _arr(hv.dtable, dl, np.uint64).tobytes()
        finally:
            L.ixb_emu_free(C.byref(o))
    finally:
        L.kamd_index_free(hh)
        L.kamd_index_free(dh)


def test_placement_order_does_not_matter(L):
    """forward and reversed placement, chunks of 7 and of 1000 buckets: the same bytes"""
    path = common.load_case("yeast_se")[1]
    dh, dv = _load(L, L.kamd_index_load_deferred, path, 2, COMPACT, 0.9)
    try:
        got = []
        for chunk, rev in ((7, 1), (1000, 0)):
            o = _Out()
            assert L.ixb_emu_build(dh, chunk, rev, C.byref(o)) == 0
            lines = o.n_buckets + o.pad_buckets
            got.append((_arr(o.table, lines * 8, np.uint64).tobytes(), _arr(o.slot_block, lines * o.slots, np.uint32).tobytes()))
            L.ixb_emu_free(C.byref(o))
        assert got[0] == got[1]
    finally:
        L.kamd_index_free(dh)


def test_flattened_file_loads_as_today(L, tmp_path):
    """a .kamd file holds its tables: kamd_index_load_deferred loads it like kamd_index_load_layout does"""
    path = common.load_case("dlist_pe")[1]
    hh, hv = _load(L, L.kamd_index_load_layout, path, 1, COMPACT, 0.0)
    flat = str(tmp_path / "i.kamd")
    assert L.kamd_index_save(hh, flat.encode()) == 0
    fh, fv = _load(L, L.kamd_index_load_deferred, flat, 2, AUTO, 0.0)
    try:
        assert fv.table and fv.slot_block and fv.slot_dist and fv.dtable and fv.n_buckets == hv.n_buckets
        lines = hv.n_buckets + hv.pad_buckets
        assert _arr(fv.table, lines * 8, np.uint64).tobytes() == _arr(hv.table, lines * 8, np.uint64).tobytes()
        assert L.kamd_index_save(fh, str(tmp_path / "again.kamd").encode()) == 0
    finally:
        L.kamd_index_free(hh)
        L.kamd_index_free(fh)


# ---- the scan against a brute-force loop ------------------------------------------------------------------------------------------------
def _serial(fill, S):
    """the host builder's loop"""
    base = np.zeros(len(fill), np.uint64)
    cursor = 0
    max_disp = 0
    for b, n in enumerate(fill.tolist()):
        cursor = max(cursor, b * S)
        base[b] = cursor
        cursor += n
        if n:
            max_disp = max(max_disp, (cursor - 1) // S - b)
    return base, cursor, max_disp


def _histograms():
    rng = np.random.default_rng(5)
    out = []
    for nb, S, lam in ((16, 3, 1.5), (17, 4, 3.6), (1000, 4, 3.6), (4099, 3, 1.5), (2048, 4, 2.0), (50, 4, 0.0), (333, 3, 3.5)):
        out.append((rng.poisson(lam, nb).astype(np.uint32), S))
    for nb, S, at, heavy in ((500, 4, 0, 40), (500, 4, 123, 300), (700, 3, 699, 250), (2000, 4, 1000, 900), (64, 4, 63, 100)):
        f = rng.poisson(2.0, nb).astype(np.uint32)
        f[at] = heavy                      # hundreds of keys in one bucket: displacements beyond 6 and 14
        out.append((f, S))
    f = np.zeros(300, np.uint32); f[0] = 1200   # everything spills past the last home bucket
    out.append((f, 4))
    return out


@pytest.mark.parametrize("chunk", [1, 7, 64, 5000])
def test_scan_equals_the_serial_loop(chunk, L):
    seen_disp = set()
    for fill, S in _histograms():
        base = np.zeros(len(fill), np.uint64)
        end, md = C.c_uint64(0), C.c_uint64(0)
        assert L.ixb_emu_scan(fill.ctypes.data_as(C.c_void_p), len(fill), S, chunk, base.ctypes.data_as(C.c_void_p), C.byref(end), C.byref(md)) == 0
        want_base, want_end, want_md = _serial(fill, S)
        assert np.array_equal(base, want_base) and end.value == want_end and md.value == want_md
        seen_disp.add(want_md)
    assert any(d > 14 for d in seen_disp) and any(6 < d <= 14 for d in seen_disp) and any(d <= 6 for d in seen_disp)


# ---- the geometry decisions against the rules -----------------------------------------------------------------------------------------------
def _bits(n):
    return int(n).bit_length()


def _shifts(k, nb, n_uec, text_bases):
    span = ((1 << 32) + nb - 1) // nb
    q = (span - 1).bit_length()
    dsh = q + max(0, 2 * k - 32)
    w = dsh + (4 if dsh + 4 + _bits(n_uec) <= 64 else 3)
    return q, dsh, w, (w + _bits(n_uec) <= 64 and text_bases <= 0x3FFFFFFF)


def _geo(L, k, n_kmers, want, load):
    ok = C.c_int(0)
    o = np.zeros(7, np.uint64)
    h = L.ixb_emu_geo_new(k, n_kmers, want, load, C.byref(ok), o.ctypes.data_as(C.c_void_p))
    return h, ok.value, [int(x) for x in o]


def test_initial_table_size(L, monkeypatch):
    monkeypatch.delenv("KAMD_TABLE_KNEE_GB", raising=False)
    for n_kmers, want, load, nb in (
            (1325, WIDE, 0.0, (1325 * 2 + 2) // 3), (5, WIDE, 0.0, 16), (5, COMPACT, 0.0, 16),
            (1325, COMPACT, 0.9, int(1325 / 0.9 / 4) + 1), (1325, AUTO, 0.0, int(1325 / 0.4 / 4) + 1), (1325, AUTO, 0.95, int(1325 / 0.4 / 4) + 1),
            (56_800_000, AUTO, 0.0, int(56_800_000 / 0.4 / 4) + 1),      # 16 B x 56.8 M / 0.4 = 2.27 GB: under the 2.4 GB knee
            (70_000_000, AUTO, 0.0, int(70_000_000 / 0.5 / 4) + 1),      # 2.8 GB at 0.4, 2.24 GB at 0.5
            (130_600_000, AUTO, 0.0, int(130_600_000 / 0.6 / 4) + 1)):   # beyond the knee at either: 0.6
        h, ok, g = _geo(L, 31, n_kmers, want, load)
        L.ixb_emu_geo_free(h)
        assert ok == 1 and g[2] == nb and g[0] == (want != WIDE) and g[1] == (4 if want != WIDE else 3) and g[6] == max(16, (n_kmers * 2 + 2) // 3), (n_kmers, want, load, g)
    monkeypatch.setenv("KAMD_TABLE_KNEE_GB", "8")
    h, ok, g = _geo(L, 31, 130_600_000, AUTO, 0.0)
    L.ixb_emu_geo_free(h)
    assert g[2] == int(130_600_000 / 0.4 / 4) + 1
    monkeypatch.delenv("KAMD_TABLE_KNEE_GB")
    h, ok, g = _geo(L, 31, 6_100_000_000, WIDE, 0.0)   # bucket numbers are 32 bits wide
    L.ixb_emu_geo_free(h)
    assert ok == 0


def test_compact_falls_back_to_wide_or_fails(L):
    o = np.zeros(7, np.uint64)
    p = o.ctypes.data_as(C.c_void_p)
    for n_uec, text_bases in ((1 << 29, 10_000), (100, 0x40000000)):      # class ids too wide beside a k = 31 tag; text positions beyond 30 bits
        assert not _shifts(31, int(1_000_000 / 0.4 / 4) + 1, n_uec, text_bases)[3]
        h, ok, g = _geo(L, 31, 1_000_000, AUTO, 0.0)
        assert L.ixb_emu_geo_fit(h, n_uec, text_bases, p) == 1            # recount: the wide table
        assert [int(x) for x in o[:3]] == [0, 3, (2_000_000 + 2) // 3]
        assert L.ixb_emu_geo_fit(h, n_uec, text_bases, p) == 0 and L.ixb_emu_geo_after_scan(h, 1000, p) == 0   # the wide table takes any displacement
        L.ixb_emu_geo_free(h)
        h, ok, g = _geo(L, 31, 1_000_000, COMPACT, 0.0)
        assert L.ixb_emu_geo_fit(h, n_uec, text_bases, p) == -1           # asked for by name: an error
        L.ixb_emu_geo_free(h)
    h, ok, g = _geo(L, 31, 1_000_000, AUTO, 0.0)
    assert L.ixb_emu_geo_fit(h, 100, 0x3FFFFFFF, p) == 0 and int(o[0]) == 1
    q, dsh, w, fits = _shifts(31, g[2], 100, 0x3FFFFFFF)
    assert fits and [int(x) for x in o[3:6]] == [q, dsh, w]
    L.ixb_emu_geo_free(h)


# (k, class ids, k-mers) at which the compact slot has room for a four-bit displacement (the first and third) or only for three bits
@pytest.mark.parametrize("k,n_uec,n_kmers", [(31, 1000, 600_000), (25, 1 << 20, 6000), (7, 50, 6000), (21, 1 << 29, 12_000)])
def test_compact_table_grows_while_a_key_lies_too_far(k, n_uec, n_kmers, L):
    """the growth step, driven by the scan's max_disp on histograms with a heavy bucket, against the rule restated here"""
    o = np.zeros(7, np.uint64)
    p = o.ctypes.data_as(C.c_void_p)
    rng = np.random.default_rng(k)
    grown = 0
    limits = set()
    for heavy in (10, 30, 70, 400):
        h, ok, g = _geo(L, k, n_kmers, COMPACT, 0.9)
        nb = g[2]
        for _ in range(6):
            assert L.ixb_emu_geo_fit(h, n_uec, 100_000, p) == 0
            q, dsh, w, fits = _shifts(k, nb, n_uec, 100_000)
            assert fits and [int(x) for x in o[2:6]] == [nb, q, dsh, w]
            fill = rng.multinomial(n_kmers - heavy, np.full(nb, 1.0 / nb)).astype(np.uint32)
            fill[nb // 2] += heavy
            base = np.zeros(nb, np.uint64)
            end, md = C.c_uint64(0), C.c_uint64(0)
            assert L.ixb_emu_scan(fill.ctypes.data_as(C.c_void_p), nb, 4, 7, base.ctypes.data_as(C.c_void_p), C.byref(end), C.byref(md)) == 0
            assert md.value == _serial(fill, 4)[2]
            limit = (1 << (w - dsh)) - 2      # 14 or 6 buckets: all ones marks an empty slot
            limits.add(limit)
            r = L.ixb_emu_geo_after_scan(h, md.value, p)
            if md.value <= limit:
                assert r == 0 and int(o[2]) == nb
                break
            nb += nb // 16 + 1
            grown += 1
            assert r == 1 and int(o[2]) == nb
        assert L.ixb_emu_total_buckets(nb, end.value, 4) == max(nb, (end.value + 3) // 4) + 1
        L.ixb_emu_geo_free(h)
    assert grown > 0
    # (at k = 25 and 21 the table starts with three bits and may earn the fourth once it has grown past a power of two: one bit less of the hash in the tag)
    assert limits == {14} if k in (31, 7) else 6 in limits
