"""Barcode whitelists without a GPU: the whitelist parser of the library (kamd_bus_whitelist_parse: host code), the CPU build of the table and of the
correction rule (tests/emu_buscorrect: kamd_buscorrect.h) against the brute-force restatement of tests/bus_correct_common.py, and a check that the
golden cases exercise every outcome.  Integers only: every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from tests import bus_correct_common as K
from tests.bus_sort_common import REC, make_records


@pytest.fixture(scope="module")
def api():
    import kallisto_amd.api as A
    A.load_library()
    return A


# ---- the parser ----
GOOD = [
    (b"ACGT\nTTTT\n", [0x1B, 0xFF], 4),
    (b"ACGT\r\nTTTT\r\n", [0x1B, 0xFF], 4),
    (b"ACGT\n\nTTTT", [0x1B, 0xFF], 4),                       # a blank line in the middle, no newline at the end
    (b"\n\r\nacgt\nAcGt\n", [0x1B, 0x1B], 4),                 # lower case; duplicates are kept
    (b"A\nC\nG\nT\nA\n", [0, 1, 2, 3, 0], 1),
    (b"T" * 32 + b"\n" + b"A" * 32 + b"\r\n" + b"ACGT" * 8, [2 ** 64 - 1, 0, int("1B" * 8, 16)], 32),
]
BAD = [
    (b"ACGT\nACNT\n", r"line 2: 'N' at base 3 is not one of ACGT"),
    (b"ACGT\n\nAC T\n", r"line 3: 0x20 at base 3"),
    (b"ACGT\nACG\n", r"line 2: 3 bases, the first barcode has 4"),
    (b"\nACG\r\n\nACGT\n", r"line 4: 4 bases, the first barcode has 3"),
    (b"A" * 33 + b"\n", r"line 1: 33 bases, a barcode holds at most 32"),
    (b"ACGT\rACGT\n", r"line 1: 0x0D at base 5"),
    (b"", r"no barcode"),
    (b"\n\r\n\n", r"no barcode"),
]


def test_parser_good_texts(api):
    for text, want, L in GOOD:
        codes, got_l = api.bus_whitelist_parse(text)
        assert (codes.tolist(), got_l) == (want, L), text
        assert [K.decode(c, L) for c in want] == [l.strip().upper() for l in text.decode().split("\n") if l.strip()]


def test_parser_refusals_name_the_line(api):
    for text, pattern in BAD:
        with pytest.raises(api.KallistoAmdError, match=pattern):
            api.bus_whitelist_parse(text)


def test_parser_count_only_and_capacity(api):
    import ctypes as C
    lib = api.load_library()
    text = b"ACGT\nTTTT\nCCCC\n"
    n, L, err = C.c_uint64(9), C.c_int32(9), C.create_string_buffer(b"#" * 63, 64)
    assert lib.kamd_bus_whitelist_parse(text, len(text), None, 0, C.byref(n), C.byref(L), err, 64) == 0
    assert (n.value, L.value, err.value) == (3, 4, b"")
    out = np.full(4, 7, np.uint64)
    assert lib.kamd_bus_whitelist_parse(text, len(text), out.ctypes.data, 2, C.byref(n), C.byref(L), err, 64) == -1   # room for two of three
    assert n.value == 3 and out.tolist() == [0x1B, 0xFF, 7, 7] and b"3 barcodes, the output holds 2" in err.value
    assert lib.kamd_bus_whitelist_parse(text, len(text), out.ctypes.data, 3, C.byref(n), C.byref(L), None, 0) == 0
    assert out.tolist() == [0x1B, 0xFF, 0x55, 7]
    assert lib.kamd_bus_whitelist_parse(text, 9, None, 0, C.byref(n), C.byref(L), None, 0) == 0 and n.value == 2     # len bounds the text: "ACGT\nTTTT"
    for cap in (0, 1, 5, 64):                                                                                           # the error text is cut to the buffer
        buf = C.create_string_buffer(b"#" * 63, 64)
        assert lib.kamd_bus_whitelist_parse(b"ACGT\nAC\n", 8, None, 0, C.byref(n), C.byref(L), buf if cap else None, cap) == -1
        assert buf.raw[cap:63] == b"#" * (63 - cap)
        if cap:
            assert buf.raw[:cap].split(b"\0")[0] == b"whitelist line 2: 2 bases, the first barcode has 4"[:cap - 1]


def test_whitelist_file_plain_and_gzip(api, tmp_path):
    import gzip
    W = K.random_codes(16, 300, 1)
    text = K.whitelist_text(W, 16)
    (tmp_path / "w.txt").write_bytes(text)
    with gzip.open(tmp_path / "w.txt.gz", "wb") as f:
        f.write(text)
    for name in ("w.txt", "w.txt.gz"):
        codes, L = api.bus_whitelist_read(str(tmp_path / name))
        assert L == 16 and np.array_equal(codes, W)
    (tmp_path / "bad.txt").write_bytes(b"ACGT\nACGX\n")
    with pytest.raises(api.KallistoAmdError, match=r"bad.txt: whitelist line 2"):
        api.bus_whitelist_read(str(tmp_path / "bad.txt"))


def test_parser_under_sanitizers():
    """the stand-alone program tests/emu_buscorrect/fuzz_main.cpp (its own main; address and undefined-behaviour sanitizers) feeds the parser malformed texts"""
    d = os.path.join(K.HERE, "emu_buscorrect")
    subprocess.check_call(["make", "-C", d, "wl_fuzz"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(d, "wl_fuzz")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
    assert b" 0 failures" in p.stdout


# ---- the table and the rule ----
def _assert_cpu_build_is_the_restatement(W, L, rec, n_buckets=0):
    wl = K.EmuWhitelist(W, L, n_buckets)
    try:
        out, status, stats = wl.correct(rec)
        want_out, want_status, want_stats = K.py_correct(W, L, rec)
        assert np.array_equal(status, want_status) and stats == want_stats
        assert out.tobytes() == want_out.tobytes()
        return wl.n_distinct, wl.max_chain, wl.n_buckets, want_stats
    finally:
        wl.close()


def test_capacity_rule_and_neighbours():
    lib = K.emu()
    for n in list(range(1, 70)) + [1000, 6794880]:
        b = int(lib.buscorrect_emu_n_buckets(n))
        assert b & (b - 1) == 0 and 4 * b >= n and (b == 1 or 4 * (b // 2) < n)        # the power of two >= n / 4, at least one bucket
    assert int(lib.buscorrect_emu_n_buckets(6794880)) * 64 == 128 << 20
    for L in K.LENGTHS:
        b = int(K.rand_barcodes(np.random.default_rng(L), L, 1)[0])
        got = [int(lib.buscorrect_emu_neighbour(b, L, j)) for j in range(3 * L)]
        assert sorted(got) == sorted(K.py_neighbours(b, L)) and len(set(got)) == 3 * L
        for j, g in enumerate(got):                                                      # lane j: position j / 3 from the front, base XOR (j % 3) + 1
            assert g ^ b == (j % 3 + 1) << (2 * (L - 1 - j // 3))


@pytest.mark.parametrize("L", K.LENGTHS)
def test_cpu_build_equals_the_restatement(L):
    for size in K.SIZES:
        W = K.random_codes(L, size, 100 * L + size)
        rec = K.mixture(W, L, 600, 7 * L + size)
        n_distinct, _, n_buckets, st = _assert_cpu_build_is_the_restatement(W, L, rec)
        assert n_distinct == len(set(W.tolist())) and n_buckets == int(K.emu().buscorrect_emu_n_buckets(len(W)))
        wl = K.EmuWhitelist(W, L)
        assert all(int(w) in wl for w in W)
        Wset = set(W.tolist())
        assert all((int(x) in wl) == (int(x) in Wset) for x in K.rand_barcodes(np.random.default_rng(size), L, 300))
        wl.close()
        if L >= 8 and size >= 7:
            assert st["n_exact"] and st["n_corrected"] and st["n_uncorrectable"]


def test_duplicates_and_order_do_not_matter():
    W = K.random_codes(16, 500, 3)
    rec = K.mixture(W, 16, 2000, 4)
    want = K.py_correct(W, 16, rec)
    rng = np.random.default_rng(5)
    for codes in (np.concatenate([W, W[:100], W[:100]]), W[rng.permutation(len(W))], W[::-1].copy()):
        wl = K.EmuWhitelist(codes, 16)
        out, status, stats = wl.correct(rec)
        assert wl.n_distinct == 500 and out.tobytes() == want[0].tobytes() and np.array_equal(status, want[1]) and stats == want[2]
        wl.close()


def test_complete_list_and_list_with_holes():
    L = 6
    full = np.arange(4 ** L, dtype=np.uint64)
    rec = K.with_fields(full[np.random.default_rng(1).permutation(4 ** L)], np.random.default_rng(2))
    _, _, _, st = _assert_cpu_build_is_the_restatement(full, L, rec)
    assert st["n_exact"] == 4 ** L == st["n_out"]
    holes = [0, 1, 4 ** L - 1, 1234, 1234 ^ (2 << 6)]                          # 0 and 1 are neighbours of each other, so are the last two
    W = np.array(sorted(set(full.tolist()) - set(holes)), np.uint64)
    _, _, _, st = _assert_cpu_build_is_the_restatement(W, L, rec)
    # a missing barcode has 3 L = 18 neighbours and at most one of them is missing too: every miss is ambiguous
    assert (st["n_exact"], st["n_corrected"], st["n_ambiguous"], st["n_uncorrectable"]) == (4 ** L - 5, 0, 5, 0)
    W1 = np.array([5], np.uint64)                                               # ... and with a single member, a miss is corrected or uncorrectable
    _, _, _, st = _assert_cpu_build_is_the_restatement(W1, L, rec)
    assert (st["n_exact"], st["n_corrected"], st["n_ambiguous"]) == (1, 18, 0)


def test_l32_marker_value():
    """at L = 32 every 64-bit value is a barcode, the empty-slot marker 2^64 - 1 (32 T) included"""
    L, ones = 32, K.ALL_ONES
    rng = np.random.default_rng(6)
    base = K.random_codes(L, 50, 7)
    probes = np.array([0, ones, ones ^ 1, ones ^ (3 << 62), 1, 2 << 62, ones ^ 5] + base[:10].tolist(), np.uint64)
    rec = K.with_fields(probes, rng)
    for extra in ([0, ones], [], [ones], [0], [ones ^ 1, ones ^ 2]):              # both, neither, each alone; two neighbours of the marker value
        W = np.concatenate([base, np.array(extra, np.uint64)])
        n_distinct, _, _, _ = _assert_cpu_build_is_the_restatement(W, L, rec)
        assert n_distinct == len(W)
        wl = K.EmuWhitelist(W, L)
        assert (ones in wl) == (ones in extra) and (0 in wl) == (0 in extra)
        wl.close()
    status = K.py_correct(np.concatenate([base, np.array([ones ^ 1, ones ^ 2], np.uint64)]), L, rec)[1]
    assert status[1] == K.AMBIGUOUS                                              # 32 T between ...TG and ...TC
    status = K.py_correct(np.concatenate([base, np.array([ones], np.uint64)]), L, rec)[1]
    assert status[1] == K.EXACT and status[2] == K.CORRECTED and status[3] == K.CORRECTED
    wl = K.EmuWhitelist(np.array([ones], np.uint64), L)                          # the marker value alone
    assert wl.n_distinct == 1 and ones in wl and 0 not in wl
    wl.close()


def test_high_bits():
    L = 8
    W = K.random_codes(L, 100, 8)
    w = int(W[0])
    bc = np.array([w, w | 1 << 16, w | 1 << 63, (w ^ 1) | 1 << 16, 1 << 16, K.ALL_ONES], np.uint64)
    rec = K.with_fields(bc, np.random.default_rng(9))
    _assert_cpu_build_is_the_restatement(W, L, rec)
    status = K.py_correct(W, L, rec)[1]
    assert status[0] == K.EXACT and all(s == K.UNCORRECTABLE for s in status[1:])
    with pytest.raises(ValueError):
        K.EmuWhitelist(np.array([w, 1 << 16], np.uint64), L)


@pytest.mark.parametrize("bucket", [5, 15])
def test_chain_over_several_buckets(bucket):
    """40 keys with one home bucket in a table of 16 buckets: the chain runs over five buckets; from the last bucket it wraps to bucket 0"""
    L, nb = 16, 16
    assert int(K.emu().buscorrect_emu_n_buckets(40)) == nb
    W = K.colliding_keys(L, 40, nb, bucket, 10 + bucket)
    assert {K.home(k, nb) for k in W.tolist()} == {bucket}
    others = K.colliding_keys(L, 200, nb, (bucket + 2) % nb, 11)                # non-members whose walk starts inside the chain
    near = np.array([K.substitute(np.random.default_rng(i), int(W[i % 40]), L) for i in range(200)], np.uint64)
    rec = K.with_fields(np.concatenate([W, others, near]), np.random.default_rng(12))
    n_distinct, max_chain, n_buckets, st = _assert_cpu_build_is_the_restatement(W, L, rec)
    assert (n_distinct, max_chain, n_buckets) == (40, 5, nb)
    assert st["n_exact"] >= 40 and st["n_corrected"] > 0


def test_golden_cases_exercise_every_outcome():
    """the whitelist of a golden case = the barcodes of the reference's records without an N: exact, corrected and uncorrectable records all occur,
    ambiguous ones on vasa, so a GPU test on these inputs exercises every path"""
    cases = K.golden_bc_cases()
    assert {"10xv3", "vasa", "surecell"} <= set(cases) and "no_bc" not in cases
    seen = {}
    for name in cases:
        W, L, lines = K.golden_whitelist(name)
        rec = make_records([bc for _, bc, _, _ in lines], [u for _, _, u, _ in lines], 0, [fl for fl, _, _, _ in lines])
        _, _, st = K.py_correct(W, L, rec)
        seen[name] = tuple(st[k] for k in K.STAT_KEYS)
        assert st["n_exact"] and st["n_corrected"] and st["n_uncorrectable"], (name, st)
        _assert_cpu_build_is_the_restatement(np.array(W, np.uint64), L, rec)
    assert seen["10xv3"] == (1875, 210, 0, 102) and seen["vasa"] == (1161, 152, 6, 53) and seen["surecell"] == (2450, 271, 0, 122)
    assert seen["vasa"][2] > 0
