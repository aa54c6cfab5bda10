"""Barcode / UMI technologies (`bus -x <technology>`) without a GPU: the layout parser (kamd_bus.cpp) and the per-item rules (kamd_bustag.h) compiled
for the CPU (tests/emu_bustag, TEST INFRASTRUCTURE), against a table written out here, a short Python restatement of the rules
(tests/bus_sc_common.py), and the fixtures of tests/golden/bus_sc, which the unmodified reference wrote.  Integers only: every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import bus_sc_common as B

FR, NONE = 1, 0
# technology -> (files, barcode parts, UMI parts, sequence part, default strand): the reference's table (src/main.cpp:1283-1408), written out once more
NAMED = {
    "10XV2": (2, [(0, 0, 16)], [(0, 16, 26)], (1, 0, 0), FR),
    "10XV3": (2, [(0, 0, 16)], [(0, 16, 28)], (1, 0, 0), FR),
    "VISIUM": (2, [(0, 0, 16)], [(0, 16, 28)], (1, 0, 0), FR),
    "SURECELL": (2, [(0, 0, 6), (0, 21, 27), (0, 42, 48)], [(0, 51, 59)], (1, 0, 0), FR),
    "DROPSEQ": (2, [(0, 0, 12)], [(0, 12, 20)], (1, 0, 0), NONE),
    "INDROPSV1": (2, [(0, 0, 11), (0, 30, 38)], [(0, 42, 48)], (1, 0, 0), NONE),
    "INDROPSV2": (2, [(1, 0, 11), (1, 30, 38)], [(1, 42, 48)], (0, 0, 0), NONE),
    "CELSEQ": (2, [(0, 0, 8)], [(0, 8, 12)], (1, 0, 0), FR),
    "CELSEQ2": (2, [(0, 6, 12)], [(0, 0, 6)], (1, 0, 0), FR),
    "SPLIT-SEQ": (2, [(1, 10, 18), (1, 48, 56), (1, 78, 86)], [(1, 0, 10)], (0, 0, 0), FR),
    "SCRBSEQ": (2, [(0, 0, 6)], [(0, 6, 16)], (1, 0, 0), NONE),
    "BDWTA": (2, [(0, 0, 9), (0, 21, 30), (0, 43, 52)], [(0, 52, 60)], (1, 0, 0), FR),
    "VASA-SEQ": (1, [(0, 6, 14)], [(0, 0, 6)], (0, 14, 0), FR),
}
CUSTOM = {
    "0,0,2:0,2,6:1,0,0": (2, [(0, 0, 2)], [(0, 2, 6)], (1, 0, 0), NONE),          # the reference's own functional test (func_tests/runtests.sh:327)
    "0,0,8:0,8,16:1,33,100": (2, [(0, 0, 8)], [(0, 8, 16)], (1, 33, 100), NONE),
    "0,0,8:0,8,0:1,0,0": (2, [(0, 0, 8)], [(0, 8, 0)], (1, 0, 0), NONE),
    "0,0,8:-1,-1,-1:1,0,0": (2, [(0, 0, 8)], [(-1, -1, -1)], (1, 0, 0), NONE),
    "-1,-1,-1:0,0,10:1,0,0": (2, [(-1, -1, -1)], [(0, 0, 10)], (1, 0, 0), NONE),
    "-1,-1,-1:-1,-1,-1:0,0,0": (1, [(-1, -1, -1)], [(-1, -1, -1)], (0, 0, 0), NONE),
    " 0, 0,16x:0,16,28,:0,5,0": (1, [(0, 0, 16)], [(0, 16, 28)], (0, 5, 0), NONE),   # std::stoi's reading of a token; a trailing comma ends the list
}


@pytest.mark.parametrize("tech", sorted(NAMED) + sorted(CUSTOM))
def test_parser_layouts(tech):
    want = dict(NAMED, **CUSTOM)[tech]
    for spelling in ([tech, tech.lower(), tech.capitalize()] if tech in NAMED else [tech]):
        L, strand = B.parse(spelling)
        d = L.as_dict()
        assert (d["n_files"], d["bc"], d["umi"], d["seq"], strand) == want, spelling
        assert B.emu().bus_emu_check(C.byref(L), None, 0) == 0


PARSE_ERRORS = {
    "0,0,16": 'Error: technology string must contain two colons (:), none found: "0,0,16"',
    "nosuchtech": 'Error: technology string must contain two colons (:), none found: "nosuchtech"',
    "0,0,16:0,16,28": 'Error: technology string must contain two colons (:), only one found: "0,0,16:0,16,28"',
    "0,0,16:0,16,28:1,0,0:1,0,0": 'Error: technology string must contain two colons (:), three found: "0,0,16:0,16,28:1,0,0:1,0,0"',
    "0,a,16:0,16,28:1,0,0": 'Error: converting to int: "a"',
    "0,,16:0,16,28:1,0,0": 'Error: converting to int: ""',
    "0,0:0,16,28:1,0,0": "Error: number of values has to be multiple of 3 0,0",
    "-2,0,16:0,16,28:1,0,0": "Error: invalid file number (-2)  -2,0,16",
    "0,-1,16:0,16,28:1,0,0": "Error: invalid start (-1)  0,-1,16",
    "0,0,16:0,28,16:1,0,0": "Error: invalid stop (16) has to be after start (28)  0,28,16",
    "0,0,16:0,16,16:1,0,0": "Error: invalid stop (16) has to be after start (16)  0,16,16",
    ":0,16,28:1,0,0": "Error: empty barcode list ",
    "0,0,16::1,0,0": "Error: empty UMI list ",
    "0,0,16:0,16,28:": "Error: empty sequence list 0,0,16",
}


@pytest.mark.parametrize("tech", sorted(PARSE_ERRORS))
def test_parser_messages_are_parse_technologys(tech):
    with pytest.raises(ValueError) as e:
        B.parse(tech)
    assert str(e.value) == PARSE_ERRORS[tech]


REFUSALS = {
    "10XV1": "three files", "indropsv3": "three files", "SMARTSEQ2": "three or four files", "SmartSeq3": "four files", "STORM-seq": "two sequence parts",
    "bulk": "not a barcode / UMI technology", "0,0,8:0,8,16:0,0,0,1,0,0": "exactly one sequence part", "0,0,8:1,0,8:2,0,0": "one or two files",
    "0,0,8:RX:1,0,0": "FASTQ comment", "0,0,33:0,33,40:1,0,0": "33 fixed bases", "0,0,20,0,30,43:0,50,58:1,0,0": "33 fixed bases",
    "0,0,8:0,8,41:1,0,0": "33 fixed bases", "0,0,8:0,8,16:-1,-1,-1": "sequence", "0,0,8,-1,-1,-1:0,8,16:1,0,0": "file -1",
    "0,0,1,0,1,2,0,2,3,0,3,4,0,4,5,0,5,6,0,6,7,0,7,8,0,8,9:0,9,16:1,0,0": "at most 8 parts", "0,0,70000:0,8,16:1,0,0": "65535",
    "99999999999,0,8:0,8,16:1,0,0": "out of range",
}


@pytest.mark.parametrize("tech", sorted(REFUSALS))
def test_parser_refusals_say_why(tech):
    with pytest.raises(ValueError, match=REFUSALS[tech]):
        B.parse(tech)


def test_parser_error_buffer_is_respected():
    L, strand = B.Layout(), C.c_int32(0)
    for cap in (0, 1, 5, 40):
        buf = C.create_string_buffer(b"#" * 63, 64)
        assert B.emu().bus_emu_parse(b"0,0,16", C.byref(L), C.byref(strand), buf if cap else None, cap) == -1
        raw = buf.raw
        assert raw[cap:63] == b"#" * (63 - cap)
        if cap:
            assert b"\0" in raw[:cap] and raw[:cap].split(b"\0")[0] == b"Error: technology string must contain two colons"[:cap - 1]


def test_parser_under_sanitizers():
    """the stand-alone program tests/emu_bustag/fuzz_main.cpp (its own main; address and undefined-behaviour sanitizers) feeds the parser malformed strings"""
    d = os.path.join(B.HERE, "emu_bustag")
    subprocess.check_call(["make", "-C", d, "parse_fuzz"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(d, "parse_fuzz")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
    assert b" 0 failures" in p.stdout


def test_seq_max_len():
    lib = B.emu()
    for tech, max_len, want in [("10XV3", 100, 100), ("VASA-SEQ", 100, 86), ("VASA-SEQ", 10, 1), ("0,0,8:0,8,16:1,33,100", 150, 67), ("0,0,8:0,8,16:1,33,100", 50, 17),
                                ("0,0,8:0,8,16:1,33,100", 33, 1)]:
        L, _ = B.parse(tech)
        assert lib.bus_emu_seq_max_len(C.byref(L), max_len) == want, (tech, max_len)


# ---- per-item rules against the Python restatement ----
def test_py_encode_is_string_to_binary():
    assert B.py_encode(b"ACGT") == (0b00011011, 0)
    assert B.py_encode(b"acgt") == (0b00011011, 0)
    assert B.py_encode(b"NACG") == (0b10000110, 1 | 0 << 2)
    assert B.py_encode(b"ACNNNN") == (0b000110101010, 3 | 2 << 2)
    assert B.py_encode(b"A" * 31 + b"n" + b"N") == (2, 1 | 31 << 2)            # the 33rd base is not looked at
    assert B.py_encode(b"T" * 40) == (2 ** 64 - 1, 0)


def _emu_vs_python(tech, items, seq_max_len=None):
    L, _ = B.parse(tech)
    lay = L.as_dict()
    flat = [r for it in items for r in it]
    words, lens, max_len = B.pack_host(flat)
    tags, src, sw, sl, st, sml = B.emu_split(L, words, lens, len(items), max_len, seq_max_len)
    surv, pst = B.py_split(lay, items)
    assert st == pst
    assert src.tolist() == [i for i, _ in surv]
    for f in ("barcode", "umi", "flags", "bc_len", "umi_len"):
        assert tags[f].tolist() == [d[f] for _, d in surv], f
    assert sl.tolist() == [len(d["seq"]) for _, d in surv]
    want_w, want_l, _ = B.pack_host([d["seq"] for _, d in surv], sml)
    assert np.array_equal(sw, want_w)   # every word of every record: 2-bit words, flag word, mask words, padding
    return st


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_emu_items_equal_python_rules(name):
    _, _, items, _ = B.case_reads(name)
    st = _emu_vs_python(B.CASES[name]["tech"], items)
    assert st["n_dropped_umi"] + st["n_dropped_bc"] > 0 and st["n_valid"] > 0


@pytest.mark.parametrize("start", [0, 1, 15, 16, 17, 31, 32, 33])
def test_emu_cut_starts_and_lengths(start):
    """the repack at word and mask-word boundaries: cut lengths 0, 1, 16, 32 and more, Ns on both sides of the cut, seq_max_len larger than needed"""
    rnd = B.lcg(1000 + start)
    items = []
    for n in (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 90):
        for rep in range(3):
            s = bytearray(b"ACGT"[next(rnd) % 4] for _ in range(start + n))
            for _ in range(rep * 2):
                if s:
                    s[next(rnd) % len(s)] = ord("N")
            items.append((b"ACGTACGTAACCGGTT", bytes(s)))
    for extra in (None, 150):
        _emu_vs_python("0,0,8:0,8,16:1,%d,0" % start, items, extra)
        _emu_vs_python("0,0,8:0,8,16:1,%d,%d" % (start, start + 32), items, extra)


# ---- against the reference ----
def _records_of(name):
    """emu tags + the oracle's set of every cut sequence -> the sorted record lines, and the emu's statistics"""
    L, _, items, _ = B.case_reads(name)
    words, lens, n, max_len = B.case_batch(name)
    tags, src, _, _, st, _ = B.emu_split(L, words, lens, n, max_len)
    sets = B.oracle_sets(name)
    assert [i for i, _ in sets] == src.tolist()
    return sorted((int(t["flags"]), int(t["barcode"]), int(t["umi"]), s) for t, (_, s) in zip(tags, sets) if s), st, L


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_records_equal_the_reference(name):
    assert name in B.golden_cases(), "the reference ran every case when the fixtures were made (tests/golden/bus_sc/dropped.json is empty)"
    meta, want = B.load_golden(name)
    got, st, L = _records_of(name)
    assert got == want
    assert st["n_valid"] == meta["n_processed"] and st["n_items"] == meta["n_reads"] == meta["reference_run_info"]["n_processed"]
    assert len(got) == meta["n_pseudoaligned"] == meta["reference_run_info"]["n_pseudoaligned"]
    assert (1,) + B.header_lens(L.as_dict(), st) == tuple(meta["bus_header"])


def test_absent_umi_repeats_the_barcode_flag():
    """ProcessReads.cpp:1744-1745 shifts in whatever `f` last held: with no UMI that is the barcode's flag.  The golden shows it."""
    _, want = B.load_golden("no_umi")
    assert all(u == 2 ** 64 - 1 and (fl >> 8) == (fl & 0xFF) for fl, _, u, _ in want)
    assert any(fl for fl, _, _, _ in want)
    _, want = B.load_golden("no_bc")
    assert all(bc == 0 and (fl & 0xFF) == 0 for fl, bc, _, _ in want) and any(fl >> 8 for fl, _, _, _ in want)
