"""The device-side inflate's shared logic (kallisto_amd/csrc/kamd_inflate.h) on the CPU, through tests/emu_inflate: decoder, CRC-32, line count,
locate and the cut of whole records.  Expected values are zlib's and Python's."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from tests import inflate_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384   # kamd_inflate.h TEXT_CHUNK


@pytest.fixture(scope="module")
def emu():
    path = os.path.join(ROOT, "tests", "emu_inflate", "libkamd_inflate_emu.so")
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: run build()")
    L = C.CDLL(path)
    L.inf_emu_member.restype = C.c_int
    L.inf_emu_member.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.inf_emu_crc_lanes.restype = C.c_uint32
    L.inf_emu_crc_lanes.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
    L.inf_emu_lines.restype = C.c_uint64
    L.inf_emu_lines.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]
    L.inf_emu_locate.restype = C.c_uint64
    L.inf_emu_locate.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]
    L.inf_emu_text_cut.restype = None
    L.inf_emu_text_cut.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def _inflate(L, comp, isize, crc):
    out = C.create_string_buffer(isize + 1)
    got_crc, nl = C.c_uint32(0), C.c_uint32(0)
    r = L.inf_emu_member(comp, len(comp), out, isize, crc, C.byref(got_crc), C.byref(nl))
    return r, out.raw[:isize], got_crc.value, nl.value


def py_locate(text, k):
    """offset just behind newline number k (1-based); len(text) when there are fewer; 0 for k = 0"""
    pos = 0
    for _ in range(k):
        i = text.find(b"\n", pos)
        if i < 0:
            return len(text)
        pos = i + 1
    return pos


def py_cut(texts, max_records):
    r = min(min(t.count(b"\n") // 4 for t in texts), max_records)
    return r, [py_locate(t, 4 * r) for t in texts]


def test_the_stream_sets_are_what_the_tests_need():
    v, d = S.valid_members(), S.damaged_members()
    assert len(d) >= 20
    assert {m.isize for m in v} >= {1, 2, 97, 65280, 65536}
    kinds = {n.rsplit("_", 1)[-1].rstrip("0123456789") for n in (x.name for x in d)}
    assert {"cut", "hdrbit", "type", "nlen", "start", "minus", "plus", "crc"} <= kinds, kinds


@pytest.mark.parametrize("i", range(len(S.valid_members())), ids=[m.name for m in S.valid_members()])
def test_valid_stream_gives_zlibs_bytes_and_crc(emu, i):
    m = S.valid_members()[i]
    r, text, crc, nl = _inflate(emu, m.comp, m.isize, m.crc)
    assert r == 0
    assert text == m.text
    assert crc == zlib.crc32(m.text) & 0xFFFFFFFF
    assert nl == m.text.count(b"\n")


def test_every_damaged_stream_is_refused(emu):
    for d in S.damaged_members():
        r, _, _, _ = _inflate(emu, d.comp, d.isize, d.crc)
        assert r != 0, d.name


def test_reasons_of_the_plain_cases(emu):
    by = {d.name: d for d in S.damaged_members()}
    want = {"fastq_l6_type3": 5, "random_nlen": 6, "distance_before_start": 4, "fastq_l6_isize_minus1": 2, "fastq_l6_isize_plus1": 3, "fastq_l6_crc": 10,
            "fastq_l0_isize_minus1": 2, "tiny_97_isize_plus1": 3}
    for name, reason in want.items():
        d = by[name]
        assert _inflate(emu, d.comp, d.isize, d.crc)[0] == reason, name
    cut = [d for d in S.damaged_members() if "_cut" in d.name]
    assert cut and all(_inflate(emu, d.comp, d.isize, d.crc)[0] != 0 for d in cut)
    assert sum(_inflate(emu, d.comp, d.isize, d.crc)[0] == 1 for d in cut) >= len(cut) // 2   # (most cuts are met as a read beyond the input)


def test_crc_of_lane_slices_combines_to_zlibs(emu):
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 63, 64, 65, 97, 1000, 4097, 65280, 65536):
        buf = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        buf = buf.replace(b"\x0b", b"\n")
        for lanes in (1, 3, 64):
            nl = C.c_uint32(0)
            assert emu.inf_emu_crc_lanes(buf, n, lanes, C.byref(nl)) == zlib.crc32(buf) & 0xFFFFFFFF, (n, lanes)
            assert nl.value == buf.count(b"\n")


def _text_with_newlines_at(n, positions):
    t = bytearray(b"x" * n)
    for p in positions:
        t[p] = 10
    return bytes(t)


def test_lines_and_locate_agree_with_python(emu):
    member = 65280
    cases = [
        _text_with_newlines_at(3 * member, [0, 5, member - 1, member, member + 1, 2 * member - 1, 2 * member, 3 * member - 1]),   # first byte, last byte, either side of a boundary
        _text_with_newlines_at(2 * CHUNK + 7, [CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 6]),
        _text_with_newlines_at(100, []),
        b"\n" * 40000,
        S.valid_members()[2].text,
    ]
    for t in cases:
        total = t.count(b"\n")
        assert emu.inf_emu_lines(t, 0, len(t)) == total
        for lo, hi in ((1, len(t)), (3, len(t) - 3), (7, 8), (len(t) // 2, len(t) // 2), (member - 1, member + 1)):
            if lo <= hi <= len(t):
                assert emu.inf_emu_lines(t, lo, hi) == t[lo:hi].count(b"\n")
        ks = sorted({0, 1, 2, total // 2, total - 1, total, total + 1} & set(range(0, total + 2)))
        for k in ks:
            assert emu.inf_emu_locate(t, len(t), k) == py_locate(t, k), (len(t), k)


def _cut(L, texts, max_records):
    arr = (C.c_char_p * 2)(*texts, *([None] * (2 - len(texts))))
    n = (C.c_uint64 * 2)(*[len(t) for t in texts], *([0] * (2 - len(texts))))
    nrec, end = C.c_uint64(0), (C.c_uint64 * 2)(0, 0)
    L.inf_emu_text_cut(arr, n, len(texts), max_records, C.byref(nrec), end)
    return nrec.value, [end[i] for i in range(len(texts))]


def test_the_head_of_a_text_is_cut_at_whole_records(emu):
    fq = S._fastq_bytes(S._reads(900, 8))
    # line 4R ends exactly at a member boundary: the text up to a record's end is padded to 65 280 bytes by a longer header
    recs = fq.split(b"\n")
    head = b"\n".join(recs[:4 * 300]) + b"\n"
    pad = 2 * 65280 - len(head)
    assert pad > 0
    exact = head[:1] + b"p" * pad + head[1:]
    assert len(exact) == 2 * 65280 and exact.count(b"\n") == 1200
    tail = b"\n".join(recs[4 * 300:4 * 300 + 6]) + b"\n"        # one record and a half
    cases = [([exact + tail], 1 << 40), ([exact], 1 << 40), ([exact + tail[:10]], 1 << 40), ([fq], 10), ([fq], 0),
             ([b"@r\nACGT\n+\n"], 5), ([b"no newline at all"], 5), ([b"\n\n\n"], 1), ([b"\n\n\n\n"], 1),
             ([fq, exact + tail], 1 << 40), ([exact + tail, fq[:5000]], 1 << 40), ([fq, fq[:-1]], 1 << 40), ([fq, b"@r\n"], 7)]
    for texts, mx in cases:
        assert _cut(emu, texts, mx) == py_cut(texts, mx), (len(texts[0]), mx)
    r, end = _cut(emu, [exact + tail], 1 << 40)
    assert r == 301 and end[0] > 2 * 65280
    r, end = _cut(emu, [exact + tail[:10]], 1 << 40)
    assert r == 300 and end[0] == 2 * 65280                      # ... the cut falls on the boundary itself
