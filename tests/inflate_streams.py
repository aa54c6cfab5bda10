"""Raw DEFLATE streams for the tests of the device-side inflate (kamd_inflate.h / kamd_inflate.hip): the valid members and the damaged set.

Every expected value is zlib's: the text of a valid stream is what `zlib.decompressobj(-15)` gives (also for the hand-assembled ones), its
CRC is `zlib.crc32`; a damaged stream is kept only when zlib itself refuses it (decoding fails, the stream does not end, or the bytes are
not ISIZE bytes with the trailer's CRC)."""
import functools
import os
import struct
import zlib

import numpy as np

from tests.test_fastq_input import _fastq_bytes, _reads


class Member:
    def __init__(self, name, comp, text):
        self.name, self.comp, self.text = name, bytes(comp), bytes(text)
        self.isize, self.crc = len(text), zlib.crc32(text) & 0xFFFFFFFF


class Damaged:
    def __init__(self, name, comp, isize, crc):
        self.name, self.comp, self.isize, self.crc = name, bytes(comp), isize, crc


def _deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


def _zlib_text(comp):
    d = zlib.decompressobj(-15)
    out = d.decompress(comp)
    assert d.eof, "zlib does not see the end of this stream"
    return out


def zlib_accepts(comp, isize, crc):
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(comp)
    except zlib.error:
        return False
    return d.eof and len(out) == isize and (zlib.crc32(out) & 0xFFFFFFFF) == crc


class _BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):            # a field: least significant bit first
        self.bits += [(value >> i) & 1 for i in range(n)]

    def code(self, code, n):            # a Huffman code: most significant bit first
        self.bits += [(code >> (n - 1 - i)) & 1 for i in range(n)]

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def bytes(self):
        self.align()
        return bytes(sum(b << i for i, b in enumerate(self.bits[j:j + 8])) for j in range(0, len(self.bits), 8))


def _canonical(lens):
    """{symbol: length} -> {symbol: (code, length)}"""
    out, code, prev = {}, 0, 0
    for length, sym in sorted((l, s) for s, l in lens.items() if l):
        code <<= length - prev
        out[sym] = (code, length)
        code += 1
        prev = length
    return out


_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _dynamic_header(w, final, hlit, hdist, cl_lens, ops):
    """ops: (code-length symbol, extra value) in stream order"""
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    hclen = max(i for i, s in enumerate(_CL_ORDER) if cl_lens.get(s, 0)) + 1
    w.put(hlit - 257, 5); w.put(hdist - 1, 5); w.put(hclen - 4, 4)
    for s in _CL_ORDER[:hclen]:
        w.put(cl_lens.get(s, 0), 3)
    codes = _canonical(cl_lens)
    for sym, extra in ops:
        w.code(*codes[sym])
        if sym >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[sym])


def hand_repeat_across_boundary():
    """A dynamic block of 257 literal/length and 4 distance lengths: 253 zeros, then eight 2s of which six are one `repeat previous` that
    starts at length 254 and ends at distance length 2."""
    w = _BitWriter()
    _dynamic_header(w, True, 257, 4, {18: 1, 2: 2, 16: 2}, [(18, 127), (18, 104), (2, 0), (16, 3), (2, 0)])
    lit = _canonical({253: 2, 254: 2, 255: 2, 256: 2})
    for s in (253, 254, 255, 253, 253, 255, 256):
        w.code(*lit[s])
    return w.bytes()


def hand_single_distance_code():
    """A dynamic block whose distance code is a single code of one bit (incomplete, and accepted by zlib): 'a', then matches of length 3 at distance 1."""
    w = _BitWriter()
    _dynamic_header(w, True, 258, 1, {18: 1, 1: 2, 2: 2}, [(18, 86), (2, 0), (18, 127), (18, 9), (2, 0), (1, 0), (1, 0)])
    lit = _canonical({97: 2, 256: 2, 257: 1})
    w.code(*lit[97])
    for _ in range(5):
        w.code(*lit[257]); w.code(0, 1)
    w.code(*lit[97])
    w.code(*lit[256])
    return w.bytes()


def _fixed_lit(w, s):
    if s < 144: w.code(0x30 + s, 8)
    elif s < 256: w.code(0x190 + s - 144, 9)
    elif s < 280: w.code(s - 256, 7)
    else: w.code(0xC0 + s - 280, 8)


def hand_distance_32768(rng):
    """32 768 stored bytes, then a fixed block with a match of length 258 at distance 32 768 (zlib's own deflate never looks that far back)."""
    data = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = _BitWriter()
    w.put(0, 1); w.put(0, 2); w.align()
    w.put(32768, 16); w.put(32768 ^ 0xFFFF, 16)
    for b in data:
        w.put(b, 8)
    w.put(1, 1); w.put(1, 2)
    _fixed_lit(w, 285)                      # length 258
    w.code(29, 5); w.put(32768 - 24577, 13)   # distance 24577 + 8191
    _fixed_lit(w, 65)
    _fixed_lit(w, 256)
    return w.bytes()


def hand_distance_before_start():
    """A fixed block that begins with a match (length 3, distance 1): there is no byte to copy."""
    w = _BitWriter()
    w.put(1, 1); w.put(1, 2)
    _fixed_lit(w, 257); w.code(0, 5)
    _fixed_lit(w, 256)
    return w.bytes()


@functools.lru_cache(maxsize=None)
def valid_members():
    rng = np.random.default_rng(20250)
    fq = _fastq_bytes(_reads(700, 3))
    assert len(fq) > 65280
    one = b"A" * 65536
    per3 = (b"xyz" * 22000)[:65280]
    rnd = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    out = []
    for level in (0, 1, 6, 9):
        out.append(Member(f"fastq_l{level}", _deflate(fq[:65280] if level else fq[:60000], level), fq[:65280] if level else fq[:60000]))
    out.append(Member("fastq_fixed", _deflate(fq[:30000], 6, zlib.Z_FIXED), fq[:30000]))
    out.append(Member("fastq_huffman_only", _deflate(fq[:30000], 6, zlib.Z_HUFFMAN_ONLY), fq[:30000]))
    out.append(Member("one_byte_64k", _deflate(one, 6), one))
    out.append(Member("one_byte_fixed", _deflate(one[:5000], 9, zlib.Z_FIXED), one[:5000]))
    out.append(Member("period3", _deflate(per3, 6), per3))
    out.append(Member("random", _deflate(rnd, 6), rnd))
    out.append(Member("full_65280", _deflate(fq[100:100 + 65280], 6), fq[100:100 + 65280]))
    for n in (1, 2, 97):
        out.append(Member(f"tiny_{n}", _deflate(fq[:n], 6), fq[:n]))
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    out.append(Member("full_flush", co.compress(fq[:20000]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(fq[20000:45000]) + co.flush(), fq[:45000]))
    for name, comp in (("hand_dist_32768", hand_distance_32768(rng)), ("hand_repeat_boundary", hand_repeat_across_boundary()),
                       ("hand_single_dist", hand_single_distance_code())):
        out.append(Member(name, comp, _zlib_text(comp)))
    assert out[-3].text[32768:32768 + 258] == out[-3].text[:258] and out[-3].isize == 32768 + 259
    assert out[-1].text == b"a" * 16 + b"a"
    return tuple(out)


@functools.lru_cache(maxsize=None)
def damaged_members():
    cand = []
    for m in valid_members():
        n = len(m.comp)
        for cut in sorted({n // 4, n // 2, n - 1}):
            cand.append(Damaged(f"{m.name}_cut{cut}", m.comp[:cut], m.isize, m.crc))
    by = {m.name: m for m in valid_members()}

    def flip(m, bit):
        b = bytearray(m.comp); b[bit >> 3] ^= 1 << (bit & 7); return bytes(b)
    for name in ("fastq_l6", "fastq_l9", "period3", "hand_repeat_boundary", "hand_single_dist"):
        for bit in (4, 9, 14, 19, 40, 77):
            cand.append(Damaged(f"{name}_hdrbit{bit}", flip(by[name], bit), by[name].isize, by[name].crc))
    for name in ("fastq_l6", "random", "tiny_1"):
        b = bytearray(by[name].comp); b[0] |= 0x06
        cand.append(Damaged(f"{name}_type3", b, by[name].isize, by[name].crc))
    for name in ("fastq_l0", "random"):
        b = bytearray(by[name].comp); b[3] ^= 0x10
        cand.append(Damaged(f"{name}_nlen", b, by[name].isize, by[name].crc))
    cand.append(Damaged("distance_before_start", hand_distance_before_start(), 3, zlib.crc32(b"\0\0\0") & 0xFFFFFFFF))
    for name in ("fastq_l6", "one_byte_64k", "tiny_97", "fastq_l0", "hand_single_dist"):
        m = by[name]
        if m.isize > 0:
            cand.append(Damaged(f"{name}_isize_minus1", m.comp, m.isize - 1, m.crc))
        if m.isize < 65536:
            cand.append(Damaged(f"{name}_isize_plus1", m.comp, m.isize + 1, m.crc))
        cand.append(Damaged(f"{name}_crc", m.comp, m.isize, m.crc ^ 0x00010000))
    kept = tuple(d for d in cand if not zlib_accepts(d.comp, d.isize, d.crc))
    assert len(kept) >= 20, len(kept)
    return kept


def write_dir(path):
    """The streams as files, for the stand-alone sanitizer program of tests/emu_inflate (fuzz_main.cpp says the layout)."""
    os.makedirs(path, exist_ok=True)
    for m in valid_members():
        with open(os.path.join(path, m.name + ".valid"), "wb") as f:
            f.write(struct.pack("<II", m.isize, m.crc) + m.comp)
        with open(os.path.join(path, m.name + ".out"), "wb") as f:
            f.write(m.text)
    for d in damaged_members():
        with open(os.path.join(path, d.name + ".bad"), "wb") as f:
            f.write(struct.pack("<II", d.isize, d.crc) + d.comp)


if __name__ == "__main__":
    import sys
    write_dir(sys.argv[1])
    print(len(valid_members()), "valid,", len(damaged_members()), "damaged")
