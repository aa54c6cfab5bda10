"""The tag word of a tuple record in the table of distinct tuples (kamd_core.h tuple_tag -- the one function k_classify, k_tup_absorb,
k_tup_absorb4, k_tup_rehash and k_tup_store take tag and probe start from), driven on the CPU (tests/emu_tupletag).

  exact form   bit 63 set: a tuple of two sets (ids below 2^31) or of three sets (ids below 2^short_id_bits) IS its tag -- so the tag must be
               injective on those tuples, and tuple_of_tag must give the tuple back (k_tup_store rebuilds the store's record from it)
  hash form    everything else: bit 63 clear, hash bits in 32 .. 62, the low half free for the owner's offset
  never 0      0 is the empty slot
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BITS = 4   # every id below 2^4: the whole domain of the three-set exact form is enumerated
_lib = None


def _emu():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(HERE, "emu_tupletag")], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(HERE, "emu_tupletag", "libkamd_tupletag_emu.so"))
        _lib.emu_tuple_tag.restype = C.c_uint64
        _lib.emu_tuple_of_tag.restype = C.c_uint32
    return _lib


def _tag(rec, bits):
    L = _emu()
    a = np.asarray(rec, np.uint32)
    start, short = C.c_uint64(0), C.c_int32(0)
    w = L.emu_tuple_tag(a.ctypes.data_as(C.c_void_p), C.c_uint32(bits), C.byref(start), C.byref(short))
    return int(w), int(start.value), bool(short.value)


def _untag(word, bits):
    L = _emu()
    ids = np.zeros(3, np.uint32)
    m = L.emu_tuple_of_tag(C.c_uint64(word), C.c_uint32(bits), ids.ctypes.data_as(C.c_void_p))
    return tuple(int(x) for x in ids[:m])


def test_exact_tags_are_injective_and_invertible():
    seen = {}
    ids = range(1 << BITS)
    for m in (2, 3):
        for t in itertools.combinations(ids, m):   # (a record's ids are sorted and distinct)
            w, _, short = _tag([m, *t], BITS)
            assert short, t
            assert w >> 63 == 1 and ((w >> 62) & 1) == (m == 3), (t, hex(w))
            assert w not in seen, (t, seen.get(w))
            seen[w] = t
            assert _untag(w, BITS) == t
    assert len(seen) == 120 + 560   # C(16, 2) + C(16, 3)
    # the same holds for unsorted or repeated ids (nothing relies on it, but equal tags must still mean equal words)
    for t in itertools.product(ids, repeat=3):
        w, _, short = _tag([3, *t], BITS)
        assert short and _untag(w, BITS) == t
    # a two-set tuple is exact whatever the width of the three-set form, up to ids of 31 bits
    for t in [(0, 1), (5, (1 << 31) - 1), ((1 << 31) - 2, (1 << 31) - 1), (1 << 20, 1 << 30)]:
        for bits in (BITS, 20):
            w, _, short = _tag([2, *t], bits)
            assert short and _untag(w, bits) == t and w >> 62 == 2


def test_hash_form_keeps_bit_63_clear_and_the_low_half_free():
    rng = np.random.default_rng(5)
    recs = [[0], [1, 7], [2, 3, 1 << 31], [2, (1 << 31) + 5, (1 << 31) + 9], [3, 1, 2, 16], [3, 16, 17, 18], [3, 0, 1, 1 << BITS]]
    for m in (4, 5, 6, 12, 64, 65, 200):
        for _ in range(40):
            recs.append([m, *sorted(rng.choice(1 << 20, m, replace=False).tolist())])
    words = set()
    for rec in recs:
        w, start, short = _tag(rec, BITS)
        assert not short, rec
        assert w != 0 and w >> 63 == 0 and w & 0xFFFFFFFF == 0, (rec, hex(w))
        assert (start >> 31) & 0x7FFFFFFF == w >> 32   # (the probe start is the hash itself: bits 32 .. 62 are the tag's)
        words.add(w)
    assert len(words) > 0.99 * len(recs)
    # at the default width the same three-set tuples are exact
    assert _tag([3, 16, 17, 18], 20)[2] and _tag([3, 0, 1, (1 << 20) - 1], 20)[2] and not _tag([3, 0, 1, 1 << 20], 20)[2]


def test_no_tag_is_zero_and_the_two_forms_never_meet():
    for rec in ([2, 0, 0], [3, 0, 0, 0], [2, 0, 1], [0], [1, 0], [4, 0, 1, 2, 3]):
        for bits in (BITS, 20):
            w, _, short = _tag(rec, bits)
            assert w != 0 and (w >> 63 == 1) == short
