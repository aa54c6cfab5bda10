"""kamd_bgzf_inflate and kamd_text_cut on the GPU (k_bgzf_inflate, k_text_lines, k_text_locate).  Expected bytes, CRCs and the verdict on every
damaged stream are zlib's (tests/inflate_streams.py); the cuts are a Python search.  Every damaged stream is corrupt in its data only: the
decoder refuses it with a reason, nothing here can fault."""
import numpy as np
import pytest

from tests import inflate_streams as S
from tests.test_inflate_cpu import py_cut

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import kallisto_amd as ka
    c = ka.Context(0)
    yield c
    c.close()


def _layout(streams, residues=False, dst_gap=0):
    """members = [(src_off, src_len, isize, crc, dst_off)], the compressed bytes, the size of the text.  residues: member i starts at
    an offset = i mod 16 in the compressed bytes and at (5 i + 3) mod 16 in the text, so that both take every residue."""
    comp, members, dst = bytearray(), [], 0
    for i, m in enumerate(streams):
        if residues:
            comp += b"\xEE" * ((i - len(comp)) % 16)
            dst += (5 * i + 3 - dst) % 16
        members.append((len(comp), len(m.comp), m.isize, m.crc, dst))
        comp += m.comp
        dst += m.isize + dst_gap
    return members, bytes(comp), dst


def _run(ctx, streams, **kw):
    import torch
    members, comp, n_text = _layout(streams, **kw)
    d_comp = torch.frombuffer(bytearray(comp + b"\0"), dtype=torch.uint8).cuda()
    d_text = torch.full((n_text + 64,), FILL, dtype=torch.uint8, device="cuda")
    res = ctx.bgzf_inflate(d_comp, members, d_text, comp_bytes=len(comp), text_cap=n_text)
    return res, members, d_text.cpu().numpy()


def _expected_text(streams, members, n):
    want = np.full(n, FILL, np.uint8)
    for m, (_, _, isize, _, dst) in zip(streams, members):
        want[dst:dst + isize] = np.frombuffer(m.text, np.uint8)
    return want


def test_all_valid_members_in_one_call_at_every_alignment(ctx):
    v = list(S.valid_members())
    assert len(v) >= 16
    res, members, got = _run(ctx, v, residues=True)
    assert {m[0] % 16 for m in members} == set(range(16)) and {m[4] % 16 for m in members} == set(range(16))
    assert res["status"] == 0 and res["n_bytes"] == sum(m.isize for m in v)
    assert res["n_newlines"] == sum(m.text.count(b"\n") for m in v)
    want = _expected_text(v, members, len(got))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"first differing byte at {bad[0]} (members at {[m[4] for m in members]})"   # the gaps and the 64 bytes behind included


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_calls_of_n_members_back_to_back(ctx, n):
    v = S.valid_members()
    streams = [v[(3 * i + n) % len(v)] for i in range(n)]
    res, members, got = _run(ctx, streams)
    assert res["status"] == 0 and res["n_bytes"] == sum(m.isize for m in streams)
    assert res["n_newlines"] == sum(m.text.count(b"\n") for m in streams)
    assert np.array_equal(got, _expected_text(streams, members, len(got)))


def test_each_damaged_member_among_valid_ones_is_reported(ctx):
    by = {m.name: m for m in S.valid_members()}
    good = [by["tiny_97"], by["hand_single_dist"], by["fastq_fixed"], by["tiny_1"]]
    for i, d in enumerate(S.damaged_members()):
        pos = i % 5
        streams = good[:pos] + [d] + good[pos:]
        res, members, got = _run(ctx, streams, dst_gap=7)
        assert res["status"] == 1 and res["first_bad_member"] == pos and res["reason"] != 0, (d.name, res)
        # what lies outside the members' destinations stays untouched, and the valid members of the call are decoded all the same
        want = np.full(len(got), FILL, np.uint8)
        mask = np.ones(len(got), bool)
        for m, (_, _, isize, _, dst) in zip(streams, members):
            if m is d:
                mask[dst:dst + isize] = False
            else:
                want[dst:dst + isize] = np.frombuffer(m.text, np.uint8)
        assert np.array_equal(got[mask], want[mask]), d.name


def test_reasons_match_the_cpu_build(ctx):
    by = {d.name: d for d in S.damaged_members()}
    for name, reason in {"fastq_l6_type3": 5, "random_nlen": 6, "distance_before_start": 4, "fastq_l6_isize_minus1": 2, "fastq_l6_isize_plus1": 3,
                         "fastq_l6_crc": 10}.items():
        res, _, _ = _run(ctx, [by[name]])
        assert (res["status"], res["reason"], res["first_bad_member"]) == (1, reason, 0), name


def test_debug_entry_with_and_without_the_crc_pass(ctx):
    """kamd_debug_bgzf_inflate: the same text either way; without the check a wrong CRC goes unnoticed and no newlines are counted"""
    import torch
    by = {m.name: m for m in S.valid_members()}
    bad = next(d for d in S.damaged_members() if d.name == "fastq_l6_crc")
    for streams in ([by["fastq_l6"], by["tiny_97"]], [by["tiny_97"], bad]):
        members, comp, n_text = _layout(streams)
        d_comp = torch.frombuffer(bytearray(comp + b"\0" * 4), dtype=torch.uint8).cuda()
        for check in (True, False):
            d_text = torch.full((n_text + 64,), FILL, dtype=torch.uint8, device="cuda")
            res = ctx.bgzf_inflate(d_comp, members, d_text, comp_bytes=len(comp), text_cap=n_text, debug_check_crc=check)
            assert res["kernel_ms"] > 0
            if check and streams[1] is bad:
                assert (res["status"], res["reason"], res["first_bad_member"]) == (1, 10, 1)
                continue
            assert res["status"] == 0 and res["n_newlines"] == (sum(m.text.count(b"\n") for m in streams) if check else 0)
            want = by["fastq_l6"].text if streams[1] is bad else streams[1].text
            dst = members[1][4]
            assert bytes(d_text.cpu().numpy()[dst:dst + len(want)]) == want


def _dev_text(t, junk=b"\n" * 64):
    """the text on the device, 16-byte aligned, with newlines behind its end that must not be counted"""
    import torch
    return torch.frombuffer(bytearray(t + junk), dtype=torch.uint8).cuda()


def test_text_cut_against_the_python_cut(ctx):
    fq = S._fastq_bytes(S._reads(2500, 8))          # several chunks of newline counts
    fq2 = S._fastq_bytes(S._reads(2500, 9, lo=30, hi=60))
    assert len(fq) > 5 * 16384
    cases = [([fq], 1 << 40), ([fq], 10), ([fq], 0), ([fq[:-1]], 1 << 40), ([fq[:40000]], 1 << 40), ([fq[:16384]], 1 << 40), ([fq[:16385]], 1 << 40),
             ([b"@r\nACGT\n+\n"], 5), ([b"no newline at all"], 5), ([b"\n\n\n\n"], 1), ([b""], 3),
             ([fq, fq2], 1 << 40), ([fq, fq2[:30000]], 1 << 40), ([fq[:50000], fq2], 1 << 40), ([fq, fq2], 777), ([fq, b"@r\n"], 7), ([fq, fq2], 0)]
    for texts, mx in cases:
        dev = [_dev_text(t) for t in texts]
        got = ctx.text_cut(dev, [len(t) for t in texts], mx)
        assert got == py_cut(texts, mx), ([len(t) for t in texts], mx)


def test_argument_errors_are_refused_before_any_launch(ctx):
    import torch
    import kallisto_amd as ka
    m = S.valid_members()[0]
    d_comp = torch.frombuffer(bytearray(m.comp), dtype=torch.uint8).cuda()
    d_text = torch.full((m.isize + 64,), FILL, dtype=torch.uint8, device="cuda")
    ok = (0, len(m.comp), m.isize, m.crc, 0)
    for members, comp_bytes, cap, word in (([(1, len(m.comp), m.isize, m.crc, 0)], len(m.comp), m.isize, "comp_bytes"),
                                           ([(len(m.comp) + 1, 0, m.isize, m.crc, 0)], len(m.comp), m.isize, "comp_bytes"),
                                           ([ok, (0, len(m.comp), m.isize, m.crc, 1)], len(m.comp), m.isize, "text_cap"),
                                           ([(0, len(m.comp), m.isize, m.crc, 2 ** 63)], len(m.comp), m.isize, "text_cap")):
        with pytest.raises(ka.KallistoAmdError) as e:
            ctx.bgzf_inflate(d_comp, members, d_text, comp_bytes=comp_bytes, text_cap=cap)
        assert "(-1)" in str(e.value) and word in str(e.value)
    # a stream longer than any member's, and a base pointer that is not 4-byte aligned (the offsets may be anything, the base may not)
    big = torch.zeros((1 << 20) + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ka.KallistoAmdError) as e:
        ctx.bgzf_inflate(big, [(0, (1 << 20) + 1, m.isize, m.crc, 0)], d_text, text_cap=m.isize)
    assert "(-1)" in str(e.value) and "src_len" in str(e.value)
    shifted = torch.zeros(len(m.comp) + 8, dtype=torch.uint8, device="cuda")
    shifted[1:1 + len(m.comp)] = d_comp
    with pytest.raises(ka.KallistoAmdError) as e:
        ctx.bgzf_inflate(shifted[1:], [ok], d_text, comp_bytes=len(m.comp), text_cap=m.isize)
    assert "(-1)" in str(e.value) and "aligned" in str(e.value)
    assert ctx.bgzf_inflate(shifted, [(1, len(m.comp), m.isize, m.crc, 0)], big, comp_bytes=len(m.comp) + 1, text_cap=m.isize)["status"] == 0
    assert bytes(big.cpu().numpy()[:m.isize]) == m.text
    assert bool((d_text.cpu() == FILL).all())          # ... the valid first member of the third call included: nothing ran
    res = ctx.bgzf_inflate(d_comp, [ok], d_text, comp_bytes=len(m.comp), text_cap=m.isize)
    assert res["status"] == 0 and bytes(d_text.cpu().numpy()[:m.isize]) == m.text
