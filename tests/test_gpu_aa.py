"""Translated search (`bus --aa`) on the GPU: kamd_cfc_frames against the CPU translation, kamd_pseudoalign_aa + kamd_ec_finalize and the
`bus --aa` front-end against the reference's output on tests/golden/aa_bulk (tests/golden/make_aa_bulk.py, oracle/_ref/kallisto at -t 1)."""
import collections
import gzip
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tests import aa_common as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
BUS_DTYPE = np.dtype([("bc", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])


@pytest.fixture(scope="module")
def ka():
    import kallisto_amd
    return kallisto_amd


@pytest.fixture(scope="module")
def contexts(ka):
    """one context per fixture index, and the fixture's reads packed once on each"""
    fx = A.fixture()
    out = {}
    for v in A.VARIANTS:
        ctx = ka.Context(0)
        ctx.upload(ka.Index(fx[v]["index"]))
        out[v] = (ctx,) + tuple(ctx.pack_reads_host(fx["reads"]))
    return out


# ---- frames ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_reads():
    base = A.frame_test_reads(random.Random(5))
    reads = [base[i % len(base)] for i in range(1000)]
    ow, ol, max_len = A.emu_frames(reads)   # the CPU translation, once
    return reads, ow, ol, max_len


@pytest.mark.parametrize("n", [1, 9, 10, 11, 63, 64, 65, 1000])
def test_cfc_frames_equal_the_cpu_translation(contexts, frame_reads, n):
    reads, ow, ol, max_len = frame_reads
    ctx = contexts["plain"][0]
    words, lens, ml = ctx.pack_reads_host(reads[:n], max_len)
    assert ml == max_len
    gw, gl = ctx.cfc_frames(words, lens, n, max_len)
    rec = len(ow) // (6 * len(reads))
    assert np.array_equal(gl.cpu().numpy().view(np.uint16), ol[:6 * n])
    assert np.array_equal(gw.cpu().numpy().view(np.uint32), ow[:6 * n * rec])


def _run(ctx, words, lens, n, max_len, batch):
    rec = words.numel() // max(n, 1)
    ctx.reset()
    for a in range(0, n, batch):
        b = min(n, a + batch)
        ctx.pseudoalign_aa(words[a * rec:b * rec], lens[a:b], b - a, max_len)
    ecs = ctx.finalize()
    return {k: c for k, c in ecs.multiset().items() if c}, ctx.aa_stats()


def test_frame_window_boundaries(contexts):
    """k = 31: a frame needs 33 translated bases, so frames 0, 1 and 2 of a read get their first window at l = 33, 34 and 35"""
    fx = A.fixture()
    ctx = contexts["plain"][0]
    prot = open(os.path.join(A.GOLD, "proteins.fa")).read().split("\n")[1]
    nt = "".join(A.codon_of(A.CODE.index(a)) for a in prot[:14])
    reads = []
    for shift in range(3):
        for ln in (32, 33, 34, 35):
            r = ("GT"[:shift] + nt)[:ln]
            reads += [r.encode(), r.encode()[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))]
    e = A.emu_pseudoalign(fx["plain"]["index"], reads)
    fwd = e["outcome"][0::2].reshape(3, 4)
    for shift in range(3):   # the forward read in the frame of its shift, from 33 + shift bases on
        assert [int(x) for x in fwd[shift]] == [shift if ln >= 33 + shift else -2 for ln in (32, 33, 34, 35)]
    words, lens, max_len = ctx.pack_reads_host(reads)
    ms, st = _run(ctx, words, lens, len(reads), max_len, len(reads))
    assert ms == e["multiset"]
    assert st["n_winner"] == [int((e["outcome"] == f).sum()) for f in range(6)]
    assert st["n_all_empty"] == int((e["outcome"] == -2).sum()) and st["n_rejected_offlist"] == 0
    for i, r in enumerate(reads):   # and read by read
        ms1, st1 = _run(ctx, words[i * (words.numel() // len(reads)):], lens[i:], 1, max_len, 1)
        assert st1["n_winner"] == [int(e["outcome"][i] == f) for f in range(6)], r


# ---- pseudoalignment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [0, 1, 10, 700])
@pytest.mark.parametrize("variant", A.VARIANTS)
def test_pseudoalign_aa_gives_the_reference_classes(contexts, variant, batch):
    fx = A.fixture()
    v = fx[variant]
    ctx, words, lens, max_len = contexts[variant]
    n = len(fx["reads"])
    for rep in range(2 if batch in (0, 700) else 1):   # (the second run: the same after reset())
        ms, st = _run(ctx, words, lens, n, max_len, batch or n)
        assert ms == v["multiset"]
        assert st["n_processed"] == n == v["run_info"]["n_processed"]
        assert st["n_frame_clashes"] == v["run_info"]["n_frame_clashes"]
        assert sum(st["n_winner"]) == v["run_info"]["n_pseudoaligned"] == sum(ms.values())
        assert st["n_rejected_offlist"] == v["case"]["emu_rejected_offlist"]
        assert st["n_rejected_offlist"] + st["n_all_empty"] + sum(st["n_winner"]) == n
        assert sum(c for s, c in ms.items() if len(s) == 1) == v["run_info"]["n_unique"]


# ---- front-end ------------------------------------------------------------------------------------------------------
def _read_bus(path):
    b = open(path, "rb").read()
    assert b[:4] == b"BUS\0"
    ver, bclen, umilen, tlen = struct.unpack("<IIII", b[4:20])
    return [ver, bclen, umilen], np.frombuffer(b[20 + tlen:], dtype=BUS_DTYPE)


def _bus(tmp_path, variant, name, *flags):
    fx = A.fixture()
    fq = str(tmp_path / "reads.fq")
    if not os.path.exists(fq):
        A.write_fastq(fq, fx["reads"])
    out = str(tmp_path / name)
    p = subprocess.run([EXE, "bus", "--aa", "-x", "bulk", "-i", fx[variant]["index"], "-o", out, "-t", "5", "--batch-size", "700", *flags, fq],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, KAMD_FASTQ_CHUNK="3000"))
    return p, out


def _bus_lines(out):
    hdr, rec = _read_bus(os.path.join(out, "output.bus"))
    ecs = A.read_ec(os.path.join(out, "matrix.ec"))
    assert len(set(ecs)) == len(ecs)
    return hdr, ["%d\t%d\t%s" % (bc, n, ",".join(map(str, s))) for bc, s, n in sorted((int(r["bc"]), ecs[int(r["ec"])], int(r["count"])) for r in rec)], set(ecs)


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_bus_aa_matches_reference(variant, tmp_path):
    assert os.path.exists(EXE), "build kallisto_amd_quant with `make -C kallisto_amd/csrc all`"
    fx = A.fixture()
    gold = os.path.join(A.GOLD, variant)
    p, out = _bus(tmp_path, variant, "bus")
    assert p.returncode == 0, p.stderr.decode()
    hdr, lines, ecs = _bus_lines(out)
    assert hdr == fx[variant]["case"]["bus_header"]
    assert lines == gzip.open(os.path.join(gold, "bus_expected.txt.gz"), "rt").read().split("\n")[:-1]
    assert ecs <= set(A.read_ec(os.path.join(gold, "matrix.ec.gz")))   # (the reference lists the index's classes too; here: the ones that occur)
    text = open(os.path.join(out, "run_info.json")).read()
    info = json.loads(text)
    for k, val in fx[variant]["run_info"].items():
        assert info[k] == val, k
    assert list(info)[-2:] == ["call", "n_frame_clashes"] and text.rstrip().endswith('"n_frame_clashes": %d\n}' % info["n_frame_clashes"])
    # --paired is ignored with the reference's message, and changes nothing
    p2, out2 = _bus(tmp_path, variant, "bus_paired", "--paired")
    assert p2.returncode == 0, p2.stderr.decode()
    assert b"[bus] --paired ignored; --aa only supports single-end reads" in p2.stderr
    assert _bus_lines(out2)[:2] == (hdr, lines)
    assert {k: v for k, v in json.load(open(os.path.join(out2, "run_info.json"))).items() if k not in ("start_time", "call")} == \
           {k: v for k, v in info.items() if k not in ("start_time", "call")}


@pytest.mark.parametrize("flag,msg", [("--union", b"--union is not compatible with this mode"), ("--no-jump", b"--no-jump is not compatible with this mode")])
def test_bus_aa_refuses_union_and_no_jump(flag, msg, tmp_path):
    p, _ = _bus(tmp_path, "plain", "bus", flag)
    assert p.returncode == 1 and msg in p.stderr
