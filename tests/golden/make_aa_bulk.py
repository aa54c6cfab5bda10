"""Golden fixture of the translated search (`bus --aa`), produced by the UNMODIFIED reference (oracle/_ref/kallisto, built by
`make -C oracle ref`) at -t 1.  Run in the build container:  python tests/golden/make_aa_bulk.py

tests/golden/aa_bulk/ keeps
    proteins.fa, host.fa        the amino-acid targets and the host sequences of the D-list
    index_plain.idx             kallisto index --aa -i ... proteins.fa
    index_dlist.idx             kallisto index --aa -d host.fa -i ... proteins.fa
    reads.txt.gz                the reads, one per line (gzipped: 5589 lines of text would drown every diff they appear in)
    <plain|dlist>/bus_expected.txt.gz   the reference's BUS file as sorted lines "barcode<TAB>count<TAB>t1,t2,..."
    <plain|dlist>/matrix.ec.gz          the reference's classes
    <plain|dlist>/run_info.json      its numbers (without start_time / call), n_frame_clashes among them
    case.json                   what was run, and what the CPU emulation (tests/emu_aa) says about the corners the reads aim at

The recipe: 40 random proteins of 300 residues in families of mutated copies; three nucleotide ORFs of 240 nt without a stop in
frames 0, 1 and reverse-complement 0, whose three translations join the protein set (their reads clash across frames); a host of
ORF[:150] + 300 random nt per ORF.  Reads: random back-translations of protein windows (lengths 99, 100, 101, 120, 150, both
strands, offsets 0-2), a fifth with one substituted base (`N` included), a tenth random, ORF windows of 118-120 nt in steps of 3,
and for every host junction windows reaching 0-39 nt past it, both strands."""
import ctypes as C
import gzip
import json
import os
import random
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import aa_common  # noqa: E402

KALLISTO = os.path.join(ROOT, "oracle", "_ref", "kallisto")
OUT = aa_common.GOLD
BUS_DTYPE = np.dtype([("bc", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
AAS = "ACDEFGHIKLMNPQRSTVWY"


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def protein_of(nt):
    return "".join(aa_common.CODE[aa_common.codon_index(nt[i:i + 3])] for i in range(0, len(nt) - len(nt) % 3, 3))


def make_orf(rng, n=240):
    """n random bases without a stop codon in frames 0, 1 and reverse-complement 0"""
    s = [rng.choice("ACGT") for _ in range(n)]
    while True:
        t = "".join(s)
        bad = [i + f for f, u in ((0, t), (1, t[1:])) for i in range(0, len(u) - 2, 3) if protein_of(u[i:i + 3]) == "*"]
        r = revcomp(t)
        bad += [n - 1 - i for i in range(0, n - 2, 3) if protein_of(r[i:i + 3]) == "*"]
        if not bad:
            return t
        for i in bad:
            j = min(max(i + rng.randrange(-2, 3), 0), n - 1)
            s[j] = rng.choice("ACGT")


def back_translate(rng, prot):
    by_aa = {}
    for c in range(64):
        by_aa.setdefault(aa_common.CODE[c], []).append(aa_common.codon_of(c))
    return "".join(rng.choice(by_aa[a]) for a in prot)


def make_inputs(rng):
    proteins, orfs = [], []
    for fam in range(8):
        base = [rng.choice(AAS) for _ in range(300)]
        for copy in range(5):
            p = list(base)
            for _ in range(0 if copy == 0 else 12):
                p[rng.randrange(300)] = rng.choice(AAS)
            proteins.append(("fam%d_%d" % (fam, copy), "".join(p)))
    for o in range(3):
        orf = make_orf(rng)
        orfs.append(orf)
        for name, nt in (("f0", orf), ("f1", orf[1:]), ("r0", revcomp(orf))):
            proteins.append(("orf%d_%s" % (o, name), protein_of(nt)))
    host = [("host%d" % o, orf[:150] + "".join(rng.choice("ACGT") for _ in range(300))) for o, orf in enumerate(orfs)]
    reads = []
    for name, p in proteins[:40]:
        for _ in range(70):
            ln = rng.choice((99, 100, 101, 120, 150))
            a = rng.randrange(0, 300 - ln // 3 - 2)
            nt = back_translate(rng, p[a:a + ln // 3 + 2])
            off = rng.randrange(3)
            r = nt[off:off + ln]
            if rng.random() < 0.5:
                r = revcomp(r)
            if rng.random() < 0.2:
                i = rng.randrange(len(r))
                r = r[:i] + rng.choice("ACGTN") + r[i + 1:]
            reads.append(r)
    for _ in range(len(reads) // 9):
        reads.append("".join(rng.choice("ACGT") for _ in range(rng.choice((99, 100, 101, 120, 150)))))
    for orf in orfs:
        for ln in (118, 119, 120):
            for a in range(0, 240 - ln + 1, 3):
                reads.append(orf[a:a + ln])
                reads.append(revcomp(orf[a:a + ln]))
    for _, h in host:
        for ln in (118, 119, 120):
            for past in range(40):
                a = 150 + past - ln
                reads.append(h[a:a + ln])
                reads.append(revcomp(h[a:a + ln]))
    # chimeras, in frame on both sides of the joint.  (a) ORF + ORF / protein at total lengths 118-121: in a frame whose length is
    # no multiple of 3 the first hit's unitig reaches past the read's end, so the jump clamp (which takes the untranslated
    # length) decides whether the second half is looked at.  (b) ORF or protein + a window over a host junction: two on-list
    # classes that do not intersect, then a D-list k-mer -- the frame intersection returns early or not, by unitig id.
    sources = orfs + [back_translate(rng, p) for _, p in proteins[0:40:5]]
    for x in sources:
        for y in orfs:
            if x is y:
                continue
            for ln in (118, 119, 120, 121):
                a, b = 3 * rng.randrange(0, 40), 3 * rng.randrange(0, 50)
                r = x[a:a + 60] + y[b:b + ln - 60]
                reads.append(r)
                reads.append(revcomp(r))
    for x in sources:
        for o, (_, h) in enumerate(host):
            if x is orfs[o]:
                continue
            for past in range(3, 40, 3):
                a = 3 * rng.randrange(0, 40)
                r = x[a:a + 48] + h[150 - 48:150 + past]
                reads.append(r)
                reads.append(revcomp(r))
    rng.shuffle(reads)
    return proteins, host, reads


def write_fasta(path, recs):
    with open(path, "w") as f:
        for n, s in recs:
            f.write(">%s\n%s\n" % (n, s))


def read_bus(path):
    b = open(path, "rb").read()
    assert b[:4] == b"BUS\0"
    ver, bclen, umilen, tlen = struct.unpack("<IIII", b[4:20])
    return [ver, bclen, umilen], np.frombuffer(b[20 + tlen:], dtype=BUS_DTYPE)


def write_gz(path, data):
    """gzip without a name or a time stamp: the same bytes on every regeneration"""
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0) as f:
        f.write(data)


def run(*cmd):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()


def main():
    if not os.path.exists(KALLISTO):
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` in the build container")
    rng = random.Random(20260207)
    proteins, host, reads = make_inputs(rng)
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    write_fasta(os.path.join(OUT, "proteins.fa"), proteins)
    write_fasta(os.path.join(OUT, "host.fa"), host)
    write_gz(os.path.join(OUT, "reads.txt.gz"), ("\n".join(reads) + "\n").encode())
    run(KALLISTO, "index", "--aa", "-t", "1", "-i", os.path.join(OUT, "index_plain.idx"), os.path.join(OUT, "proteins.fa"))
    run(KALLISTO, "index", "--aa", "-t", "1", "-d", os.path.join(OUT, "host.fa"), "-i", os.path.join(OUT, "index_dlist.idx"), os.path.join(OUT, "proteins.fa"))
    case = {"n_reads": len(reads), "reference": "pachterlab/kallisto v0.51.1, oracle/_ref/kallisto (unmodified sources), bus --aa -x bulk -t 1",
            "variants": {}}
    with tempfile.TemporaryDirectory() as tmp:
        fq = os.path.join(tmp, "reads.fq")
        aa_common.write_fastq(fq, [r.encode() for r in reads])
        for variant in aa_common.VARIANTS:
            idx = os.path.join(OUT, "index_%s.idx" % variant)
            outs = []
            for rep in range(2):   # (the output is deterministic at -t 1: checked on every regeneration)
                bus_out = os.path.join(tmp, "bus_%s_%d" % (variant, rep))
                run(KALLISTO, "bus", "--aa", "-x", "bulk", "-t", "1", "-i", idx, "-o", bus_out, fq)
                outs.append(open(os.path.join(bus_out, "output.bus"), "rb").read() + open(os.path.join(bus_out, "matrix.ec"), "rb").read())
            assert outs[0] == outs[1]
            dst = os.path.join(OUT, variant)
            os.makedirs(dst)
            hdr, rec = read_bus(os.path.join(bus_out, "output.bus"))
            ecs = aa_common.read_ec(os.path.join(bus_out, "matrix.ec"))
            lines = {}
            for r in rec:
                assert int(r["umi"]) == 2 ** 64 - 1 and int(r["flags"]) == 0
                k = (int(r["bc"]), ecs[int(r["ec"])])
                lines[k] = lines.get(k, 0) + int(r["count"])
            write_gz(os.path.join(dst, "bus_expected.txt.gz"), "".join("%d\t%d\t%s\n" % (bc, n, ",".join(map(str, s))) for (bc, s), n in sorted(lines.items())).encode())
            write_gz(os.path.join(dst, "matrix.ec.gz"), open(os.path.join(bus_out, "matrix.ec"), "rb").read())
            info = json.load(open(os.path.join(bus_out, "run_info.json")))
            for k in ("start_time", "call"):
                info.pop(k)
            json.dump(info, open(os.path.join(dst, "run_info.json"), "w"), indent=1)
            # the corners the reads aim at, counted by the CPU emulation of the per-item logic
            emu = aa_common.emu_pseudoalign(idx, [r.encode() for r in reads], diag=True)
            case["variants"][variant] = {
                "bus_header": hdr, "n_records_reference": int(len(rec)), "n_frame_clashes": int(info["n_frame_clashes"]),
                "emu_rejected_offlist": int((emu["outcome"] == -1).sum()),
                "emu_reads_changed_without_step1": int(emu["diag"][2]),
                "emu_reads_class_list_changed_by_translated_clamp": int(emu["diag"][1]),
                "emu_reads_early_return_before_offlist_set": int(emu["diag"][0]),
            }
            print(variant, case["variants"][variant], {k: info[k] for k in ("n_processed", "n_pseudoaligned", "n_unique")})
    json.dump(case, open(os.path.join(OUT, "case.json"), "w"), indent=1)
    assert case["variants"]["dlist"]["emu_reads_changed_without_step1"] >= 100
    assert case["variants"]["dlist"]["n_frame_clashes"] >= 100


if __name__ == "__main__":
    main()
