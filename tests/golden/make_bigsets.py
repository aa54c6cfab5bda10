"""Generate tests/golden/bigsets_pe/: an index whose transcript sets have 129 to 4400 members, with the UNMODIFIED reference
(oracle/_ref, `make -C oracle ref`).  Run in the build container only:

    python tests/golden/make_bigsets.py

Why: EC resolution (kallisto_amd/csrc/kamd_ec.hip) takes another code path for every size class of a tuple's smallest set and of its
other sets -- all pairs in registers up to 16 members, the LDS kernel k_resolve_big<1024> for 17..1024, k_resolve_big<4096> for
1025..4096, a plain path beyond, bitmaps instead of binary search for sets of more than 128 members, a wavefront copy for dense
sets of more than 64 -- and no other fixture has a set of more than 78 members.

The transcriptome is synthetic: 4400 transcripts, each a distinct 12-base head followed by the 40-base segments of the "families"
it belongs to, in the same family order in every transcript.  A family's segment is shared by its member set, so the 10 k-mers
inside a segment carry exactly that set; the junctions between neighbouring segments carry further sets (the members of both
families that have no family in between).  Families exist at every threshold of the kernels, one on each side:
16/17 (RES_BIG_MIN), 64/65 (k_cand_singles' wavefront copy), 128/129 (BM_MIN_MEMBERS), 1024/1025 (RB_CAND_BIG), 4096/4097
(RB_CAND_HUGE).

The directory holds
    index.idx.gz                      `kallisto index -k 31` (reference binary), gzipped: tests gunzip it into a temporary directory
    reads_1.txt.gz reads_2.txt.gz     one read per line
    expected_pe.txt.gz expected_se.txt.gz   oracle/_ref/dump_ec quant (NPROC / EC / FLEN / TR lines), as for the other cases, but gzipped:
                                      a TR line per transcript makes each file 5000 lines; common.load_expected reads either form
    case.json                         how the case was made, the histogram of the set sizes
A second run gives the same reads and the same expected_*.txt.gz byte for byte; the reference's index file differs by a few hundred bytes
from run to run (case.json's index_bytes with it) while holding the same sets.
It is NOT one of tests/common.CASES (no index.idx, no cli_* directories): tests/bigsets.py loads it.
"""
from __future__ import annotations

import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from kallisto_amd import synth  # noqa: E402
from tests import bigsets  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
KALLISTO = os.path.join(REF, "kallisto")
DUMP = os.path.join(REF, "dump_ec")
NAME = "bigsets_pe"
K = 31
SEG = K + 9          # bases of a family's segment: 10 k-mers inside it, 30 across each junction
HEAD = 12
T = 4400
N_HUB = 300
N_PAIRS = 2500
READ_LEN = 75
BOUNDARY = (16, 17, 64, 65, 128, 129, 1024, 1025, 4096, 4097)
SE = ["--single", "-l", "130", "-s", "15"]
VARIANTS = {"pe": [], "se": SE}


def families(rng):
    """member sets, in the order their segments take in a transcript"""
    fams = [np.arange(0, 4300), np.arange(60, 4400),                       # two sets beyond 4096; they meet in 60..4299
            np.arange(0, 2500), np.arange(1500, 4000), np.arange(2600, 4400),   # 1025..4096: overlapping, and disjoint (first and third)
            rng.choice(T, 1300, replace=False)]
    for n in (4097, 4096, 1025, 1024):
        fams.append(rng.choice(T, n, replace=False))
    # 129..1024: ranges that are disjoint / share more than 64 members by construction, and random ones
    fams += [np.arange(100, 500), np.arange(420, 1020), np.arange(2000, 2300), np.arange(3000, 3900)]
    for _ in range(6):
        fams.append(rng.choice(T, int(rng.integers(129, 1025)), replace=False))
    for n in (129, 128, 65, 64, 17, 16):
        fams.append(rng.choice(T, n, replace=False))
    for _ in range(20):
        fams.append(rng.choice(T, int(rng.integers(17, 129)), replace=False))
    for _ in range(40):
        fams.append(rng.choice(T, int(rng.integers(2, 17)), replace=False))
    # short ranges next to each other: sets of 65..128 members that share more than 64 (their junction is range(4010, 4100))
    fams += [np.arange(4000, 4100), np.arange(4010, 4120)]
    # N_HUB families of 17 members that all hold the same 16 transcripts (the "hub" group, inside the four large ranges) and one more each:
    # hundreds of distinct sets with a common member -- tuples of more than 256 sets whose intersection is not empty -- at the price of
    # N_HUB junction kinds only (the group's transcripts carry the same run of segments; that junction's set is the group itself: 16 members)
    hub = np.sort(rng.choice(np.arange(1600, 2400), 16, replace=False))
    rest = np.setdiff1d(np.arange(T), hub)
    for x in rng.choice(rest, N_HUB, replace=False):
        fams.append(np.append(hub, x))
    return [np.sort(f) for f in fams]


def transcriptome(seed=5):
    rng = np.random.default_rng(seed)
    fams = families(rng)
    segs = [synth._ACGT[rng.integers(0, 4, SEG)] for _ in fams]
    member = [[] for _ in range(T)]
    for f, mem in enumerate(fams):
        for t in mem:
            member[int(t)].append(f)
    heads, seqs = set(), []
    for t in range(T):
        while True:
            h = synth._ACGT[rng.integers(0, 4, HEAD)]
            if h.tobytes() not in heads:
                heads.add(h.tobytes())
                break
        seqs.append(np.concatenate([h] + [segs[f] for f in member[t]]))
    return seqs, [len(f) for f in fams]


def write_gz(path, data):
    """gzip without a name or a time stamp in the header: the same input gives the same file"""
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0, filename="") as f:
        f.write(data)


def write_lines(path, reads):
    write_gz(path, b"".join(bytes(r) + b"\n" for r in reads))


def write_fastq(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            s = bytes(r)
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))


def main():
    if not (os.path.exists(KALLISTO) and os.path.exists(DUMP)):
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` in the build container")
    d = os.path.join(HERE, NAME)
    os.makedirs(d, exist_ok=True)
    seqs, fam_sizes = transcriptome()
    # reads and fragments shorter than the transcripts: 75-base mates, fragments of about 130 bases (a transcript of two families has 92)
    r1, r2 = synth.simulate_reads(seqs, N_PAIRS, READ_LEN, paired=True, frag_mean=130, frag_sd=15, err=0.002, n_frac=0.002, seed=51, expr_sigma=1.0)
    r1 = [bytes(x) for x in r1]
    r2 = [bytes(x) for x in r2]
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "b.fa")
        synth.write_fasta(fa, seqs)
        idx = os.path.join(tmp, "index.idx")
        subprocess.check_call([KALLISTO, "index", "-k", str(K), "-i", idx, fa], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(idx, "rb") as fi:
            write_gz(os.path.join(d, "index.idx.gz"), fi.read())
        write_lines(os.path.join(d, "reads_1.txt.gz"), r1)
        write_lines(os.path.join(d, "reads_2.txt.gz"), r2)
        f1, f2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        write_fastq(f1, r1)
        write_fastq(f2, r2)
        for vname, extra in VARIANTS.items():
            files = [f1] if "--single" in extra else [f1, f2]
            out = subprocess.run([DUMP, "quant", idx, "1", *extra, *files], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
            write_gz(os.path.join(d, f"expected_{vname}.txt.gz"), out)
        from oracle import oracle as O
        sets = bigsets.sets_of_oracle_index(O.Index(idx))
        raw_bytes = os.path.getsize(idx)
    hist = bigsets.size_histogram(sets.sizes)
    meta = {"name": NAME, "k": K, "paired": True, "n": len(r1), "variants": VARIANTS, "targets": T, "n_sets": int(len(sets.sizes)),
            "largest_set": int(sets.sizes.max()), "set_size_histogram": hist, "boundary_sizes": list(BOUNDARY), "family_sizes": fam_sizes,
            "index_bytes": raw_bytes,
            "note": f"{T} transcripts = a 12-base head + the 40-base segments of the families they belong to (seed 5, make_bigsets.py); "
                    f"simulate_reads({N_PAIRS} PE-{READ_LEN}, fragments 130 +- 15, err 0.2 %, seed=51)",
            "reference": "pachterlab/kallisto v0.51.1 via oracle/_ref/dump_ec (unmodified sources)"}
    with open(os.path.join(d, "case.json"), "w") as f:      # one key per line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in meta.items()) + "\n}\n")
    for fn in sorted(os.listdir(d)):
        print(fn, os.path.getsize(os.path.join(d, fn)))
    print(hist)


if __name__ == "__main__":
    main()
