"""Rate of the translated search (kamd_pseudoalign_aa) on a synthetic protein set, beside the reference's `kallisto bus --aa -t 16` on the
same input when oracle/_ref/kallisto is present.  Not part of bench.py: the flagship line does not touch this path.

    python tools/aa_rate.py [--proteins 2000] [--reads 1000000] [--read-len 150] [--repeats 5] [--out profiles/aa_rate.md]

The index of an amino-acid FASTA can only be built by the reference (`kallisto index --aa`); without the binary the proteins and the
index of tests/golden/aa_bulk are used (a 49-target index: a statement about overheads, not about the matcher).  Times are HIP events
around kamd_pseudoalign_aa over warmed-up repeats, and the library's own events around its two kernels (kamd_aa_stats)."""
import argparse
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import aa_common as A  # noqa: E402

KALLISTO = os.path.join(ROOT, "oracle", "_ref", "kallisto")
AAS = "ACDEFGHIKLMNPQRSTVWY"


def make_proteins(rng, n):
    out = []
    while len(out) < n:
        base = [rng.choice(AAS) for _ in range(300)]
        for copy in range(4):
            p = list(base)
            for _ in range(0 if copy == 0 else 10):
                p[rng.randrange(300)] = rng.choice(AAS)
            out.append("".join(p))
    return out[:n]


def make_reads(rng, proteins, n, ln):
    by_aa = {}
    for c in range(64):
        by_aa.setdefault(A.CODE[c], []).append(A.codon_of(c))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    # (two random back-translations per protein, reads are windows of them: the translated frames are what the matcher sees)
    nts = [["".join(rng.choice(by_aa[x]) for x in p).encode() for _ in range(2)] for p in proteins]
    noise = bytes(rng.choice(b"ACGT") for _ in range(1 << 20))
    reads = []
    for _ in range(n):
        if rng.random() < 0.1:
            a = rng.randrange(0, len(noise) - ln)
            reads.append(noise[a:a + ln])
            continue
        nt = rng.choice(rng.choice(nts))
        a = rng.randrange(0, len(nt) - ln)
        r = nt[a:a + ln]
        reads.append(r[::-1].translate(comp) if rng.random() < 0.5 else r)
    return reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=2000)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aa_rate.md"))
    args = ap.parse_args()
    import torch
    import kallisto_amd as ka
    if not torch.cuda.is_available():
        sys.exit("aa_rate.py measures on the GPU: no HIP device visible")
    rng = random.Random(7)
    lines = ["# Translated search (`bus --aa`): measured rate", ""]
    with tempfile.TemporaryDirectory() as tmp:
        have_ref = os.path.exists(KALLISTO)
        if have_ref:
            proteins = make_proteins(rng, args.proteins)
            fa = os.path.join(tmp, "proteins.fa")
            with open(fa, "w") as f:
                f.write("".join(">p%d\n%s\n" % (i, p) for i, p in enumerate(proteins)))
            idx = os.path.join(tmp, "aa.idx")
            subprocess.run([KALLISTO, "index", "--aa", "-t", "16", "-i", idx, fa], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        else:
            proteins = [l.strip() for l in open(os.path.join(A.GOLD, "proteins.fa")) if not l.startswith(">")]
            proteins = [p for p in proteins if len(p) >= 300]
            idx = os.path.join(A.GOLD, "index_plain.idx")
        reads = make_reads(rng, proteins, args.reads, args.read_len)
        index = ka.Index(idx)
        K = int(index.view.k)
        ctx = ka.Context(0)
        ctx.upload(index)
        words, lens, max_len = ctx.pack_reads_host(reads)
        n = len(reads)
        times, tr, ma = [], [], []
        for rep in range(2 + args.repeats):   # two warm-up runs
            ctx.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            ctx.pseudoalign_aa(words, lens, n, max_len)
            e1.record(ctx.stream)
            e1.synchronize()
            if rep >= 2:
                st = ctx.aa_stats()
                times.append(e0.elapsed_time(e1)); tr.append(st["translate_ms"]); ma.append(st["match_ms"])
        ecs = ctx.finalize()
        st = ctx.aa_stats()
        med = lambda x: sorted(x)[len(x) // 2]
        lines += ["Input: %d proteins of 300 residues (%s), k = %d; %d reads of %d nt (nine in ten back-translated protein windows on either strand, one in ten random)."
                  % (len(proteins), "families of four mutated copies, index by the reference's `index --aa`" if have_ref else "the fixture of tests/golden/aa_bulk",
                     K, n, args.read_len), "",
                  "| what | ms (median of %d, min .. max) | reads/s | frames/s |" % args.repeats, "|---|---|---|---|",
                  "| `kamd_pseudoalign_aa`, one call (HIP events; both kernels, record absorption, the host read-backs between them) | %.2f (%.2f .. %.2f) | %.3g | %.3g |"
                  % (med(times), min(times), max(times), n / med(times) * 1e3, 6 * n / med(times) * 1e3),
                  "| of which frame translation `k_aa_translate` | %.2f (%.2f .. %.2f) | %.3g | %.3g |" % (med(tr), min(tr), max(tr), n / med(tr) * 1e3, 6 * n / med(tr) * 1e3),
                  "| of which match and decide `k_aa_match` | %.2f (%.2f .. %.2f) | %.3g | %.3g |" % (med(ma), min(ma), max(ma), n / med(ma) * 1e3, 6 * n / med(ma) * 1e3), "",
                  "Outcome: %d of %d reads pseudoaligned into %d classes, %d rejected for an off-list member, %d with all frames empty, %d frame clashes; winners per frame %s."
                  % (sum(st["n_winner"]), n, len(ecs.counts), st["n_rejected_offlist"], st["n_all_empty"], st["n_frame_clashes"], st["n_winner"]), ""]
        if have_ref:
            fq = os.path.join(tmp, "reads.fq")
            A.write_fastq(fq, reads)
            t0 = time.time()
            subprocess.run([KALLISTO, "bus", "--aa", "-x", "bulk", "-t", "16", "-i", idx, "-o", os.path.join(tmp, "ref_out"), fq], check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            wall = time.time() - t0
            lines += ["Reference on the same reads: `kallisto bus --aa -x bulk -t 16`, wall clock of the whole command (index load, FASTQ parsing and output included): %.2f s, %.3g reads/s."
                      % (wall, n / wall), ""]
        else:
            lines += ["Reference: not measured (oracle/_ref/kallisto is not built here).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
