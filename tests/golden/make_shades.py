"""Generate tests/golden/shades_pe/: an index with shades (targets named <base>_shade_<variant>, kallisto 0.51's allele-aware classes) and
what the UNMODIFIED reference (oracle/_ref, `make -C oracle ref`) computes on it.  Run in the build container only:

    python tests/golden/make_shades.py

The transcriptome is synthetic, k = 31.  A base transcript is a distinct 14-base head followed by the 110-base segments of the "families"
it belongs to (the same family order in every transcript), so a family's segment carries the family's member set; families exist on each
side of the thresholds of the EC kernels: 16/17, 64/65, 128/129, 1024/1025, and a dozen small ones.  A shade is a 91-base window of its
base transcript around one substituted base, placed DIRECTLY AFTER its base in the FASTA, so shade ids interleave with the ids of the
other targets: the 31 k-mers over the substitution belong to the shade alone, the 30 k-mers of the flanks to the shade and to whatever
holds that text.  Every family has shades inside its segment for several members; in the families of 16 and of 128 two members have a
shade at the same place with the same base (two paralogs, one variant: those k-mers carry both shades).  In the families of 17, 129 and
1025 one member carries 20 shades 6 bases apart inside the family's (260-base) segment: cores of more than 16, 128 and 1024 members beside
more than 16 shades; the family of 1060 has no shades (a second shade-free set with a core above 1024).  One long transcript, in no
family, carries 24 shades 6 bases apart: a read from it meets more than 12 distinct sets (the overflow pass) whose shades unite to more
than 16.

6 000 pairs of 90 bases, fragments of about 180: from a base transcript or from a haplotype with one of its variants, 10 % with one mate
replaced by random bases (orphans: r = u1), 10 % with one substituted base.

The directory holds
    index.idx.gz                      `kallisto index -k 31` (reference binary), gzipped: tests gunzip it into a temporary directory
    reads_1.txt.gz reads_2.txt.gz     one read per line
    expected_<variant>.txt.gz         oracle/_ref/dump_ec quant <index> 1 ... (NPROC / EC / FLEN / TR lines) for pe, pe_fr, pe_rf, pe_union,
                                      pe_nojump, se_so
    bus_pe/                           `kallisto bus -t 1 -x bulk --paired`: bus_expected.txt.gz (lines "barcode<TAB>count<TAB>t1,t2,..."), flens.txt,
                                      run_info.json (without start_time / call)
    case.json                         how the case was made; counted from the reference's output and the index: the histogram of the cores'
                                      sizes, the shades, the pairs with a shade in their class, with an orphan mate, with more than 12 sets,
                                      the largest union of shades
It is NOT one of tests/common.CASES: tests/shades.py loads it.
"""
from __future__ import annotations

import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from kallisto_amd import synth  # noqa: E402
from tests import bigsets, shades  # noqa: E402
from tests.golden.make_bigsets import write_fastq, write_gz, write_lines  # noqa: E402
from tests.golden.make_bus_tcc import bus_lines, read_bus, read_ec  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
KALLISTO = os.path.join(REF, "kallisto")
DUMP = os.path.join(REF, "dump_ec")
NAME = shades.NAME
K = 31
HEAD, SEG, WIN = 14, 110, 45
N_BASE = 1100
FAMILY_SIZES = (1060, 1025, 1024, 129, 128, 65, 64, 17, 16)
PLAIN_FAMILY = 1060                 # no shades: with the shade-free stretch of the 1025 family's segment a second set without shades whose core exceeds 1024
STRETCH_FAMILIES = (1025, 129, 17)  # one member of each carries N_STRETCH shades LONG_STEP bases apart inside the family's (longer) segment
N_STRETCH, SEG_STRETCH, STRETCH_AT = 20, 260, 50
N_SMALL = 12
SHADE_OFFSETS = (48, 55, 62)        # of a family's three shaded members, inside the segment
N_LONG_SHADES, LONG_STEP, LONG_LEN = 24, 6, 500
N_PAIRS, READ_LEN = 6000, 90
VARIANTS = {"pe": [], "pe_fr": ["--fr"], "pe_rf": ["--rf"], "pe_union": ["--union"], "pe_nojump": ["--no-jump"],
            "se_so": ["--single", "-l", "200", "-s", "20", "--single-overhang"]}
BUS_FLAGS = ["--paired"]


def other_base(rng, b):
    return int(rng.choice([x for x in b"ACGT" if x != b]))


def transcriptome(seed=7):
    """[(name, sequence)] in FASTA order, and per base transcript the list of (position, substituted base) of its shades"""
    rng = np.random.default_rng(seed)
    fams = [np.sort(rng.choice(N_BASE, n, replace=False)) for n in FAMILY_SIZES]
    fams += [np.sort(rng.choice(N_BASE, int(rng.integers(2, 9)), replace=False)) for _ in range(N_SMALL)]
    segs = [synth._ACGT[rng.integers(0, 4, SEG_STRETCH if len(f) in STRETCH_FAMILIES else SEG)] for f in fams]
    member = [[] for _ in range(N_BASE)]
    for f, mem in enumerate(fams):
        for t in mem:
            member[int(t)].append(f)
    heads, base = set(), []
    for t in range(N_BASE):
        while True:
            h = synth._ACGT[rng.integers(0, 4, HEAD)]
            if h.tobytes() not in heads:
                heads.add(h.tobytes())
                break
        parts = [h] + [segs[f] for f in member[t]]
        if not member[t]:
            parts.append(synth._ACGT[rng.integers(0, 4, SEG)])
        base.append(np.concatenate(parts))
    variants = [[] for _ in range(N_BASE + 1)]   # (position in the transcript, base)
    seg_start = lambda t, f: HEAD + sum(len(segs[g]) for g in member[t][:member[t].index(f)])
    for f, mem in enumerate(fams):
        if len(mem) == PLAIN_FAMILY:
            continue
        if len(mem) in STRETCH_FAMILIES:          # cores of more than 16 / 128 / 1024 members beside more than 16 shades
            t = int(rng.choice(mem))
            for j in range(N_STRETCH):
                off = STRETCH_AT + LONG_STEP * j
                variants[t].append((seg_start(t, f) + off, other_base(rng, int(segs[f][off]))))
            continue
        chosen = rng.choice(mem, min(3, len(mem)), replace=False)
        paralogs = len(mem) in (16, 128)          # the first two shaded members share place and base
        alt0 = None
        for j, t in enumerate(chosen):
            off = SHADE_OFFSETS[0] if (paralogs and j == 1) else SHADE_OFFSETS[j]
            pos = seg_start(int(t), f) + off
            alt = alt0 if (paralogs and j == 1) else other_base(rng, int(segs[f][off]))
            if j == 0:
                alt0 = alt
            variants[int(t)].append((pos, alt))
    long_tr = np.concatenate([synth._ACGT[rng.integers(0, 4, HEAD)], synth._ACGT[rng.integers(0, 4, LONG_LEN)]])
    base.append(long_tr)
    for j in range(N_LONG_SHADES):
        pos = 150 + LONG_STEP * j
        variants[N_BASE].append((pos, other_base(rng, int(long_tr[pos]))))
    fasta = []
    for t, s in enumerate(base):
        fasta.append((f"t{t}", s))
        for j, (pos, alt) in enumerate(sorted(variants[t])):
            w = s[pos - WIN:pos + WIN + 1].copy()
            w[WIN] = alt
            fasta.append((f"t{t}_shade_v{j}", w))
    return fasta, base, variants, [len(f) for f in fams]


def simulate(base, variants, seed=71):
    rng = np.random.default_rng(seed)
    weight = np.array([1.0 + 12.0 * len(v) for v in variants])
    weight[N_BASE] = 0.08 * weight[:N_BASE].sum()
    weight /= weight.sum()
    r1, r2, n_orphan = [], [], 0
    for _ in range(N_PAIRS):
        t = int(rng.choice(len(base), p=weight))
        s = base[t].copy()
        if variants[t] and rng.random() < 0.6:     # a haplotype with one of the variants
            pos, alt = variants[t][int(rng.integers(len(variants[t])))]
            s[pos] = alt
        flen = int(np.clip(rng.normal(180, 20), READ_LEN + 5, len(s)))
        a = int(rng.integers(0, len(s) - flen + 1))
        frag = s[a:a + flen]
        if rng.random() < 0.5:
            frag = synth.revcomp(frag)
        m = [frag[:READ_LEN].copy(), synth.revcomp(frag[-READ_LEN:]).copy()]
        u = rng.random()
        if u < 0.10:
            m[int(rng.integers(2))] = synth._ACGT[rng.integers(0, 4, READ_LEN)]
            n_orphan += 1
        elif u < 0.20:
            x, p = int(rng.integers(2)), int(rng.integers(READ_LEN))
            m[x][p] = other_base(rng, int(m[x][p]))
        r1.append(bytes(m[0]))
        r2.append(bytes(m[1]))
    return r1, r2, n_orphan


def main():
    if not (os.path.exists(KALLISTO) and os.path.exists(DUMP)):
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` in the build container")
    d = os.path.join(HERE, NAME)
    os.makedirs(os.path.join(d, "bus_pe"), exist_ok=True)
    fasta, base, variants, fam_sizes = transcriptome()
    r1, r2, n_orphan = simulate(base, variants)
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "s.fa")
        with open(fa, "wb") as f:
            for name, s in fasta:
                f.write(b">%s\n%s\n" % (name.encode(), bytes(s)))
        idx = os.path.join(tmp, "index.idx")
        subprocess.check_call([KALLISTO, "index", "-k", str(K), "-i", idx, fa], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(idx, "rb") as fi:
            write_gz(os.path.join(d, "index.idx.gz"), fi.read())
        write_lines(os.path.join(d, "reads_1.txt.gz"), r1)
        write_lines(os.path.join(d, "reads_2.txt.gz"), r2)
        f1, f2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        write_fastq(f1, r1)
        write_fastq(f2, r2)
        em_rounds = {}
        for vname, extra in VARIANTS.items():
            files = [f1] if "--single" in extra else [f1, f2]
            outs = [subprocess.run([DUMP, "quant", idx, th, *extra, *files], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
                    for th in ("1", "4")]
            assert outs[0] == outs[1], f"{vname}: the reference's output differs between 1 and 4 threads"
            # the round the reference's EM stops in, from the reference CLI itself ("... ran for N rounds")
            cli = [a.replace("--fr", "--fr-stranded").replace("--rf", "--rf-stranded") for a in extra]
            q = subprocess.run([KALLISTO, "quant", "-t", "1", "-i", idx, "-o", os.path.join(tmp, "q_" + vname), "--plaintext", *cli, *files],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert q.returncode == 0, q.stderr.decode()
            em_rounds[vname] = int(re.search(r"ran for ([\d,]+) rounds", q.stderr.decode()).group(1).replace(",", ""))
            write_gz(os.path.join(d, f"expected_{vname}.txt.gz"), outs[0])
        bus_out = os.path.join(tmp, "bus")
        p = subprocess.run([KALLISTO, "bus", "-x", "bulk", "-t", "1", "-i", idx, "-o", bus_out, *BUS_FLAGS, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()
        hdr, rec = read_bus(os.path.join(bus_out, "output.bus"))
        ecs = read_ec(os.path.join(bus_out, "matrix.ec"))
        write_gz(os.path.join(d, "bus_pe", "bus_expected.txt.gz"), ("\n".join(bus_lines(rec, ecs)) + "\n").encode())
        info = json.load(open(os.path.join(bus_out, "run_info.json")))
        for k in ("start_time", "call"):
            info.pop(k)
        json.dump(info, open(os.path.join(d, "bus_pe", "run_info.json"), "w"), indent=1)
        with open(os.path.join(bus_out, "flens.txt")) as fi, open(os.path.join(d, "bus_pe", "flens.txt"), "w") as fo:
            fo.write(fi.read())
        # the refused combinations: the reference itself aborts there
        aborts = {}
        for what, extra, files in (("se", ["--single", "-l", "200", "-s", "20"], [f1]), ("pe_l", ["-l", "200", "-s", "20"], [f1, f2])):
            q = subprocess.run([DUMP, "quant", idx, "1", *extra, *files], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            aborts[what] = q.returncode
            assert q.returncode != 0, f"{what}: the reference no longer aborts here; the library refuses this combination because it does"
        # the index as the library's own loader sees it, and the per-pair facts by the per-item logic on the CPU (tests/emu_shade)
        st = shades.stats_of_fixture(idx, r1, r2)
        raw_bytes = os.path.getsize(idx)
    exp = shades.load_expected("pe")
    shade_ids = set(int(x) for x in st["shade_ids"])
    with_shade = sum(c for e, c in exp["ecs"].items() if shade_ids & set(e))
    meta = {"name": NAME, "k": K, "paired": True, "n": len(r1), "variants": VARIANTS, "bus_flags": BUS_FLAGS, "targets": len(fasta),
            "bases": len(base), "n_shades": len(fasta) - len(base), "family_sizes": fam_sizes,
            "core_size_histogram": bigsets.size_histogram(st["core_sizes"]), "largest_core": int(max(st["core_sizes"])),
            "pairs_with_shade_in_class": int(with_shade), "pairs_with_orphan_mate": int(n_orphan),
            "pairs_with_more_than_12_sets": int(st["more_than_12_sets"]), "largest_shade_union": int(st["largest_shade_union"]),
            "classes": {v: len(shades.load_expected(v)["ecs"]) for v in VARIANTS}, "em_rounds": em_rounds,
            "largest_class": max(len(e) for e in exp["ecs"]),
            "reference_exit_status_of_refused_runs": aborts, "index_bytes": raw_bytes, "bus_header": list(hdr),
            "note": f"{len(base)} base transcripts + their shades (seed 7, make_shades.py); {N_PAIRS} PE-{READ_LEN}, fragments 180 +- 20 (seed 71)",
            "reference": "pachterlab/kallisto v0.51.1 via oracle/_ref/dump_ec and oracle/_ref/kallisto bus (unmodified sources), -t 1"}
    with open(os.path.join(d, "case.json"), "w") as f:      # one key per line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in meta.items()) + "\n}\n")
    for root, _, fs in os.walk(d):
        for fn in sorted(fs):
            print(os.path.relpath(os.path.join(root, fn), d), os.path.getsize(os.path.join(root, fn)))
    print({k: v for k, v in meta.items() if k not in ("family_sizes", "variants")})


if __name__ == "__main__":
    main()
