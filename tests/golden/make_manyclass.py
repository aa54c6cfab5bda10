"""Generate tests/golden/manyclass_pe/: reads that meet 2 to several hundred (unitig, set) classes each, on an index built by the
UNMODIFIED reference (oracle/_ref, `make -C oracle ref`).  Run in the build container only:

    python tests/golden/make_manyclass.py

Why: an item with more than eight distinct classes leaves kernel A's first pass unfinished (kallisto_amd/csrc/kamd_match.hip).  It goes
through the matcher again with an append-only list of 192 entries, k_classify_long ranks the list three entries per lane, and an item
whose list overflows again goes to the straight-line kernel.  The other fixtures' items append 31 classes at the most, so no test of
theirs reaches a lane's second or third entry, the 192 / 193 edge or the hand-over.  The reads here are placed by hand to hit them.

The transcriptome is synthetic, k = 31.  Five "spines" carry short side transcripts that cut them into unitigs of one to three k-mers:
  dense   a branch every 2..3 bases that shares the 40 bases in front of its branch point (10 k-mers) and then diverges: every branch
          point ends a unitig, every branch start changes the set -- neighbouring classes carry distinct sets.  The reverse complement of
          its first 430 bases is a transcript too (sets of mixed sense: the strand filter changes them), and a second spine shares 320
          bases of it (intersections of more than one transcript).
  quiet   a branch every 2 bases that shares 30 bases only: no common k-mer, so the fork ends a unitig and the set stays -- hundreds of
          classes over five sets (the spine and four transcripts that are stretches of it).
  aba     a spine that repeats a 170-base segment (A B A) with dense branches: every class of A returns 230 bases later -- duplicates
          that are no neighbours, first and later entry in different 64-entry slices of the appended list.
  ring9 / ring8   a tandem repeat of period 18 / 14 with a fork at every second base or so: 9 / 8 classes that a read visits in turn, round
          after round -- few classes, long lists.
A read is a stretch of a spine (mate 2 reverse-complemented, or placed on the same strand for the cases that need it), trimmed base by
base until the emulation of the stepper (tests/emu_classlist, emu_class_list) reports the wanted count: tests/manyclass.py says how D, A and S
are counted and lists the groups; case.json records the three numbers of every item under every variant and the members of every group.

The directory holds index.idx.gz, reads_1.txt.gz, reads_2.txt.gz, expected_<variant>.txt.gz (oracle/_ref/dump_ec quant) and case.json,
everything gzipped without a time stamp.  A second run gives the same reads and expected files byte for byte; the reference's index file
differs by a few hundred bytes from run to run while holding the same graph.  It is NOT one of tests/common.CASES: tests/manyclass.py
loads it.
"""
from __future__ import annotations

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
from tests import manyclass as M  # noqa: E402
from tests import emu_binding as E  # noqa: E402
sys.path.insert(0, HERE)
from make_bigsets import write_gz, write_lines, write_fastq  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
KALLISTO = os.path.join(REF, "kallisto")
DUMP = os.path.join(REF, "dump_ec")
K = 31
MAX_READ = 400
SE = ["--single", "-l", "200", "-s", "20"]
VARIANTS = {"pe": [], "pe_union": ["--union"], "pe_fr": ["--fr"], "pe_nojump": ["--no-jump"], "se": SE}


def transcriptome(seed=7):
    rng = np.random.default_rng(seed)
    rnd = lambda n: synth._ACGT[rng.integers(0, 4, n)]
    seqs, spines = [], {}

    def spine(name, s):
        spines[name] = s
        seqs.append(s)

    def branch(s, p, shared, tail):
        """shares s[p - shared : p], then diverges: its next base is not the spine's"""
        t = rnd(tail)
        while t[0] == s[p]:
            t[0] = synth._ACGT[rng.integers(0, 4)]
        seqs.append(np.concatenate([s[p - shared:p], t]))

    def dense_branches(s, lo, hi):
        p = lo
        while p < hi:
            branch(s, p, 40, 34)
            p += int(rng.integers(2, 4))

    dense = rnd(840)
    spine("dense", dense)
    dense_branches(dense, 44, 830)
    seqs.append(synth.revcomp(dense[:430]))
    seqs.append(np.concatenate([rnd(80), dense[480:800], rnd(80)]))

    quiet = rnd(640)
    spine("quiet", quiet)
    for p in range(34, 630, 2):
        branch(quiet, p, 30, 36)
    for a, b in ((100, 560), (180, 620), (260, 420), (300, 600)):
        seqs.append(quiet[a:b].copy())

    a_seg, b_seg = rnd(170), rnd(60)
    aba = np.concatenate([rnd(45), a_seg, b_seg, a_seg, rnd(45)])
    spine("aba", aba)
    dense_branches(aba, 45 + 42, 45 + 170 + 60)

    # (the way into the repeat and the way out of it are forks as well: which classes they add depends on the phase they meet)
    for name, period, phases in (("ring9", 18, range(0, 18, 2)), ("ring8", 14, (0, 2, 4, 5, 6, 8, 10, 12))):
        s = np.concatenate([rnd(45), np.tile(rnd(period), 26), rnd(45)])
        spine(name, s)
        for phase in phases:
            branch(s, 45 + 3 * period + phase, 30, 36)
    return seqs, spines, rng


class Fitter:
    """trims a read base by base until the emulation reports the wanted count"""

    def __init__(self, ix):
        self.ix = ix
        self.tables = M.class_tables(ix)

    def figures(self, m1, m2):
        words, l16, max_len = E.pack([bytes(m1), bytes(m2)], MAX_READ)
        return M.item_figures(self.ix, words, l16, 1, 1, max_len, tables=self.tables)[0]

    def fit(self, gen, key, target, lo, hi):
        """the pair gen(L), lo <= L <= hi, with key(figures) == target -- key is monotone in L; None if no L gives it"""
        a, b = lo, hi
        while a < b:
            mid = (a + b) // 2
            if key(self.figures(*gen(mid))) >= target:
                b = mid
            else:
                a = mid + 1
        pair = gen(a)
        return pair if key(self.figures(*pair)) == target else None


def reads(spines, rng, ix):
    fit = Fitter(ix)
    rc = synth.revcomp
    junk = lambda n=60: synth._ACGT[rng.integers(0, 4, n)]
    A, D = (lambda f: f.A), (lambda f: f.D)
    out, notes = [], []

    def add(pair, what):
        if pair is None:
            notes.append(f"not reachable: {what}")
            return
        m1, m2 = pair
        assert len(m1) <= MAX_READ and len(m2) <= MAX_READ
        out.append((bytes(m1), bytes(m2)))

    dense, quiet, aba, ring9, ring8 = (spines[n] for n in ("dense", "quiet", "aba", "ring9", "ring8"))

    def flipped(gen):   # the pair in the other orientation: mate 1 on the reverse strand
        return lambda L: tuple(rc(x) for x in gen(L))

    # generators: L is the length of the mate that is trimmed
    one_mate = lambda s, st: (lambda L: (s[st:st + L], junk()))                                    # mate 2 has no hit
    pair_fr = lambda s, s1, l1, e2: (lambda L: (s[s1:s1 + l1], rc(s[e2 - L:e2])))                  # a proper pair, mate 2 trimmed at its far end
    overlap = lambda s, s1, l1: (lambda L: (s[s1:s1 + l1], rc(s[s1 + l1 - L:s1 + l1])))            # mate 2 starts in mate 1's last class, walks back over it
    same_strand = lambda s, s1, l1: (lambda L: (s[s1:s1 + l1], s[s1 + l1 - 31:s1 + l1 - 31 + L]))  # mate 2 goes on where mate 1 ends

    # 1. the first pass's edge
    for d in (7, 8, 9):
        for j, (s, st) in enumerate(((dense, 50), (dense, 333), (dense, 610), (quiet, 40), (aba, 60), (dense, 200))):
            add(fit.fit(one_mate(s, st), D, d, K, 120), f"D={d} at {st}")
        add(fit.fit(pair_fr(dense, 500, 33, 640), D, d, K, 100), f"D={d} pair")
    for st, n in ((60, 80), (70, 150), (61, 300), (90, 390), (100, 200)):          # ring8: eight classes, round after round
        add((ring8[st:st + n], rc(ring8[st + 20:st + 20 + n])), "ring8")
        add((ring8[st:st + n], junk()), "ring8")
    for st in (36, 60, 95, 97, 175, 255, 297, 415, 555):                              # quiet: one set, or a set boundary inside eight classes
        add(fit.fit(one_mate(quiet, st), D, 8, K, 120), f"quiet D=8 at {st}")
        add(fit.fit(one_mate(quiet, st), D, 3, K, 120), f"quiet D=3 at {st}")
    # 2. / 3. the lane slots of k_classify_long and the re-overflow
    for a in M.LANE_SLOT_A + (193, 194):
        add(fit.fit(one_mate(dense, 40 + a), A, a, K, MAX_READ), f"A={a} one mate, dense")
        add(fit.fit(pair_fr(dense, 30, 35 + a // 4, 800), A, a, K, MAX_READ), f"A={a} pair, dense, antisense region")
        add(fit.fit(pair_fr(dense, 440, 35 + a // 3, 836), A, a, K, MAX_READ), f"A={a} pair, dense")
        add(fit.fit(flipped(pair_fr(dense, 450, 40 + a // 3, 830)), A, a, K, MAX_READ), f"A={a} pair, dense, other orientation")
        add(fit.fit(flipped(one_mate(dense, 435)), A, a, K, MAX_READ), f"A={a} one mate, other orientation")
        add(fit.fit(overlap(dense, 445, 31 + (17 * a) // 20), A, a, K, 31 + (17 * a) // 20), f"A={a} overlap, dense")
        add(fit.fit(overlap(dense, 20, 31 + (17 * a) // 20), A, a, K, 31 + (17 * a) // 20), f"A={a} overlap, dense, antisense region")
        add(fit.fit(same_strand(dense, 460, 36 + a // 3), A, a, K, MAX_READ), f"A={a} same strand, dense")
        add(fit.fit(one_mate(aba, 40), A, a, K, MAX_READ), f"A={a} one mate, aba")
        if a > 100:
            add(fit.fit(pair_fr(aba, 50, 160, 480), A, a, K, MAX_READ), f"A={a} pair, aba")
        add(fit.fit(pair_fr(quiet, 36, 34 + a // 2, 636), A, a, K, MAX_READ), f"A={a} pair, quiet")
        add(fit.fit(pair_fr(ring9, 50, 40 + a, 500), A, a, K, MAX_READ), f"A={a} pair, ring9")
    for a in (160, 170, 180):
        add(fit.fit(pair_fr(quiet, 40 + a % 7, 340, 630), A, a, K, MAX_READ), f"A={a} pair, quiet")
    add(fit.fit(pair_fr(ring9, 60, 380, 490), A, 180, K, MAX_READ), "A=180 pair, ring9")
    for a in (193, 200, 230, 260, 300):
        add(fit.fit(pair_fr(ring9, 55, 390, 495), A, a, K, MAX_READ), f"A={a} pair, ring9")
    add((dense[20:420], rc(dense[430:830])), "two mates of 400")
    add((dense[30:430], rc(dense[436:836])), "two mates of 400")
    add((dense[436:836], rc(dense[20:420])), "two mates of 400")
    add((quiet[30:430], rc(quiet[240:640])), "two mates of 400, quiet")
    add((aba[30:430], rc(aba[90:490])), "two mates of 400, aba")
    # 4. mates
    for st in (60, 300, 500):
        add((dense[st:st + 150], rc(quiet[st:st + 140])), "sets with an empty intersection")
        add((junk(90), rc(dense[st:st + 180])), "mate 1 without a hit")
        add((junk(70), junk(80)), "unmapped")
        add((dense[st:st + 31], rc(dense[st + 100:st + 131])), "two classes")
    return out, notes


def main():
    if not (os.path.exists(KALLISTO) and os.path.exists(DUMP)):
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` in the build container")
    d = os.path.join(HERE, M.NAME)
    os.makedirs(d, exist_ok=True)
    seqs, spines, rng = transcriptome()
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "m.fa")
        synth.write_fasta(fa, seqs)
        idx = os.path.join(tmp, "index.idx")
        subprocess.check_call([KALLISTO, "index", "-k", str(K), "-i", idx, fa], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        ix = E.EmuIndex(idx)
        pairs, notes = reads(spines, rng, ix)
        r1, r2 = [p[0] for p in pairs], [p[1] for p in pairs]
        n = len(pairs)
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
        # the figures of every item under the three ways the matcher runs
        words, l16, max_len = E.pack([x for p in pairs for x in p], MAX_READ)
        w1, l1, _ = E.pack(r1, MAX_READ)
        figs = {"pe": M.item_figures(ix, words, l16, n, 1, max_len), "pe_nojump": M.item_figures(ix, words, l16, n, 1, max_len, no_jump=1),
                "se": M.item_figures(ix, w1, l1, n, 0, max_len)}
        oc = M.filter_outcomes(ix, words, l16, n, max_len, strand=1)
        raw_bytes = os.path.getsize(idx)
        n_sets, n_uec = int(ix.view.n_ecs), int(ix.view.n_uec)
    grp = M.groups(figs["pe"], oc)
    short = {g: len(v) for g, v in grp.items() if len(v) < M.SINGLE.get(g, M.MIN_ITEMS)}
    lane = {}
    for a in M.LANE_SLOT_A:      # S as close to A as the graph allows, per A
        lane[str(a)] = max((figs["pe"][i].S for i in grp[f"A={a}"]), default=0)
    meta = {"name": M.NAME, "k": K, "paired": True, "n": n, "variants": VARIANTS, "targets": len(seqs), "n_sets": n_sets, "n_classes": n_uec,
            "index_bytes": raw_bytes, "max_read": MAX_READ,
            "figures": {v: {"D": [it.D for it in f], "A": [it.A for it in f], "S": [it.S for it in f]} for v, f in figs.items()},
            "filter_outcome_fr": oc.tolist(),
            "groups": grp,
            "largest_S_at_A": lane,
            "groups_short_of_items": short,
            "not_reachable": notes,
            "note": "spines dense / quiet / aba / ring9 / ring8 with side transcripts every 2..3 bases (seed 7, make_manyclass.py); reads placed by hand and "
                    "trimmed until the emulation's count is the wanted one.  largest_S_at_A: the nearest S to A reached per A (a jump's back-off "
                    "can revisit a class, so S stays a few below A for some).  A pair that pair_is_mapped refuses although a mate has hits needs a class whose set is EMPTY: the reference's "
                    "index builder gives every class of this transcriptome a set -- with --d-list as well (tried: the D-list k-mers' class carries an off-listed "
                    "target, such items are dropped when the sets are resolved) -- so the unmapped items here have no hit at all and never reach the long-list route.",
            "reference": "pachterlab/kallisto v0.51.1 via oracle/_ref/dump_ec (unmodified sources)"}
    with open(os.path.join(d, "case.json"), "w") as f:      # one key per line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in meta.items()) + "\n}\n")
    for fn in sorted(os.listdir(d)):
        print(fn, os.path.getsize(os.path.join(d, fn)))
    print("items", n, "transcripts", len(seqs), "classes", n_uec, "sets", n_sets)
    print({g: len(v) for g, v in grp.items()})
    print("short:", short)
    print("largest S at A:", lane)
    print("\n".join(notes))


if __name__ == "__main__":
    main()
