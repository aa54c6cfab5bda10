"""What the barcode / UMI path costs (kamd_bus_split, kamd_bus_records) beside kamd_pseudoalign and kamd_read_ecs on the same cut batch, for a
synthetic 10xv3 run.  Not part of bench.py: the flagship line does not touch this path.

    python tools/bus_sc_rate.py [--transcripts 6000] [--reads 2000000] [--repeats 5] [--cache DIR] [--out profiles/bus_sc_rate.md]

The transcriptome is kallisto_amd/synth.py's yeast_like; its index is built by the reference binary (oracle/_ref/kallisto index) and kept under
--cache when given.  The reads are single-end 100 nt from it, the tag reads 28 random bases from a pool of 4096 barcodes, both written as FASTQ
so that the reference can read the same files.  The steps run as child processes, each under its own `timeout`, and the script stops at the first
one that fails:

    prepare   index and FASTQ files (CPU)
    measure   the GPU: the files through kamd_fastq_unit_pack, then per repeat bus_split / pseudoalign / finalize / read_ecs / bus_records.
              kamd_bus_split and kamd_read_ecs report their kernels by the library's HIP events; kamd_pseudoalign and kamd_bus_records are timed by
              HIP events around the call (kamd_bus_records: its three launches and the read-back of its counters)
    reference where oracle/_ref/kallisto is present: wall time of `kallisto bus -x 10xv3 -t 16` on the same files (CPU)
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KALLISTO = os.path.join(ROOT, "oracle", "_ref", "kallisto")
TECH = "10XV3"


def med(x):
    return sorted(x)[len(x) // 2]


def fastq_bytes(reads):
    """(n, L) uint8 -> strict 4-line FASTQ text with constant headers and qualities"""
    n, L = reads.shape
    rec = np.empty((n, 3 + L + 3 + L + 1), np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@r\n", np.uint8)
    rec[:, 3:3 + L] = reads
    rec[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 6 + L:6 + 2 * L] = ord("I")
    rec[:, 6 + 2 * L] = ord("\n")
    return rec.tobytes()


def prepare(args, work):
    from kallisto_amd import synth
    seqs = synth.yeast_like(n_tr=args.transcripts, seed=1)
    cache = args.cache or work
    os.makedirs(cache, exist_ok=True)
    idx = os.path.join(cache, "yeast_%d.idx" % args.transcripts)
    if not os.path.exists(idx):
        if not os.path.exists(KALLISTO):
            sys.exit("bus_sc_rate.py: the index of the synthetic transcriptome is built by oracle/_ref/kallisto, which is not built here")
        fa = os.path.join(work, "tr.fa")
        synth.write_fasta(fa, seqs)
        subprocess.run([KALLISTO, "index", "-t", "16", "-i", idx + ".tmp", fa], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        os.replace(idx + ".tmp", idx)
    r1, _ = synth.simulate_reads(seqs, args.reads, read_len=100, paired=False, seed=5)
    rng = np.random.default_rng(9)
    pool = rng.integers(0, 4, (4096, 16))
    tags = np.concatenate([pool[rng.integers(0, 4096, args.reads)], rng.integers(0, 4, (args.reads, 12))], axis=1)
    tags = np.frombuffer(b"ACGT", np.uint8)[tags]
    tags[rng.random(args.reads) < 0.01, 5] = ord("N")
    with open(os.path.join(work, "tags.fq"), "wb") as f:
        f.write(fastq_bytes(tags))
    with open(os.path.join(work, "cdna.fq"), "wb") as f:
        f.write(fastq_bytes(np.ascontiguousarray(r1)))
    json.dump({"index": idx, "n": args.reads, "transcripts": len(seqs)}, open(os.path.join(work, "workload.json"), "w"))
    return 0


def measure(args, work):
    import torch
    import kallisto_amd as ka
    from kallisto_amd import api as A
    if not torch.cuda.is_available():
        print("bus_sc_rate.py: no HIP device visible", file=sys.stderr)
        return 3
    w = json.load(open(os.path.join(work, "workload.json")))
    n = w["n"]
    ctx = ka.Context(0)
    ctx.upload(ka.Index(w["index"]))
    texts = [open(os.path.join(work, f), "rb").read() for f in ("tags.fq", "cdna.fq")]
    words, lens, n_items, max_len, status, _ = ctx.fastq_unit_pack(texts, n)
    assert status == 0 and n_items == n
    words, lens = words.clone(), lens.clone()
    del texts
    layout, strand = ka.BusLayout.parse(TECH)
    opts = ka.QuantOpts(0, 200.0, 20.0, 1, strand, 0, 0)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t = {"split": [], "align": [], "read_ecs": [], "records": []}
    for rep in range(2 + args.repeats):   # two warm-up runs
        ctx.reset()
        sp = ctx.bus_split(layout, words, lens, n, max_len)
        cut = (sp["seq_words"], sp["seq_len"], sp["n_valid"], sp["seq_max_len"])
        e0, e1 = ev(), ev()
        e0.record(ctx.stream)
        ctx.pseudoalign(opts, *cut)
        e1.record(ctx.stream)
        e1.synchronize()
        ecs = ctx.finalize()
        d_ec, st = ctx.read_ecs(opts, *cut)
        e2, e3 = ev(), ev()
        e2.record(ctx.stream)
        rec = ctx.bus_records(sp["tags"], d_ec, sp["n_valid"])
        e3.record(ctx.stream)
        e3.synchronize()
        if rep >= 2:
            t["split"].append(sp["stats"]["ms"]); t["align"].append(e0.elapsed_time(e1)); t["read_ecs"].append(st["ms"]); t["records"].append(e2.elapsed_time(e3))
    r = A.bus_records_numpy(rec)
    ok = len(r) == st["n_mapped"] == int(ecs.counts.sum()) and np.array_equal(np.bincount(r["ec"], minlength=len(ecs.counts)), ecs.counts.astype(np.int64))
    out = {"device": torch.cuda.get_device_name(0), "n": n, "transcripts": w["transcripts"], "n_valid": sp["n_valid"], "n_records": int(len(r)),
           "n_classes": int(len(ecs.counts)), "consistent": bool(ok), "repeats": args.repeats,
           "ms": {k: [med(v), min(v), max(v)] for k, v in t.items()}}
    json.dump(out, open(os.path.join(work, "measure.json"), "w"))
    ctx.close()
    return 0 if ok else 1


def reference(args, work):
    w = json.load(open(os.path.join(work, "workload.json")))
    t0 = time.perf_counter()
    p = subprocess.run([KALLISTO, "bus", "-x", TECH, "-t", "16", "-i", w["index"], "-o", os.path.join(work, "ref_out"), os.path.join(work, "tags.fq"),
                        os.path.join(work, "cdna.fq")], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        print(p.stderr.decode(errors="replace")[-500:], file=sys.stderr)
        return 1
    info = json.load(open(os.path.join(work, "ref_out", "run_info.json")))
    json.dump({"wall_s": wall, "n_pseudoaligned": info["n_pseudoaligned"]}, open(os.path.join(work, "reference.json"), "w"))
    return 0


def report(args, work):
    m = json.load(open(os.path.join(work, "measure.json")))
    n, ms = m["n"], m["ms"]
    row = lambda what, k: "| %s | %.2f (%.2f .. %.2f) | %.3g |" % (what, ms[k][0], ms[k][1], ms[k][2], n / ms[k][0] * 1e3)
    total = sum(ms[k][0] for k in ms)
    lines = ["# Barcode / UMI technologies (`kamd_bus_split`, `kamd_bus_records`): measured times", "",
             "Synthetic %s run: %d read sets (28-base tag reads from a pool of 4096 barcodes, 100 nt cDNA reads), %d transcripts, one batch.  Device: %s."
             % (TECH, n, m["transcripts"], m["device"]), "",
             "| what | ms (median of %d, min .. max) | read sets/s |" % m["repeats"], "|---|---|---|",
             row("`kamd_bus_split`: count, scan, scatter of tags, repack of the cut sequences (the library's HIP events)", "split"),
             row("`kamd_pseudoalign` on the cut batch (HIP events around the call)", "align"),
             row("`kamd_read_ecs` on the cut batch, table build included (the library's HIP events)", "read_ecs"),
             row("`kamd_bus_records`: count, scan, scatter and the read-back of its counters (HIP events around the call)", "records"), "",
             "Of the four, `kamd_read_ecs` is %.0f %% of the time, `kamd_pseudoalign` %.0f %%, `kamd_bus_split` %.0f %%, `kamd_bus_records` %.0f %%; "
             "`kamd_read_ecs` takes %.2f x `kamd_pseudoalign`." % (100 * ms["read_ecs"][0] / total, 100 * ms["align"][0] / total, 100 * ms["split"][0] / total,
                                                               100 * ms["records"][0] / total, ms["read_ecs"][0] / ms["align"][0]),
             "Outcome: %d of %d read sets survive the drop rules, %d records in %d classes; the histogram of the records' classes %s the finalized counts."
             % (m["n_valid"], n, m["n_records"], m["n_classes"], "equals" if m["consistent"] else "DIFFERS FROM"), ""]
    ref = os.path.join(work, "reference.json")
    if os.path.exists(ref):
        r = json.load(open(ref))
        lines += ["The reference, `kallisto bus -x %s -t 16` on the same two FASTQ files (wall time of the whole program: reading, pseudoalignment, writing "
                  "output.bus): %.2f s, %d reads pseudoaligned (the GPU path: %d).  The four device calls above sum to %.1f ms; reading and packing the FASTQ text, "
                  "kamd_ec_finalize and the download of the records are not in that sum." % (TECH, r["wall_s"], r["n_pseudoaligned"], m["n_records"], total), ""]
    else:
        lines += ["oracle/_ref/kallisto was not present: the reference's wall time was not measured.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0


STEPS = {"prepare": (prepare, 600), "measure": (measure, 300), "reference": (reference, 600), "report": (report, 60)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transcripts", type=int, default=6000)
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=None, help="directory that keeps the index between runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bus_sc_rate.md"))
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--work", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return STEPS[args.step][0](args, args.work)
    with tempfile.TemporaryDirectory() as work:
        for step in ("prepare", "measure", "reference", "report"):
            if step == "reference" and not os.path.exists(KALLISTO):
                continue
            cmd = ["timeout", "-k", "10", str(STEPS[step][1]), sys.executable, os.path.abspath(__file__), "--step", step, "--work", work,
                   "--transcripts", str(args.transcripts), "--reads", str(args.reads), "--repeats", str(args.repeats), "--out", args.out]
            cmd += ["--cache", args.cache] if args.cache else []
            rc = subprocess.run(cmd).returncode
            if rc != 0:   # the first failure ends the run: nothing more is started
                print("bus_sc_rate.py: step %s failed (%d)" % (step, rc), file=sys.stderr)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
