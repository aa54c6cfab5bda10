"""Rate of the per-read class pass (kamd_read_ecs) beside kamd_pseudoalign on the same batches, for one paired and one single-end synthetic
workload.  Not part of bench.py: the flagship line does not touch this path.

    python tools/read_ecs_rate.py [--genes 2000] [--transcripts 6000] [--reads 1000000] [--repeats 5] [--cache DIR] [--out profiles/read_ecs_rate.md]

The transcriptomes are kallisto_amd/synth.py's (human_like for the paired workload, yeast_like for the single-end one); their indexes are built
by the reference binary (oracle/_ref/kallisto index) and kept under --cache when given.  Times are HIP events around the calls over warmed-up
repeats, and the library's own events around the table build and the per-item launches (kamd_debug_read_ecs)."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KALLISTO = os.path.join(ROOT, "oracle", "_ref", "kallisto")


def workload(kind, size, cache):
    from kallisto_amd import synth
    seqs = synth.human_like(n_genes=size, seed=2) if kind == "human" else synth.yeast_like(n_tr=size, seed=1)
    idx = os.path.join(cache, "%s_%d.idx" % (kind, size))
    if not os.path.exists(idx):
        if not os.path.exists(KALLISTO):
            sys.exit("read_ecs_rate.py: the index of a synthetic transcriptome is built by oracle/_ref/kallisto, which is not built here")
        fa = os.path.join(cache, "%s_%d.fa" % (kind, size))
        synth.write_fasta(fa, seqs)
        subprocess.run([KALLISTO, "index", "-t", "16", "-i", idx + ".tmp", fa], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        os.replace(idx + ".tmp", idx)
        os.remove(fa)
    return seqs, idx


def med(x):
    return sorted(x)[len(x) // 2]


def measure(ka, torch, name, seqs, idx, paired, n, repeats):
    from kallisto_amd import synth
    r1, r2 = synth.simulate_reads(seqs, n, read_len=100, paired=paired, seed=5)
    reads = np.stack([r1, r2], axis=1).reshape(2 * n, 100) if paired else r1
    index = ka.Index(idx)
    ctx = ka.Context(0)
    ctx.upload(index)
    words, lens = ctx.pack_reads(torch.from_numpy(np.ascontiguousarray(reads)).cuda(), 100)
    opts = ka.QuantOpts(1, 0.0, 0.0, 0, 0) if paired else ka.QuantOpts(0, 200.0, 20.0, 0, 0)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t_align = []
    for rep in range(2 + repeats):   # two warm-up runs
        ctx.reset()
        e0, e1 = ev(), ev()
        e0.record(ctx.stream)
        ctx.pseudoalign(opts, words, lens, n, 100)
        e1.record(ctx.stream)
        e1.synchronize()
        if rep >= 2:
            t_align.append(e0.elapsed_time(e1))
    ecs = ctx.finalize()
    t_call, t_items, t_table = [], [], []
    for rep in range(2 + repeats):
        if rep >= 2:
            ctx.ec_upload(ecs.ec_off, ecs.ec_ids, ecs.counts)   # the same result installed again: the next call builds its table
        e0, e1 = ev(), ev()
        e0.record(ctx.stream)
        d, st = ctx.read_ecs(opts, words, lens, n, 100)
        e1.record(ctx.stream)
        e1.synchronize()
        dbg = ctx.debug_read_ecs(0, 0)
        if rep >= 2:
            t_call.append(e0.elapsed_time(e1)); t_items.append(dbg["items_ms"]); t_table.append(dbg["table_ms"])
    d = d.cpu().numpy()
    ok = np.array_equal(np.bincount(d[d >= 0], minlength=len(ecs.counts)), ecs.counts.astype(np.int64)) and st["n_foreign"] == 0
    sizes = np.diff(ecs.ec_off.astype(np.int64))
    what = "pairs" if paired else "reads"
    lines = ["## %s: %d transcripts, %d %s of 100 nt" % (name, len(seqs), n, what), "",
             "| what | ms (median of %d, min .. max) | %s/s |" % (repeats, what), "|---|---|---|",
             "| `kamd_pseudoalign`, one call (HIP events) | %.2f (%.2f .. %.2f) | %.3g |" % (med(t_align), min(t_align), max(t_align), n / med(t_align) * 1e3),
             "| `kamd_read_ecs`, one call on the same batch, table build included (HIP events) | %.2f (%.2f .. %.2f) | %.3g |"
             % (med(t_call), min(t_call), max(t_call), n / med(t_call) * 1e3),
             "| of which the per-item launches `k_read_ecs` (both tiers, all chunks) | %.2f (%.2f .. %.2f) | %.3g |"
             % (med(t_items), min(t_items), max(t_items), n / med(t_items) * 1e3),
             "| of which the table build `k_rec_table_build` (memset + one launch over %d classes) | %.3f (%.3f .. %.3f) | |"
             % (len(ecs.counts), med(t_table), min(t_table), max(t_table)), "",
             "`kamd_read_ecs` takes %.2f x the time of `kamd_pseudoalign` here; %s dominates the pass (%.1f %% of the call)."
             % (med(t_call) / med(t_align), "`k_read_ecs`" if med(t_items) >= med(t_table) else "`k_rec_table_build`",
                100.0 * max(med(t_items), med(t_table)) / med(t_call)),
             "Outcome: %d of %d %s in %d classes (largest %d members, %d with more than 64), %d without a class, %d items went to the second tier; "
             "the histogram of the ids %s the finalized counts." % (st["n_mapped"], n, what, len(ecs.counts), int(sizes.max(initial=0)), int((sizes > 64).sum()),
                                                                   st["n_none"], dbg["n_second_tier"], "equals" if ok else "DIFFERS FROM"), ""]
    ctx.close()
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=2000, help="paired workload: genes of synth.human_like")
    ap.add_argument("--transcripts", type=int, default=6000, help="single-end workload: transcripts of synth.yeast_like")
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=None, help="directory that keeps the indexes between runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_ecs_rate.md"))
    args = ap.parse_args()
    import torch
    import kallisto_amd as ka
    if not torch.cuda.is_available():
        sys.exit("read_ecs_rate.py measures on the GPU: no HIP device visible")
    lines = ["# Per-read equivalence classes (`kamd_read_ecs`): measured rate", "",
             "One thread per item; chunks of 65536 items, a first tier of 64 list entries per item, a second tier of 1024.  Device: %s." % torch.cuda.get_device_name(0), ""]
    all_ok = True
    with tempfile.TemporaryDirectory() as tmp:
        cache = args.cache or tmp
        os.makedirs(cache, exist_ok=True)
        for name, kind, size, paired in (("Paired", "human", args.genes, True), ("Single-end", "yeast", args.transcripts, False)):
            seqs, idx = workload(kind, size, cache)
            part, ok = measure(ka, torch, name, seqs, idx, paired, args.reads, args.repeats)
            lines += part
            all_ok = all_ok and ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
