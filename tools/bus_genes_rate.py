"""What the gene-level count costs on the device (kamd_bus_genes_create, kamd_bus_count_genes) beside the class-level count (kamd_bus_count) and beside
the host path a driver would otherwise need (download of the records, the groups' gene sets intersected in a Python loop over dicts), on the
records of tools/bus_sc_rate.py's synthetic 10xv3 run.  Not part of bench.py: the flagship line does not touch this path.

    python tools/bus_genes_rate.py [--transcripts 6000] [--reads 2000000] [--repeats 5] [--cache DIR] [--out profiles/bus_genes_rate.md]

The steps run as child processes, each under its own `timeout`, and the script stops at the first one that fails:

    prepare   tools/bus_sc_rate.py's: index and FASTQ files (CPU)
    measure   the GPU: one pass of bus_split / pseudoalign / finalize / read_ecs / bus_records / bus_sort gives the sorted, collapsed records and
              their classes.  Gene map: gene(t) = t // 3.  Per repeat: kamd_bus_genes_create on the batch's classes (upload, list build; the
              library's HIP events), kamd_bus_count_genes (likewise, and the part of the two resolve kernels), kamd_bus_count on the same records,
              and the host path: tensor.cpu(), then per (barcode, UMI) group the intersection of its classes' gene sets and a dict of
              (barcode, gene) counts (wall clock)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bus_sc_rate as R  # noqa: E402


def host_path(d_rec, A, gene_sets):
    """-> ({(barcode, gene): count}, seconds per step); gene_sets[class] = frozenset of gene ids"""
    t0 = time.perf_counter()
    rec = A.bus_records_numpy(d_rec).copy()
    t1 = time.perf_counter()
    groups = {}
    for b, u, e in zip(rec["barcode"].tolist(), rec["umi"].tolist(), rec["ec"].tolist()):
        g = groups.get((b, u))
        groups[(b, u)] = gene_sets[e] if g is None else g & gene_sets[e]
    matrix = {}
    for (b, _), g in groups.items():
        if len(g) == 1:
            k = (b, next(iter(g)))
            matrix[k] = matrix.get(k, 0) + 1
    t2 = time.perf_counter()
    return matrix, (t1 - t0, t2 - t1)


def measure(args, work):
    import torch
    import kallisto_amd as ka
    from kallisto_amd import api as A
    if not torch.cuda.is_available():
        print("bus_genes_rate.py: no HIP device visible", file=sys.stderr)
        return 3
    w = json.load(open(os.path.join(work, "workload.json")))
    n = w["n"]
    index = ka.Index(w["index"])
    ctx = ka.Context(0)
    ctx.upload(index)
    texts = [open(os.path.join(work, f), "rb").read() for f in ("tags.fq", "cdna.fq")]
    words, lens, n_items, max_len, status, _ = ctx.fastq_unit_pack(texts, n)
    assert status == 0 and n_items == n
    words, lens = words.clone(), lens.clone()
    del texts
    layout, strand = ka.BusLayout.parse(R.TECH)
    opts = ka.QuantOpts(0, 200.0, 20.0, 1, strand, 0, 0)
    ctx.reset()
    sp = ctx.bus_split(layout, words, lens, n, max_len)
    cut = (sp["seq_words"], sp["seq_len"], sp["n_valid"], sp["seq_max_len"])
    ctx.pseudoalign(opts, *cut)
    ecs = ctx.finalize()
    d_ec, _ = ctx.read_ecs(opts, *cut)
    d_rec = ctx.bus_records(sp["tags"], d_ec, sp["n_valid"])
    n_records = int(d_rec.shape[0])
    srt, _ = ctx.bus_sort(d_rec, None, True)
    srt = srt.clone()
    n_targets = int(index.num_targets)
    tr_gene = (np.arange(n_targets) // 3).astype(np.int32)
    n_genes = (n_targets + 2) // 3
    ec_off, ec_ids = np.ascontiguousarray(ecs.ec_off, np.uint64), np.ascontiguousarray(ecs.ec_ids, np.uint32)
    gene_sets = [frozenset((ec_ids[int(ec_off[c]):int(ec_off[c + 1])] // 3).tolist()) for c in range(len(ec_off) - 1)]
    t = {"create": [], "count_genes": [], "resolve": [], "count": [], "host_download": [], "host_groups": []}
    for rep in range(2 + args.repeats):   # two warm-up runs
        table = ctx.bus_genes(tr_gene, n_genes, (ec_off, ec_ids))
        g = ctx.bus_count_genes(table, srt, A.BUS_COUNT_UMIS)
        c = ctx.bus_count(srt, A.BUS_COUNT_UMIS)
        matrix, hs = host_path(srt, A, gene_sets)
        if rep >= 2:
            t["create"].append(table.stats["ms"]); t["count_genes"].append(g["stats"]["ms"]); t["resolve"].append(g["stats"]["resolve_ms"]); t["count"].append(c["stats"]["ms"])
            for k, s in zip(("host_download", "host_groups"), hs):
                t[k].append(1e3 * s)
        tstats = dict(table.stats)
        table.free()
    en = A.bus_entries_numpy(g["entries"])
    barcodes = g["barcodes"].cpu().numpy().view(np.uint64).tolist()
    got = {(barcodes[r], e): v for r, e, v in zip(en["row"].tolist(), en["ec"].tolist(), en["value"].tolist())}
    ok = got == matrix
    out = {"device": torch.cuda.get_device_name(0), "n": n, "transcripts": w["transcripts"], "n_records": n_records, "n_sorted": int(srt.shape[0]),
           "table": {k: v for k, v in tstats.items() if k != "ms"}, "genes": {k: v for k, v in g["stats"].items() if not k.endswith("ms")},
           "count": {k: v for k, v in c["stats"].items() if k != "ms"}, "identical": bool(ok), "repeats": args.repeats,
           "ms": {k: [R.med(v), min(v), max(v)] for k, v in t.items()}}
    json.dump(out, open(os.path.join(work, "measure.json"), "w"))
    ctx.close()
    return 0 if ok else 1


def report(args, work):
    m = json.load(open(os.path.join(work, "measure.json")))
    ms, tb, g, c = m["ms"], m["table"], m["genes"], m["count"]
    row = lambda what, k, per: "| %s | %.2f (%.2f .. %.2f) | %.3g |" % (what, ms[k][0], ms[k][1], ms[k][2], per / ms[k][0] * 1e3)
    host = sum(ms[k][0] for k in ("host_download", "host_groups"))
    lines = ["# Gene-level counts on the device (`kamd_bus_genes_create`, `kamd_bus_count_genes`): measured times", "",
             "Synthetic %s run of tools/bus_sc_rate.py: %d read sets, %d transcripts, one batch: %d records, %d after sort and collapse.  Gene map: gene(t) = t // 3 "
             "(%d genes).  Device: %s." % (R.TECH, m["n"], m["transcripts"], m["n_records"], m["n_sorted"], tb["n_genes"], m["device"]),
             "The table: %d classes with %d entries -> %d distinct (class, gene) pairs, %d classes without a gene, longest list %d."
             % (tb["n_classes"], tb["n_entries_in"], tb["n_pairs"], tb["n_empty"], tb["max_list"]),
             "The count: %d barcodes, %d groups: %d counted, %d without a gene, %d with several; %d entries.  **%d groups took the wave path** "
             "(`k_gen_wave`), the others were settled by a thread.  `kamd_bus_count` on the same records: %d entries, %d multi-class groups."
             % (g["n_barcodes"], g["n_umis"], g["n_counted"], g["n_no_gene"], g["n_multi_gene"], g["n_entries"], g["n_wave_groups"], c["n_entries"], c["n_multi_groups"]), "",
             "| what | ms (median of %d, min .. max) | items/s |" % m["repeats"], "|---|---|---|",
             row("`kamd_bus_genes_create`: upload of map and classes (pageable), keys, sort with collapse, offsets (the library's HIP events; per entry)", "create", tb["n_entries_in"]),
             row("`kamd_bus_count_genes`: all launches, its second sort and the three synchronisations (the library's HIP events; per record)", "count_genes", m["n_sorted"]),
             row("... of which the resolve step, `k_gen_thread` + `k_gen_wave` (per group)", "resolve", g["n_umis"]),
             row("`kamd_bus_count` on the same records (per record)", "count", m["n_sorted"]),
             row("host path: download of the records (`tensor.cpu()`, pageable)", "host_download", m["n_sorted"]),
             row("host path: gene sets intersected per group in a Python loop, a dict of (barcode, gene) counts (per record)", "host_groups", m["n_sorted"]), "",
             "The resolve step is %.0f %% of `kamd_bus_count_genes`, which takes %.2f x the time of `kamd_bus_count` (%.2f ms against %.2f ms)."
             % (100.0 * ms["resolve"][0] / ms["count_genes"][0], ms["count_genes"][0] / ms["count"][0], ms["count_genes"][0], ms["count"][0]),
             "The host path sums to %.1f ms: %.0f x the device call.  The device's matrix is %s the host path's.  No time was promised in advance."
             % (host, host / ms["count_genes"][0], "identical to" if m["identical"] else "DIFFERENT FROM"), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0


STEPS = {"prepare": (R.prepare, 600), "measure": (measure, 400), "report": (report, 60)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transcripts", type=int, default=6000)
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=None, help="directory that keeps the index between runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bus_genes_rate.md"))
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--work", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return STEPS[args.step][0](args, args.work)
    with tempfile.TemporaryDirectory() as work:
        for step in ("prepare", "measure", "report"):
            cmd = ["timeout", "-k", "10", str(STEPS[step][1]), sys.executable, os.path.abspath(__file__), "--step", step, "--work", work,
                   "--transcripts", str(args.transcripts), "--reads", str(args.reads), "--repeats", str(args.repeats), "--out", args.out]
            cmd += ["--cache", args.cache] if args.cache else []
            rc = subprocess.run(cmd).returncode
            if rc != 0:   # the first failure ends the run: nothing more is started
                print("bus_genes_rate.py: step %s failed (%d)" % (step, rc), file=sys.stderr)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
