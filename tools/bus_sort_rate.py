"""What the sort / collapse / count of BUS records costs on the device (kamd_bus_sort, kamd_bus_count) beside the host path the single-cell driver
used before (download of the records, np.lexsort over four fields, run-length collapse), on the records of tools/bus_sc_rate.py's synthetic 10xv3
run.  Not part of bench.py: the flagship line does not touch this path.

    python tools/bus_sort_rate.py [--transcripts 6000] [--reads 2000000] [--repeats 5] [--cache DIR] [--out profiles/bus_sort_rate.md]

The steps run as child processes, each under its own `timeout`, and the script stops at the first one that fails:

    prepare   tools/bus_sc_rate.py's: index and FASTQ files (CPU)
    measure   the GPU: one pass of bus_split / pseudoalign / finalize / read_ecs / bus_records gives the records (one per pseudoaligned read set, in
              input order, batch-local classes); then per repeat, each on a fresh copy of them, kamd_bus_sort with collapse and without (the library's
              HIP events: everything between the call's first launch and its last read-back) and kamd_bus_count on the collapsed result (likewise);
              and the host path on the same records: tensor.cpu(), np.lexsort((flags, ec, umi, barcode)), the collapse (wall clock)
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


def host_path(d_rec, A):
    """the driver's former path: every record downloaded, np.lexsort over four fields, equal keys collapsed -> (records, seconds per step)"""
    t0 = time.perf_counter()
    rec = A.bus_records_numpy(d_rec).copy()
    t1 = time.perf_counter()
    rec = rec[np.lexsort((rec["flags"], rec["ec"], rec["umi"], rec["barcode"]))]
    t2 = time.perf_counter()
    first = np.ones(len(rec), bool)
    first[1:] = (rec["barcode"][1:] != rec["barcode"][:-1]) | (rec["umi"][1:] != rec["umi"][:-1]) | (rec["ec"][1:] != rec["ec"][:-1]) | (rec["flags"][1:] != rec["flags"][:-1])
    starts = np.flatnonzero(first)
    out = rec[starts].copy()
    out["count"] = np.diff(np.append(starts, len(rec)))
    t3 = time.perf_counter()
    return out, (t1 - t0, t2 - t1, t3 - t2)


def measure(args, work):
    import torch
    import kallisto_amd as ka
    from kallisto_amd import api as A
    if not torch.cuda.is_available():
        print("bus_sort_rate.py: no HIP device visible", file=sys.stderr)
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
    layout, strand = ka.BusLayout.parse(R.TECH)
    opts = ka.QuantOpts(0, 200.0, 20.0, 1, strand, 0, 0)
    ctx.reset()
    sp = ctx.bus_split(layout, words, lens, n, max_len)
    cut = (sp["seq_words"], sp["seq_len"], sp["n_valid"], sp["seq_max_len"])
    ctx.pseudoalign(opts, *cut)
    ctx.finalize()
    d_ec, _ = ctx.read_ecs(opts, *cut)
    base = ctx.bus_records(sp["tags"], d_ec, sp["n_valid"]).clone()
    t = {"sort_collapse": [], "sort": [], "count": [], "host_download": [], "host_lexsort": [], "host_collapse": []}
    passes = cst = None
    for rep in range(2 + args.repeats):   # two warm-up runs
        col, st1 = ctx.bus_sort(base.clone(), None, True)
        srt, st2 = ctx.bus_sort(base.clone(), None, False)
        c = ctx.bus_count(col, A.BUS_COUNT_UMIS)
        want, hs = host_path(base, A)
        if rep >= 2:
            t["sort_collapse"].append(st1["ms"]); t["sort"].append(st2["ms"]); t["count"].append(c["stats"]["ms"])
            for k, s in zip(("host_download", "host_lexsort", "host_collapse"), hs):
                t[k].append(1e3 * s)
        passes, cst = st1["passes"], c["stats"]
    ok = A.bus_records_numpy(col).tobytes() == want.tobytes() and len(srt) == len(base)
    out = {"device": torch.cuda.get_device_name(0), "n": n, "transcripts": w["transcripts"], "n_records": int(len(base)), "n_collapsed": int(len(col)), "passes": int(passes),
           "key_bits": int(st1["key_bits"]), "count": {k: v for k, v in cst.items() if k != "ms"}, "identical": bool(ok), "repeats": args.repeats,
           "ms": {k: [R.med(v), min(v), max(v)] for k, v in t.items()}}
    json.dump(out, open(os.path.join(work, "measure.json"), "w"))
    ctx.close()
    return 0 if ok else 1


def report(args, work):
    m = json.load(open(os.path.join(work, "measure.json")))
    nr, ms = m["n_records"], m["ms"]
    row = lambda what, k: "| %s | %.2f (%.2f .. %.2f) | %.3g |" % (what, ms[k][0], ms[k][1], ms[k][2], nr / ms[k][0] * 1e3)
    host = sum(ms[k][0] for k in ("host_download", "host_lexsort", "host_collapse"))
    gb = 96.0 * nr * m["passes"] / 1e9   # per pass and record: 32 read and 32 written by the scatter, and the histogram's 16-byte loads touch every 32-byte record once more
    lines = ["# BUS records -> cells x classes (`kamd_bus_sort`, `kamd_bus_count`): measured times", "",
             "Synthetic %s run of tools/bus_sc_rate.py: %d read sets, %d transcripts, one batch: %d records (one per pseudoaligned read set, input order), %d after the collapse."
             "  The keys differ in %d bits: %d LSD passes.  Device: %s." % (R.TECH, m["n"], m["transcripts"], nr, m["n_collapsed"], m["key_bits"], m["passes"], m["device"]), "",
             "| what | ms (median of %d, min .. max) | records/s |" % m["repeats"], "|---|---|---|",
             row("`kamd_bus_sort`, collapse on: pre-pass, %d passes, collapse, both synchronisations (the library's HIP events)" % m["passes"], "sort_collapse"),
             row("`kamd_bus_sort`, collapse off", "sort"),
             row("`kamd_bus_count` (UMIS) on the collapsed records, its second sort included (the library's HIP events)", "count"),
             row("host path: download of the records (`tensor.cpu()`, pageable)", "host_download"),
             row("host path: `np.lexsort((flags, ec, umi, barcode))` and the gather", "host_lexsort"),
             row("host path: collapse of equal keys", "host_collapse"), "",
             "The host path sums to %.1f ms; the device sort with collapse takes %.2f ms: %.1f x.  The device result is %s the host path's, byte for byte."
             % (host, ms["sort_collapse"][0], host / ms["sort_collapse"][0], "identical to" if m["identical"] else "DIFFERENT FROM"),
             "At about 96 bytes of traffic per record and pass the %d passes move %.2f GB: %.0f GB/s over the whole call without collapse."
             % (m["passes"], gb, gb / (ms["sort"][0] * 1e-3)),
             "The count: %d barcodes, %d (barcode, UMI) groups, %d of them multi-class (%d records handed to the host), %d matrix entries."
             % (m["count"]["n_barcodes"], m["count"]["n_umis"], m["count"]["n_multi_groups"], m["count"]["n_multi_records"], m["count"]["n_entries"]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0


STEPS = {"prepare": (R.prepare, 600), "measure": (measure, 300), "report": (report, 60)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transcripts", type=int, default=6000)
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=None, help="directory that keeps the index between runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bus_sort_rate.md"))
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
                print("bus_sort_rate.py: step %s failed (%d)" % (step, rc), file=sys.stderr)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
