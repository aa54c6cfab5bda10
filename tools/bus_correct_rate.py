"""What the barcode whitelist costs on the device (kamd_bus_whitelist_create, kamd_bus_correct) beside the sort it feeds (kamd_bus_sort) and beside the
host path a driver would otherwise need (download of the records, membership in the list, the neighbour loop in numpy), on the records of
tools/bus_sc_rate.py's synthetic 10xv3 run.  Not part of bench.py: the flagship line does not touch this path.

    python tools/bus_correct_rate.py [--transcripts 6000] [--reads 2000000] [--repeats 5] [--whitelist 6794880] [--cache DIR] [--out profiles/bus_correct_rate.md]

The steps run as child processes, each under its own `timeout`, and the script stops at the first one that fails:

    prepare   tools/bus_sc_rate.py's: index and FASTQ files (CPU)
    measure   the GPU: one pass of bus_split / pseudoalign / finalize / read_ecs / bus_records gives the records.  Their distinct barcodes are mapped
              onto members of a synthetic whitelist of --whitelist random distinct 16-mers (the size of the 10x v3 list); then 3 % of the records get
              one substituted base and 1 % two.  Per repeat: kamd_bus_whitelist_create (upload, table build; the library's HIP events), kamd_bus_correct
              on the records (likewise, and the part of k_cor_neigh), kamd_bus_sort with collapse on the corrected records, and the host path on the
              same records: tensor.cpu(), np.isin against the list, and for the misses the 48 neighbours looked up one position and base at a time
              (np.searchsorted in the list sorted once outside the clock: np.isin sorts the list again on every call) (wall clock)
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

BC_LEN = 16


def member(w_sorted, x):
    i = np.searchsorted(w_sorted, x)
    i[i == len(w_sorted)] = 0
    return w_sorted[i] == x


def host_path(d_rec, A, W, w_sorted):
    """-> (status uint8 [n], the barcodes the records keep, seconds per step)"""
    t0 = time.perf_counter()
    rec = A.bus_records_numpy(d_rec).copy()
    t1 = time.perf_counter()
    bc = rec["barcode"]
    exact = np.isin(bc, W)
    t2 = time.perf_counter()
    miss = np.flatnonzero(~exact)
    b = bc[miss]
    hits, fixed = np.zeros(len(miss), np.int32), b.copy()
    for p in range(BC_LEN):
        for x in (1, 2, 3):
            nb = b ^ np.uint64(x << (2 * p))
            h = member(w_sorted, nb)
            hits += h
            fixed[h] = nb[h]
    status = np.zeros(len(rec), np.uint8)
    status[miss] = np.where(hits == 1, 1, np.where(hits >= 2, 2, 3))
    keep = bc.copy()
    keep[miss] = fixed
    t3 = time.perf_counter()
    return status, keep, (t1 - t0, t2 - t1, t3 - t2)


def measure(args, work):
    import torch
    import kallisto_amd as ka
    from kallisto_amd import api as A
    if not torch.cuda.is_available():
        print("bus_correct_rate.py: no HIP device visible", file=sys.stderr)
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
    rec = A.bus_records_numpy(ctx.bus_records(sp["tags"], d_ec, sp["n_valid"])).copy()
    # the synthetic whitelist and the records' barcodes on it, with sequencing errors
    rng = np.random.default_rng(17)
    W = np.unique(rng.integers(0, 4 ** BC_LEN, args.whitelist + args.whitelist // 64 + 1024, dtype=np.uint64))
    W = W[rng.permutation(len(W))[:args.whitelist]]
    assert len(W) == args.whitelist
    uniq, inv = np.unique(rec["barcode"], return_inverse=True)
    bc = W[inv]
    kind = rng.random(len(rec))
    p1 = rng.integers(0, BC_LEN, len(rec))
    p2 = (p1 + rng.integers(1, BC_LEN, len(rec))) % BC_LEN
    one, two = kind < 0.04, kind < 0.01
    bc[one] ^= rng.integers(1, 4, int(one.sum())).astype(np.uint64) << (2 * p1[one]).astype(np.uint64)
    bc[two] ^= rng.integers(1, 4, int(two.sum())).astype(np.uint64) << (2 * p2[two]).astype(np.uint64)
    rec["barcode"] = bc
    base = torch.from_numpy(rec.view(np.int64).reshape(-1, 4).copy()).to("cuda:0")
    w_sorted = np.sort(W)
    t = {"create": [], "correct": [], "neigh": [], "sort": [], "host_download": [], "host_isin": [], "host_neigh": []}
    for rep in range(2 + args.repeats):   # two warm-up runs
        wl = ctx.bus_whitelist(W, BC_LEN)
        cor, cst, d_status = ctx.bus_correct(wl, base, True)
        _, sst = ctx.bus_sort(cor.clone(), None, True)
        h_status, h_keep, hs = host_path(base, A, W, w_sorted)
        if rep >= 2:
            t["create"].append(wl.stats["ms"]); t["correct"].append(cst["ms"]); t["neigh"].append(cst["neigh_ms"]); t["sort"].append(sst["ms"])
            for k, s in zip(("host_download", "host_isin", "host_neigh"), hs):
                t[k].append(1e3 * s)
        wstats = dict(wl.stats)
        wl.free()
    ok = np.array_equal(d_status.cpu().numpy(), h_status) and np.array_equal(A.bus_records_numpy(cor)["barcode"], h_keep[h_status <= 1])
    out = {"device": torch.cuda.get_device_name(0), "n": n, "transcripts": w["transcripts"], "n_records": int(len(rec)), "n_barcodes": int(len(uniq)),
           "whitelist": {k: v for k, v in wstats.items() if k != "ms"}, "correct": {k: v for k, v in cst.items() if k not in ("ms", "neigh_ms")},
           "identical": bool(ok), "repeats": args.repeats, "ms": {k: [R.med(v), min(v), max(v)] for k, v in t.items()}}
    json.dump(out, open(os.path.join(work, "measure.json"), "w"))
    ctx.close()
    return 0 if ok else 1


def report(args, work):
    m = json.load(open(os.path.join(work, "measure.json")))
    nr, ms, wl, c = m["n_records"], m["ms"], m["whitelist"], m["correct"]
    row = lambda what, k, per: "| %s | %.2f (%.2f .. %.2f) | %.3g |" % (what, ms[k][0], ms[k][1], ms[k][2], per / ms[k][0] * 1e3)
    host = sum(ms[k][0] for k in ("host_download", "host_isin", "host_neigh"))
    n_miss = c["n_corrected"] + c["n_ambiguous"] + c["n_uncorrectable"]
    lines = ["# Barcode whitelist on the device (`kamd_bus_whitelist_create`, `kamd_bus_correct`): measured times", "",
             "Synthetic %s run of tools/bus_sc_rate.py: %d read sets, %d transcripts, one batch: %d records with %d distinct barcodes, mapped onto a synthetic whitelist of %d "
             "random %d-mers; 3 %% of the records then got one substituted base, 1 %% two.  Device: %s." % (R.TECH, m["n"], m["transcripts"], nr, m["n_barcodes"], wl["n_in"], BC_LEN, m["device"]),
             "The table: %d buckets of 64 bytes (%.0f MiB), %d distinct keys, max_chain %d.  The records: %d exact, %d corrected, %d ambiguous, %d uncorrectable; %d survive."
             % (wl["n_buckets"], wl["bytes"] / 2 ** 20, wl["n_distinct"], wl["max_chain"], c["n_exact"], c["n_corrected"], c["n_ambiguous"], c["n_uncorrectable"], c["n_out"]), "",
             "| what | ms (median of %d, min .. max) | items/s |" % m["repeats"], "|---|---|---|",
             row("`kamd_bus_whitelist_create`: upload of the codes (pageable), table build, read-back (the library's HIP events; per key)", "create", wl["n_in"]),
             row("`kamd_bus_correct`: all five launches and the read-back (the library's HIP events; per record)", "correct", nr),
             row("... of which `k_cor_neigh`, one wavefront per miss (per miss)", "neigh", n_miss),
             row("`kamd_bus_sort`, collapse on, on the corrected records in the same run (per record)", "sort", c["n_out"]),
             row("host path: download of the records (`tensor.cpu()`, pageable)", "host_download", nr),
             row("host path: `np.isin(barcodes, whitelist)`", "host_isin", nr),
             row("host path: the 48 neighbours of the misses, `np.searchsorted` in the list sorted beforehand (per miss)", "host_neigh", n_miss), "",
             "`k_cor_neigh` is %.0f %% of `kamd_bus_correct`.  Correct takes %.2f x the time of the sort it feeds (%.2f ms against %.2f ms)."
             % (100.0 * ms["neigh"][0] / ms["correct"][0], ms["correct"][0] / ms["sort"][0], ms["correct"][0], ms["sort"][0]),
             "The host path sums to %.1f ms: %.0f x the device call.  The device's statuses and corrected barcodes are %s the host path's."
             % (host, host / ms["correct"][0], "identical to" if m["identical"] else "DIFFERENT FROM"), ""]
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
    ap.add_argument("--whitelist", type=int, default=6794880, help="barcodes on the synthetic whitelist")
    ap.add_argument("--cache", default=None, help="directory that keeps the index between runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bus_correct_rate.md"))
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--work", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return STEPS[args.step][0](args, args.work)
    with tempfile.TemporaryDirectory() as work:
        for step in ("prepare", "measure", "report"):
            cmd = ["timeout", "-k", "10", str(STEPS[step][1]), sys.executable, os.path.abspath(__file__), "--step", step, "--work", work,
                   "--transcripts", str(args.transcripts), "--reads", str(args.reads), "--repeats", str(args.repeats), "--whitelist", str(args.whitelist), "--out", args.out]
            cmd += ["--cache", args.cache] if args.cache else []
            rc = subprocess.run(cmd).returncode
            if rc != 0:   # the first failure ends the run: nothing more is started
                print("bus_correct_rate.py: step %s failed (%d)" % (step, rc), file=sys.stderr)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
