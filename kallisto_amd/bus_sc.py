"""`kallisto bus -x <technology>` over the library: a small Python driver that writes a `kallisto bus` output directory for a barcode / UMI technology.

    python -m kallisto_amd.bus_sc -x TECH -i index.idx -o out [--fr-stranded|--rf-stranded|--unstranded] [--no-jump] [--union] [--bus-per-read] files...

TECH is a technology name (10XV3, SURECELL, INDROPSV2, VASA-SEQ, ...) or a custom "bc:umi:seq" string (BusLayout.parse); the files come in sets of the
technology's file count, plain or gzip.  Per batch of UNIT_RECORDS read sets the driver runs

    reset -> bus_split -> pseudoalign -> finalize -> read_ecs -> bus_records -> download of the records and of the batch's classes

Class ids are batch-local; they are mapped to the ids of matrix.ec by transcript set, in order of first appearance, so the input is read once and
nothing of a batch is kept but its records.  output.bus holds the records sorted by barcode, UMI, class and flags and collapsed with summed counts
(--bus-per-read: one record per read); its header lengths are the layout's fixed sums or the modes of the run's length histograms.  run_info.json:
n_reads = read sets read, n_processed = those that survive the drop rules (a part of barcode or UMI outside its read), n_pseudoaligned, n_unique.

This is a driver for moderate inputs: records of the whole run are held in host memory and the FASTQ text is read through Python.  It is not the
streaming C++ front-end (`kallisto_amd_quant bus` takes `-x bulk` only): the product is the C ABI, which a front-end that parses `-x` itself binds.
"""
from __future__ import annotations

import argparse
import gzip
import json
import os
import sys
import time

import numpy as np

from . import api as A

UNIT_RECORDS = 1 << 20   # read sets per batch


def _open(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    return gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")


def _read_unit(handles, n_records):
    """up to n_records 4-line records from every file -> (list of texts, records read); the files must hold equally many records"""
    texts, counts = [], []
    for h in handles:
        lines = []
        for _ in range(4 * n_records):
            l = h.readline()
            if not l:
                break
            lines.append(l)
        if lines and not lines[-1].endswith(b"\n"):
            lines[-1] += b"\n"
        if len(lines) % 4:
            raise A.KallistoAmdError("a FASTQ file ends inside a record")
        texts.append(b"".join(lines))
        counts.append(len(lines) // 4)
    if len(set(counts)) != 1:
        raise A.KallistoAmdError("the files of a read set hold different numbers of records")
    return texts, counts[0]


def _pack_unit(ctx, texts, n_records, n_files):
    """the unit as a packed batch of n_records items: on the device (kamd_fastq_unit_pack), or, where the unit is not strict 4-line FASTQ to it
    (status != 0: an empty read, for one), through the host packer"""
    words, lens, n_items, max_len, status, _ = ctx.fastq_unit_pack(texts, n_records)
    if status == 0:
        return words, lens, n_items, max_len
    seqs = [t.split(b"\n")[1::4] for t in texts]
    seqs = [[s.rstrip(b"\r") for s in f] for f in seqs]
    flat = [seqs[f][i] for i in range(n_records) for f in range(n_files)]
    words, lens, max_len = ctx.pack_reads_host(flat)
    return words, lens, n_records, max_len


def run(technology, index_path, out_dir, files, strand=None, no_jump=False, union=False, per_read=False, unit_records=UNIT_RECORDS, device=0, call=""):
    layout, default_strand = A.BusLayout.parse(technology)
    if strand is None:
        strand = default_strand
    if len(files) == 0 or len(files) % layout.n_files:
        raise A.KallistoAmdError(f"Number of files ({len(files)}) does not match number of input files required by technology {technology} ({layout.n_files})")
    start_time = time.ctime()
    index = A.Index(index_path)
    ctx = A.Context(device)
    ctx.upload(index)
    opts = A.QuantOpts(0, 200.0, 20.0, 1, strand, 1 if no_jump else 0, 1 if union else 0)   # what `bus` runs single-end reads with
    ec_of, ec_sets = {}, []          # transcript set -> id of matrix.ec, in order of first appearance
    chunks = []                      # the records of every batch, classes already global
    bc_hist, umi_hist = np.zeros(33, np.uint64), np.zeros(33, np.uint64)
    n_reads = n_processed = n_pseudoaligned = n_unique = 0
    for s in range(0, len(files), layout.n_files):
        handles = [_open(f) for f in files[s:s + layout.n_files]]
        try:
            while True:
                texts, n_rec = _read_unit(handles, unit_records)
                if n_rec == 0:
                    break
                n_reads += n_rec
                words, lens, n_items, max_len = _pack_unit(ctx, texts, n_rec, layout.n_files)
                ctx.reset()
                sp = ctx.bus_split(layout, words, lens, n_items, max_len)
                st = sp["stats"]
                bc_hist += np.array(st["bc_len_hist"], np.uint64)
                umi_hist += np.array(st["umi_len_hist"], np.uint64)
                nv = sp["n_valid"]
                n_processed += nv
                if nv == 0:
                    continue
                ctx.pseudoalign(opts, sp["seq_words"], sp["seq_len"], nv, sp["seq_max_len"])
                ecs = ctx.finalize()
                d_ec, _ = ctx.read_ecs(opts, sp["seq_words"], sp["seq_len"], nv, sp["seq_max_len"])
                rec = A.bus_records_numpy(ctx.bus_records(sp["tags"], d_ec, nv)).copy()
                # batch-local rows -> ids of matrix.ec
                row_to_ec = np.zeros(max(len(ecs.counts), 1), np.int32)
                for r in range(len(ecs.counts)):
                    key = tuple(ecs.ec_ids[int(ecs.ec_off[r]):int(ecs.ec_off[r + 1])].tolist())
                    e = ec_of.get(key)
                    if e is None:
                        e = ec_of[key] = len(ec_sets)
                        ec_sets.append(key)
                    row_to_ec[r] = e
                    if len(key) == 1:
                        n_unique += int(ecs.counts[r])
                rec["ec"] = row_to_ec[rec["ec"]]
                n_pseudoaligned += len(rec)
                chunks.append(rec)
        finally:
            for h in handles:
                h.close()
    rec = np.concatenate(chunks) if chunks else np.zeros(0, A.BUS_RECORD_DTYPE)
    order = np.lexsort((rec["flags"], rec["ec"], rec["umi"], rec["barcode"]))
    rec = rec[order]
    if not per_read and len(rec):   # collapse equal (barcode, UMI, class, flags), counts summed
        first = np.ones(len(rec), bool)
        first[1:] = (rec["barcode"][1:] != rec["barcode"][:-1]) | (rec["umi"][1:] != rec["umi"][:-1]) | (rec["ec"][1:] != rec["ec"][:-1]) | (rec["flags"][1:] != rec["flags"][:-1])
        starts = np.flatnonzero(first)
        runs = np.diff(np.append(starts, len(rec)))
        assert runs.max() <= 0xFFFFFFFF   # (`count` is 32 bits; a run that long is beyond this driver)
        rec = rec[starts].copy()
        rec["count"] = runs
    bclen, umilen = layout.header_lens(bc_hist, umi_hist)
    os.makedirs(out_dir, exist_ok=True)
    text = b"BUS file produced by kallisto"
    with open(os.path.join(out_dir, "output.bus"), "wb") as f:
        f.write(b"BUS\0" + np.array([1, bclen, umilen, len(text)], "<u4").tobytes() + text)
        f.write(rec.tobytes())
    with open(os.path.join(out_dir, "matrix.ec"), "w") as f:
        for e, s in enumerate(ec_sets):
            f.write("%d\t%s\n" % (e, ",".join(map(str, s))))
    with open(os.path.join(out_dir, "transcripts.txt"), "w") as f:
        for n in index.target_names():
            f.write(n + "\n")
    p = lambda x: "%.1f" % (100.0 * x / n_processed if n_processed else 0.0)
    info = {"n_targets": int(index.num_targets), "n_bootstraps": 0, "n_reads": n_reads, "n_processed": n_processed, "n_pseudoaligned": n_pseudoaligned,
            "n_unique": n_unique, "p_pseudoaligned": float(p(n_pseudoaligned)), "p_unique": float(p(n_unique)), "kallisto_version": "0.51.1",
            "index_version": 13, "k-mer length": int(index.k), "start_time": start_time, "call": call}
    with open(os.path.join(out_dir, "run_info.json"), "w") as f:
        json.dump(info, f, indent=1)
        f.write("\n")
    return info


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m kallisto_amd.bus_sc", description="BUS records of a barcode / UMI technology on the GPU (a driver for moderate inputs)")
    ap.add_argument("-x", "--technology", required=True)
    ap.add_argument("-i", "--index", required=True)
    ap.add_argument("-o", "--output-dir", required=True)
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--fr-stranded", dest="strand", action="store_const", const=1)
    g.add_argument("--rf-stranded", dest="strand", action="store_const", const=2)
    g.add_argument("--unstranded", dest="strand", action="store_const", const=0)
    ap.add_argument("--no-jump", action="store_true")
    ap.add_argument("--union", action="store_true")
    ap.add_argument("--bus-per-read", action="store_true")
    ap.add_argument("--unit-records", type=int, default=UNIT_RECORDS, help=argparse.SUPPRESS)
    ap.add_argument("files", nargs="+")
    a = ap.parse_args(argv)
    try:
        info = run(a.technology, a.index, a.output_dir, a.files, a.strand, a.no_jump, a.union, a.bus_per_read, a.unit_records,
                   call="python -m kallisto_amd.bus_sc " + " ".join(sys.argv[1:] if argv is None else argv))
    except A.KallistoAmdError as e:
        print("Error:", e, file=sys.stderr)
        return 1
    print("[bus] processed %d of %d read sets, %d pseudoaligned" % (info["n_processed"], info["n_reads"], info["n_pseudoaligned"]), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
