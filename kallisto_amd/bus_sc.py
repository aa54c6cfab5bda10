"""`kallisto bus -x <technology>` over the library: a small Python driver that writes a `kallisto bus` output directory for a barcode / UMI technology.

    python -m kallisto_amd.bus_sc -x TECH -i index.idx -o out [--fr-stranded|--rf-stranded|--unstranded] [--no-jump] [--union] [--bus-per-read] [--count] [--genecounts -g T2G] [-w WHITELIST] files...

TECH is a technology name (10XV3, SURECELL, INDROPSV2, VASA-SEQ, ...) or a custom "bc:umi:seq" string (BusLayout.parse); the files come in sets of the
technology's file count, plain or gzip.  Per batch of UNIT_RECORDS read sets the driver runs

    reset -> bus_split -> pseudoalign -> finalize -> read_ecs -> bus_records -> [bus_correct] -> bus_sort (the batch's classes as its map) -> download of the batch's classes

Class ids are batch-local; they are mapped to the ids of matrix.ec by transcript set, batch by batch in order of first appearance (the new sets of a batch in ascending order), so the input is read once and
nothing of a batch is kept but its records.  The records stay on the device: every batch's are sorted and collapsed there (kamd_bus_sort), the
sorted chunks are merged by sorting their concatenation whenever more than merge_records records have come in since the last merge, and only the
run's final records are downloaded.  output.bus holds them sorted by barcode, UMI, class and flags and collapsed with summed counts
(--bus-per-read: one record per read); its header lengths are the layout's fixed sums or the modes of the run's length histograms.  run_info.json:
n_reads = read sets read, n_processed = those that survive the drop rules (a part of barcode or UMI outside its read), n_pseudoaligned, n_unique.

--count: what `bustools count` makes of output.bus, into out/counts/: output.mtx (MatrixMarket coordinate integer, rows = barcodes, columns =
classes, 1-based, sorted by row then column), output.barcodes.txt (the rows' barcodes as bases), output.ec.txt (the classes: matrix.ec).  The matrix
is counted on the device (kamd_bus_count: distinct UMIs per (barcode, class), or reads where the layout has no UMI); a UMI whose records name
several classes is resolved here as bustools does: the transcript sets of its classes are intersected, an empty intersection drops the UMI,
otherwise it counts 1 for the class of the intersection, which is appended to matrix.ec when it is new.  `kallisto_amd_quant quant-tcc -e
counts/output.ec.txt counts/output.mtx` takes the result.

--genecounts -g T2G: what `bustools count --genecounts -g T2G` makes of output.bus, into out/genes/: output.mtx (rows = barcodes, columns = genes in
the order of their first appearance in T2G, the layout of --count's file), output.barcodes.txt, output.genes.txt and count.json.  T2G names a gene
for transcripts of the index (white-space separated columns: transcript, gene[, common name]); a transcript it does not name has no gene.  After the
last merge the gene lists of the run's classes are built on the device (kamd_bus_genes_create) and the run's records are counted there
(kamd_bus_count_genes): per UMI the gene lists of its classes are intersected, exactly one gene left counts 1 for it, none or several drop the UMI;
where the layout has no UMI every record whose class has one gene adds its count.  No record is looked at on the host.  The counters (n_barcodes,
n_umis, n_counted, n_no_gene, n_multi_gene) go into genes/count.json and, with the prefix genes_, into the dict run() returns.  Works with or
without --count (the classes --count appends to matrix.ec are named by no record).  Refused: --genecounts without -g, -g without --genecounts, a bad
map (the parser's text).

-w / --whitelist FILE: what `bustools correct` does between the records and their sort.  FILE lists the technology's barcodes, one per line, plain
or gzip.  Every batch's records go through kamd_bus_correct: a record whose barcode is on the list is kept, one whose barcode is one substitution
away from exactly one listed barcode takes that barcode, every other record is dropped.  output.bus and --count then hold listed barcodes only.
The four counters (n_exact, n_corrected, n_ambiguous, n_uncorrectable) go into out/correct.json and into the dict run() returns; run_info.json keeps
the reference's keys and meanings, n_pseudoaligned is counted before the correction.  Refused where the layout has no barcode, where a barcode part
is open-ended, and where the barcode's length differs from the list's.

This is a driver for moderate inputs: the collapsed records of the whole run are held in device memory and the FASTQ text is read through Python.  It is not the
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
MERGE_RECORDS = 1 << 25  # records that come in between two merges of the sorted chunks


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


def run(technology, index_path, out_dir, files, strand=None, no_jump=False, union=False, per_read=False, unit_records=UNIT_RECORDS, device=0, call="", count=False,
        merge_records=MERGE_RECORDS, whitelist=None, genecounts=False, genemap=None):
    layout, default_strand = A.BusLayout.parse(technology)
    if genecounts and not genemap:
        raise A.KallistoAmdError("--genecounts needs a transcripts-to-genes file: -g FILE")
    if genemap and not genecounts:
        raise A.KallistoAmdError("-g/--genemap is only used with --genecounts")
    wl_codes = _read_whitelist(whitelist, layout, technology) if whitelist else None
    if strand is None:
        strand = default_strand
    if len(files) == 0 or len(files) % layout.n_files:
        raise A.KallistoAmdError(f"Number of files ({len(files)}) does not match number of input files required by technology {technology} ({layout.n_files})")
    start_time = time.ctime()
    index = A.Index(index_path)
    gm = A.genemap_read(genemap, index.target_names()) if genecounts else None   # (a bad map: refused before anything runs)
    ctx = A.Context(device)
    ctx.upload(index)
    opts = A.QuantOpts(0, 200.0, 20.0, 1, strand, 1 if no_jump else 0, 1 if union else 0)   # what `bus` runs single-end reads with
    ec_of, ec_sets = {}, []          # transcript set -> id of matrix.ec, in order of first appearance
    chunks, since_merge = [], 0      # sorted device chunks of records, classes already global; records that came in since the last merge
    torch = ctx.torch
    wl = ctx.bus_whitelist(wl_codes[0], wl_codes[1]) if wl_codes else None
    corrected = dict.fromkeys(CORRECT_KEYS, 0)

    def merge():
        """the chunks held -> one sorted (and, unless per_read, collapsed) chunk"""
        if len(chunks) > 1:
            both, _ = ctx.bus_sort(torch.cat(chunks), None, collapse=not per_read)
            chunks[:] = [both.clone()]   # (the copy lets go of the records the collapse left behind)
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
                d_rec = ctx.bus_records(sp["tags"], d_ec, nv)
                # batch-local rows -> ids of matrix.ec.  The rows of a finalized result come in no fixed order, so the sets a batch brings in
                # are numbered in ascending order of their transcripts: two runs over the same input write the same bytes
                row_to_ec = np.zeros(max(len(ecs.counts), 1), np.int32)
                keys = [tuple(ecs.ec_ids[int(ecs.ec_off[r]):int(ecs.ec_off[r + 1])].tolist()) for r in range(len(ecs.counts))]
                for key in sorted(k for k in keys if k not in ec_of):
                    ec_of[key] = len(ec_sets)
                    ec_sets.append(key)
                for r, key in enumerate(keys):
                    row_to_ec[r] = ec_of[key]
                    if len(key) == 1:
                        n_unique += int(ecs.counts[r])
                n_pseudoaligned += int(d_rec.shape[0])   # (before the correction: what the reference counts)
                if wl is not None:
                    d_rec, cst = ctx.bus_correct(wl, d_rec)
                    for k in CORRECT_KEYS:
                        corrected[k] += cst[k]
                if d_rec.shape[0] == 0:
                    continue
                srt, _ = ctx.bus_sort(d_rec, torch.from_numpy(row_to_ec).to(d_rec.device), collapse=not per_read)
                chunks.append(srt.clone())
                since_merge += int(d_rec.shape[0])
                if since_merge > merge_records:
                    merge()
                    since_merge = 0
        finally:
            for h in handles:
                h.close()
    merge()
    d_all = chunks[0] if chunks else torch.zeros((0, 4), dtype=torch.int64, device=f"cuda:{device}")
    rec = A.bus_records_numpy(d_all)
    bclen, umilen = layout.header_lens(bc_hist, umi_hist)
    os.makedirs(out_dir, exist_ok=True)
    gene_counted = _genecount(ctx, d_all, layout, gm, ec_sets, bclen, os.path.join(out_dir, "genes")) if genecounts else {}   # (before --count: the run's own classes)
    counted = _count(ctx, d_all, layout, ec_of, ec_sets, bclen, os.path.join(out_dir, "counts")) if count else {}
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
    if wl is not None:
        with open(os.path.join(out_dir, "correct.json"), "w") as f:
            json.dump(corrected, f, indent=1)
            f.write("\n")
        counted = dict(counted, **corrected)
    counted = dict(counted, **{"genes_" + k: v for k, v in gene_counted.items()})
    info = dict(info, **counted)   # (run_info.json keeps the reference's keys)
    return info


CORRECT_KEYS = ("n_exact", "n_corrected", "n_ambiguous", "n_uncorrectable")


def _read_whitelist(path, layout, technology):
    """the whitelist file of -w -> (codes, barcode length), or the reason why this technology's records cannot be corrected against it"""
    parts = layout.parts("bc")
    if parts[0][0] < 0:
        raise A.KallistoAmdError(f"-w/--whitelist: technology {technology} has no barcode")
    if any(stop == 0 for _, _, stop in parts):
        raise A.KallistoAmdError(f"-w/--whitelist: a barcode part of technology {technology} is open-ended: its barcodes have no fixed length")
    tech_len = sum(stop - start for _, start, stop in parts)
    codes, wl_len = A.bus_whitelist_read(path)
    if wl_len != tech_len:
        raise A.KallistoAmdError(f"barcode length of whitelist ({wl_len}) differs from the technology's ({tech_len})")
    return codes, wl_len


def count_mode(layout):
    """distinct UMIs per (barcode, class), or reads where the layout has no UMI"""
    return A.BUS_COUNT_READS if layout.parts("umi")[0][0] < 0 else A.BUS_COUNT_UMIS


def resolve_multi(multi, matrix, ec_of, ec_sets):
    """the rule of `bustools count` for a UMI whose records name several classes, restated: multi = the host copy of Context.bus_count's multi records,
    matrix = {(row, class): value} of its entries.  Per group the transcript sets of its classes are intersected; an empty intersection drops the
    group, otherwise it adds 1 to (row, class of the intersection), a new class being appended to ec_sets / ec_of.  Returns the groups dropped."""
    groups = {}   # (row, UMI) -> classes: d_multi holds whole groups, each with its barcode's row in pad
    for row, umi, e in zip(multi["pad"].tolist(), multi["umi"].tolist(), multi["ec"].tolist()):
        groups.setdefault((row, umi), []).append(e)
    dropped = 0
    for (row, _), classes in groups.items():
        common = set(ec_sets[classes[0]])
        for e in classes[1:]:
            common &= set(ec_sets[e])
        if not common:
            dropped += 1
            continue
        key = tuple(sorted(common))
        e = ec_of.get(key)
        if e is None:
            e = ec_of[key] = len(ec_sets)
            ec_sets.append(key)
        matrix[(row, e)] = matrix.get((row, e), 0) + 1
    return dropped


def _count(ctx, d_rec, layout, ec_of, ec_sets, bclen, out_dir):
    """the run's sorted records -> out_dir/output.mtx, output.barcodes.txt, output.ec.txt (ec_sets grows by the classes the multi-class UMIs resolve to)"""
    c = ctx.bus_count(d_rec, count_mode(layout))
    ent = A.bus_entries_numpy(c["entries"])
    matrix = dict(zip(zip(ent["row"].tolist(), ent["ec"].tolist()), ent["value"].tolist()))
    resolve_multi(A.bus_records_numpy(c["multi"]), matrix, ec_of, ec_sets)
    barcodes = c["barcodes"].cpu().numpy().view(np.uint64)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "output.mtx"), "w") as f:
        f.write("%%MatrixMarket matrix coordinate integer general\n")
        f.write("%d\t%d\t%d\n" % (len(barcodes), len(ec_sets), len(matrix)))
        for (row, e), v in sorted(matrix.items()):
            f.write("%d\t%d\t%d\n" % (row + 1, e + 1, v))
    with open(os.path.join(out_dir, "output.barcodes.txt"), "w") as f:
        for b in barcodes.tolist():
            f.write("".join("ACGT"[(b >> (2 * (bclen - 1 - i))) & 3] for i in range(bclen)) + "\n")
    with open(os.path.join(out_dir, "output.ec.txt"), "w") as f:
        for e, s in enumerate(ec_sets):
            f.write("%d\t%s\n" % (e, ",".join(map(str, s))))
    st = c["stats"]
    return {"n_barcodes": st["n_barcodes"], "n_umis": st["n_umis"], "n_multi_umis": st["n_multi_groups"]}


GENE_KEYS = ("n_barcodes", "n_umis", "n_counted", "n_no_gene", "n_multi_gene")


def _genecount(ctx, d_rec, layout, gm, ec_sets, bclen, out_dir):
    """the run's sorted records -> out_dir/output.mtx, output.barcodes.txt, output.genes.txt, count.json; gm = genemap_read's result"""
    tr_gene, names, _ = gm
    table = ctx.bus_genes(tr_gene, len(names), ec_sets)
    try:
        c = ctx.bus_count_genes(table, d_rec, count_mode(layout))
    finally:
        table.free()
    ent = A.bus_entries_numpy(c["entries"])
    barcodes = c["barcodes"].cpu().numpy().view(np.uint64)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "output.mtx"), "w") as f:
        f.write("%%MatrixMarket matrix coordinate integer general\n")
        f.write("%d\t%d\t%d\n" % (len(barcodes), len(names), len(ent)))
        for row, g, v in zip(ent["row"].tolist(), ent["ec"].tolist(), ent["value"].tolist()):   # (sorted by row, then gene: as the device leaves them)
            f.write("%d\t%d\t%d\n" % (row + 1, g + 1, v))
    with open(os.path.join(out_dir, "output.barcodes.txt"), "w") as f:
        for b in barcodes.tolist():
            f.write("".join("ACGT"[(b >> (2 * (bclen - 1 - i))) & 3] for i in range(bclen)) + "\n")
    with open(os.path.join(out_dir, "output.genes.txt"), "w") as f:
        for g in names:
            f.write(g + "\n")
    out = {k: c["stats"][k] for k in GENE_KEYS}
    with open(os.path.join(out_dir, "count.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


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
    ap.add_argument("--count", action="store_true", help="also write the barcodes x classes matrix of the records into <output-dir>/counts")
    ap.add_argument("--genecounts", action="store_true", help="also write the barcodes x genes matrix of the records into <output-dir>/genes (needs -g)")
    ap.add_argument("-g", "--genemap", metavar="FILE", help="transcripts-to-genes file of --genecounts: transcript, gene[, common name] per line")
    ap.add_argument("-w", "--whitelist", metavar="FILE", help="correct the records' barcodes against this list (one barcode per line, plain or gzip): what `bustools correct` does")
    ap.add_argument("--unit-records", type=int, default=UNIT_RECORDS, help=argparse.SUPPRESS)
    ap.add_argument("--merge-records", type=int, default=MERGE_RECORDS, help=argparse.SUPPRESS)
    ap.add_argument("files", nargs="+")
    a = ap.parse_args(argv)
    try:
        info = run(a.technology, a.index, a.output_dir, a.files, a.strand, a.no_jump, a.union, a.bus_per_read, a.unit_records, count=a.count, merge_records=a.merge_records, whitelist=a.whitelist,
                   genecounts=a.genecounts, genemap=a.genemap, call="python -m kallisto_amd.bus_sc " + " ".join(sys.argv[1:] if argv is None else argv))
    except A.KallistoAmdError as e:
        print("Error:", e, file=sys.stderr)
        return 1
    print("[bus] processed %d of %d read sets, %d pseudoaligned" % (info["n_processed"], info["n_reads"], info["n_pseudoaligned"]), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
