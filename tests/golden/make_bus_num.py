"""Golden fixtures for `bus -n / --num` (one BUS record per pseudoaligned read, the read's number in `flags`, src/ProcessReads.cpp:1747-1749),
produced by the UNMODIFIED reference (oracle/_ref/kallisto, built by `make -C oracle ref`).  Run in the build container:
    python tests/golden/make_bus_num.py

For every case below the reads of an existing fixture are cut into samples (no new read files are committed: the tests cut the same fixtures
the same way) and run through

    kallisto bus -n -x bulk -t 1 [--paired] [variant flags] -i index.idx  sample files... | -B batch.txt

and tests/golden/bus_num/<case>/ keeps
    case.json         the command line, the cuts, how the numbers run (`numbering`: "run" = one count over all files of the command line,
                      "entry" = every line of the batch file starts at 0 again -- decided by what the reference wrote), and the counts of
                      records, of distinct classes and of reads without a record
    expected.txt.gz   one line per record, "flags<TAB>barcode<TAB>t0,t1,..." (class ids resolved through the reference's matrix.ec), sorted
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import common  # noqa: E402
from tests.golden.make_bus_tcc import read_bus, read_ec, write_fastq  # noqa: E402

KALLISTO = os.path.join(ROOT, "oracle", "_ref", "kallisto")
OUT = os.path.join(common.GOLDEN, "bus_num")

# name: (fixture, sample boundaries as fractions, bus flags, ids of a batch file or None = the files go on the command line)
CASES = {
    "ref_test_pe": ("ref_test_pe", [0.0, 0.45, 1.0], ["--paired"], None),
    "yeast_se": ("yeast_se", [0.0, 0.3, 0.7, 1.0], [], ["A", "B", "A"]),
    "mosaic_pe": ("mosaic_pe", [0.0, 0.5, 1.0], ["--paired", "--fr-stranded"], None),
}


def sample_ranges(n, cuts):
    return [(int(round(cuts[s] * n)), int(round(cuts[s + 1] * n))) for s in range(len(cuts) - 1)]


def barcodes_of(ids, n_samples):
    """batch_id_mapping: lines with the same id share a barcode; files on the command line are batch0, batch1, ..."""
    if ids is None:
        return list(range(n_samples))
    seen = {}
    return [seen.setdefault(i, len(seen)) for i in ids]


def main():
    if not os.path.exists(KALLISTO):
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` in the build container")
    only = sys.argv[1:]
    for name, (fixture, cuts, bus_flags, ids) in CASES.items():
        if only and name not in only:
            continue
        meta, idx, r1, r2 = common.load_case(fixture)
        paired = "--paired" in bus_flags
        ranges = sample_ranges(len(r1), cuts)
        bcs = barcodes_of(ids, len(ranges))
        dst = os.path.join(OUT, name)
        shutil.rmtree(dst, ignore_errors=True)
        os.makedirs(dst)
        with tempfile.TemporaryDirectory() as tmp:
            files, shown = [], []
            for s, (a, b) in enumerate(ranges):
                fs = [os.path.join(tmp, "s%d_1.fq" % s)]
                write_fastq(fs[0], r1[a:b])
                if paired:
                    fs.append(os.path.join(tmp, "s%d_2.fq" % s))
                    write_fastq(fs[1], r2[a:b])
                files.append(fs)
                shown.append([os.path.basename(f) for f in fs])
            bus_out = os.path.join(tmp, "bus")
            if ids is None:
                inputs = [f for fs in files for f in fs]
                shown_inputs = [f for fs in shown for f in fs]
            else:
                bf = os.path.join(tmp, "batch.txt")
                with open(bf, "w") as f:
                    for i, fs in zip(ids, files):
                        f.write(" ".join([i] + fs) + "\n")
                inputs = ["-B", bf]
                shown_inputs = ["-B", "batch.txt"]
            p = subprocess.run([KALLISTO, "bus", "-n", "-x", "bulk", "-t", "1", "-i", idx, "-o", bus_out, *bus_flags, *inputs],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 0, p.stderr.decode()
            hdr, rec = read_bus(os.path.join(bus_out, "output.bus"))
            ecs = read_ec(os.path.join(bus_out, "matrix.ec"))
        assert all(int(r["count"]) == 1 and int(r["umi"]) == 2 ** 64 - 1 for r in rec)
        # how do the numbers run?  "run": the records of line s carry numbers of [a_s, b_s); "entry": numbers below the line's own size
        by_bc = {}
        for s, (a, b) in enumerate(ranges):
            by_bc.setdefault(bcs[s], []).append((a, b))
        h_run = all(any(a <= int(r["flags"]) < b for a, b in by_bc[int(r["bc"])]) for r in rec)
        h_entry = all(int(r["flags"]) < max(b - a for a, b in by_bc[int(r["bc"])]) for r in rec)
        assert h_run != h_entry, (name, h_run, h_entry)
        lines = sorted((int(r["flags"]), int(r["bc"]), ecs[int(r["ec"])]) for r in rec)
        with gzip.GzipFile(os.path.join(dst, "expected.txt.gz"), "wb", mtime=0) as f:
            for fl, bc, s in lines:
                f.write(("%d\t%d\t%s\n" % (fl, bc, ",".join(map(str, s)))).encode())
        n_reads = ranges[-1][1]
        json.dump({"fixture": fixture, "cuts": cuts, "bus_flags": bus_flags, "batch_ids": ids,
                   "command": ["kallisto", "bus", "-n", "-x", "bulk", "-t", "1", "-i", "index.idx", "-o", "out", *bus_flags, *shown_inputs],
                   "samples": shown, "numbering": "run" if h_run else "entry", "bus_header": list(hdr),
                   "n_reads": n_reads, "n_records": int(len(rec)), "n_classes": len({l[2] for l in lines}), "n_reads_without_record": n_reads - int(len(rec)),
                   "oracle_disagrees_on_reads": [],
                   "reference": "pachterlab/kallisto v0.51.1, oracle/_ref/kallisto (unmodified sources), -t 1"},
                  open(os.path.join(dst, "case.json"), "w"), indent=1)
        print(name, "samples", len(ranges), "reads", n_reads, "records", len(rec), "numbering", "run" if h_run else "entry",
              "bytes", os.path.getsize(os.path.join(dst, "expected.txt.gz")))


if __name__ == "__main__":
    main()
