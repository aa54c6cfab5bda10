"""Golden fixtures for the barcode / UMI technologies (`kallisto bus -x <technology>`), produced by the UNMODIFIED reference (oracle/_ref/kallisto, built
by `make -C oracle ref`).  Run in the build container:
    python tests/golden/make_bus_sc.py [case ...]

For every case of tests/bus_sc_common.CASES the cDNA reads of an existing fixture and the tag reads of the generator there (no read file is committed:
the tests build the same reads) are written as FASTQ and run through

    kallisto bus -x <technology> -t 1 [strand flag] -i index.idx -o out files...

and tests/golden/bus_sc/<case>/ keeps
    case.json         the command line, the BUS header, the numbers of run_info.json (`reference_run_info`; `n_processed` beside it is the number of
                      read sets that survive the drop rules, which the reference's own n_processed includes), the reads dropped, and the corner counts (all asserted non-zero
                      here where the layout has the field, so that no case can silently stop testing its corner)
    expected.txt.gz   one line "flags<TAB>barcode<TAB>umi<TAB>t0,t1,..." per record of the reference's output.bus (classes resolved through its
                      matrix.ec), sorted
Checked while generating: the reference drops at most 10 % of the reads; it processed exactly the reads the rules of kamd_bustag.h keep; its header is
the one tests/bus_sc_common.header_lens derives; it pseudoaligned no fewer reads than the oracle does of the surviving cut sequences (the share of the
underlying fixture's single-end reads, minus the dropped).  A case on which the reference crashes or writes nothing gets no directory and an entry in
tests/golden/bus_sc/dropped.json.
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
from tests import bus_sc_common as B  # noqa: E402
from tests import common  # noqa: E402
from tests.golden.make_bus_tcc import read_bus, read_ec, write_fastq  # noqa: E402

KALLISTO = os.path.join(ROOT, "oracle", "_ref", "kallisto")


def main():
    if not os.path.exists(KALLISTO):
        sys.exit("oracle/_ref is not built: run `make -C oracle ref` in the build container")
    only = sys.argv[1:]
    os.makedirs(B.GOLD, exist_ok=True)
    dropped_path = os.path.join(B.GOLD, "dropped.json")
    dropped = json.load(open(dropped_path)) if os.path.exists(dropped_path) else {}
    for name, c in B.CASES.items():
        if only and name not in only:
            continue
        L, strand, items, names = B.case_reads(name)
        lay = L.as_dict()
        _, idx, _, _ = common.load_case(c["fixture"])
        dst = os.path.join(B.GOLD, name)
        shutil.rmtree(dst, ignore_errors=True)
        dropped.pop(name, None)
        with tempfile.TemporaryDirectory() as tmp:
            files = [os.path.join(tmp, "reads_%d.fq" % f) for f in range(lay["n_files"])]
            for f, p in enumerate(files):
                write_fastq(p, [it[f] for it in items])
            out = os.path.join(tmp, "bus")
            cmd = ["bus", "-x", c["tech"], "-t", "1", "-i", idx, "-o", out, *c["flags"], *files]
            p = subprocess.run([KALLISTO, *cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            if p.returncode != 0 or not os.path.exists(os.path.join(out, "output.bus")):
                dropped[name] = {"command": cmd[:6], "returncode": p.returncode, "stderr_tail": p.stderr.decode(errors="replace")[-400:]}
                print(name, "DROPPED: the reference failed", p.returncode)
                continue
            hdr, rec = read_bus(os.path.join(out, "output.bus"))
            ecs = read_ec(os.path.join(out, "matrix.ec"))
            info = json.load(open(os.path.join(out, "run_info.json")))
        assert all(int(r["count"]) == 1 for r in rec)
        surv, st = B.py_split(lay, items)
        n = len(items)
        # run_info.json's n_processed is every read set the reader delivered (MasterProcessor::update adds seqs.size() / nfiles, src/ProcessReads.cpp:1372):
        # the sets processBuffer `continue`s over are in it, and nothing the reference writes counts them.  The drops are therefore the rules' own;
        # what the reference shows of them is that no record comes from such a read (the multiset the tests compare).
        assert int(info["n_processed"]) == n, (name, info["n_processed"], n)
        n_drop = n - st["n_valid"]
        assert n_drop == st["n_dropped_umi"] + st["n_dropped_bc"] and n_drop <= 0.10 * n, (name, n_drop, n)
        assert tuple(hdr[1:]) == B.header_lens(lay, st), (name, hdr, B.header_lens(lay, st))
        want_aligned = sum(1 for _, s in B.oracle_sets(name) if s)
        assert len(rec) >= want_aligned and int(info["n_pseudoaligned"]) == len(rec), (name, len(rec), want_aligned, info["n_pseudoaligned"])
        lines = sorted((int(r["flags"]), int(r["bc"]), int(r["umi"]), ecs[int(r["ec"])]) for r in rec)
        # corners: how often the generator placed each (where the layout has the field), what of it is in the records
        corners = {k: names.count(k) for k in B.CORNERS}
        corners.update({"dropped_umi": st["n_dropped_umi"], "dropped_bc": st["n_dropped_bc"],
                        "records_flag_bc": sum(1 for l in lines if l[0] & 0xFF), "records_flag_umi": sum(1 for l in lines if l[0] >> 8),
                        "records_flag_both": sum(1 for l in lines if (l[0] & 0xFF) and (l[0] >> 8)),
                        "records_three_or_more_n": sum(1 for l in lines if (l[0] & 3) == 3 or ((l[0] >> 8) & 3) == 3),
                        "records_n_at_0": sum(1 for l in lines if (l[0] & 0xFF) in (1, 2, 3) or ((l[0] >> 8) & 0xFF) in (1, 2, 3)),
                        "records_umi_truncated": sum(1 for _, d in surv if d["umi_len"] > 32),
                        "records_empty_sequence": sum(1 for _, d in surv if len(d["seq"]) == 0),
                        "repeated_bc_umi_records": len(lines) - len({(l[1], l[2]) for l in lines})})
        must = list(B.CORNERS) + ["records_three_or_more_n", "records_n_at_0", "repeated_bc_umi_records"]
        has_bc, has_umi = lay["bc"][0][0] >= 0, lay["umi"][0][0] >= 0
        must += ["dropped_umi"] if has_umi and (not has_bc or max(b for _, _, b in lay["umi"]) >= max(b for _, _, b in lay["bc"]) or name == "open_umi") else []
        must += ["dropped_bc"] if has_bc and (not has_umi or (name != "open_umi" and max(b for _, _, b in lay["bc"]) > max(b for _, _, b in lay["umi"]))) else []
        must += ["records_flag_bc"] if has_bc else ["records_flag_umi"]
        must += ["records_flag_umi", "records_flag_both"] if has_umi and has_bc else []
        must += ["records_flag_umi"] if not has_umi else []   # the quirk: an absent UMI repeats the barcode's flag
        must += ["records_umi_truncated"] if name == "open_umi" else []
        must += ["records_empty_sequence"] if name == "vasa" else []
        for k in must:
            assert corners[k] > 0, (name, k, corners)
        os.makedirs(dst)
        with gzip.GzipFile(os.path.join(dst, "expected.txt.gz"), "wb", mtime=0) as f:
            for fl, bc, umi, s in lines:
                f.write(("%d\t%d\t%d\t%s\n" % (fl, bc, umi, ",".join(map(str, s)))).encode())
        json.dump({"technology": c["tech"], "fixture": c["fixture"], "reads": list(c["reads"]), "flags": c["flags"], "layout": lay, "default_strand": strand,
                   "command": ["kallisto", "bus", "-x", c["tech"], "-t", "1", "-i", "index.idx", "-o", "out", *c["flags"],
                               *["reads_%d.fq" % f for f in range(lay["n_files"])]],
                   "bus_header": [int(x) for x in hdr], "n_reads": n, "n_processed": st["n_valid"], "n_pseudoaligned": int(info["n_pseudoaligned"]),
                   "n_unique": int(info["n_unique"]), "n_dropped": n_drop,
                   "reference_run_info": {k: info[k] for k in ("n_processed", "n_pseudoaligned", "n_unique")}, "n_records": len(lines), "n_classes": len({l[3] for l in lines}),
                   "oracle_pseudoaligned_of_survivors": want_aligned, "corners": corners,
                   "reference": "pachterlab/kallisto v0.51.1, oracle/_ref/kallisto (unmodified sources), -t 1"},
                  open(os.path.join(dst, "case.json"), "w"), indent=1)
        print(name, "reads", n, "survivors", st["n_valid"], "records", len(lines), "header", list(hdr), "dropped", n_drop,
              "bytes", os.path.getsize(os.path.join(dst, "expected.txt.gz")))
    json.dump(dropped, open(dropped_path, "w"), indent=1)


if __name__ == "__main__":
    main()
