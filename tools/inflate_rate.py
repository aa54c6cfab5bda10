"""Rate of the device-side inflate (`--inflate device`) beside the host inflate of the same build on the same BGZF file, in one run.
Not part of bench.py: the flagship line does not touch this path.

    python tools/inflate_rate.py [--pairs 2000000] [--rounds 3] [--case human_pe] [--out profiles/inflate_rate.md]

The reads are those of a golden case (so that they pseudoalign against its index), repeated to `--pairs` pairs and written with
synth_fastq.FastqText: headers and quality strings as a sequencer writes them, which is what decides how the text deflates.  The two
files are compressed as `bgzip` does (members of 65 280 bytes, zlib level 6).  Timed, alternating, `--rounds` times each: the front-end
from input to equivalence classes with `--inflate host -t 16` and with `--inflate device -t 16`.  The input waits for the index
(KAMD_FQ_NO_OVERLAP) and the time counts from the moment the index is on the device (`[timing] ... on the device after`) to `[timing] reads
parsed, packed and pseudoaligned after`: the input path alone, not the index load.  Beside these kamd_bgzf_inflate alone on the members of
mate 1 by HIP events, and its kernel with and without the CRC-32 / newline pass (kamd_debug_bgzf_inflate)."""
import argparse
import ctypes
import os
import re
import struct
import subprocess
import sys
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import common  # noqa: E402

EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
BLOCK = 65280


def bgzf_members(data, level=6):
    def one(a):
        chunk = bytes(data[a:a + BLOCK])
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        return co.compress(chunk) + co.flush(), zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(one, range(0, len(data), BLOCK)))


def bgzf_file(path, members):
    with open(path, "wb") as f:
        for comp, crc, n in members + [(b"\x03\x00", 0, 0)]:
            f.write(b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(comp) + 8 - 1)
                    + comp + struct.pack("<II", crc, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--case", default="human_pe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_rate.md"))
    args = ap.parse_args()
    import torch
    import kallisto_amd as ka
    from kallisto_amd import synth_fastq
    if not torch.cuda.is_available():
        sys.exit("inflate_rate.py measures on the GPU: no HIP device visible")
    meta, idx_path, r1, r2 = common.load_case(args.case)
    L = max(set(map(len, r1)), key=[len(r) for r in r1].count)
    keep = [i for i in range(len(r1)) if len(r1[i]) == L and len(r2[i]) == L]
    base = [np.stack([np.frombuffer(r[i], np.uint8) for i in keep]) for r in (r1, r2)]
    reps = -(-args.pairs // len(keep))
    med = lambda x: sorted(x)[len(x) // 2]
    lines = ["# Device-side inflate of BGZF FASTQ (`--inflate device`): measured rate", ""]
    with tempfile.TemporaryDirectory() as tmp:
        files, sizes, members1 = [], [], None
        for mate in (0, 1):
            reads = np.tile(base[mate], (reps, 1))[:args.pairs]
            fq = os.path.join(tmp, "r_%d.fastq" % (mate + 1))
            synth_fastq.write_fastq(fq, reads, mate=mate)
            data = np.fromfile(fq, np.uint8)
            mem = bgzf_members(memoryview(data))
            gz = fq + ".gz"
            bgzf_file(gz, mem)
            files.append(gz); sizes.append((len(data), os.path.getsize(gz)))
            if mate == 0:
                members1 = mem
            os.remove(fq)
        text_mb, comp_mb = sum(s[0] for s in sizes) / 1e6, sum(s[1] for s in sizes) / 1e6
        rates, whole = {"host": [], "device": []}, {"host": [], "device": []}
        notes = {}
        for rnd in range(args.rounds):
            for mode in ("host", "device"):
                p = subprocess.run([EXE, "quant", "-i", idx_path, "-o", os.path.join(tmp, "out_" + mode), "--plaintext", "--verbose", "-t", "16", "--inflate", mode, *files],
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, KAMD_FQ_NO_OVERLAP="1"), timeout=300)
                err = p.stderr.decode()
                if p.returncode != 0:
                    sys.exit("quant --inflate %s failed:\n%s" % (mode, err[-3000:]))
                m = re.search(r"reads parsed, packed and pseudoaligned after ([0-9.eE+-]+) s", err)
                ready = re.search(r"on the device after ([0-9.eE+-]+) s", err)
                rates[mode].append(args.pairs / (float(m.group(1)) - float(ready.group(1))))
                whole[mode].append(args.pairs / float(m.group(1)))
                t = [l for l in err.splitlines() if l.startswith("[timing] device inflate:")]
                if t:
                    notes["device"] = t[-1]
        same = open(os.path.join(tmp, "out_host", "abundance.tsv"), "rb").read() == open(os.path.join(tmp, "out_device", "abundance.tsv"), "rb").read()
        # the kernel alone: the members of mate 1 (at most 4000 of them), resident
        mem = members1[:4000]
        comp = b"".join(m[0] for m in mem)
        layout, so, do = [], 0, 0
        for c, crc, n in mem:
            layout.append((so, len(c), n, crc, do)); so += len(c); do += n
        ctx = ka.Context(0)
        d_comp = torch.frombuffer(bytearray(comp + b"\0" * 8), dtype=torch.uint8).cuda()
        d_text = torch.zeros(do + 64, dtype=torch.uint8, device="cuda")
        ms = []
        for rep in range(2 + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            res = ctx.bgzf_inflate(d_comp, layout, d_text, comp_bytes=len(comp), text_cap=do)
            e1.record(ctx.stream)
            e1.synchronize()
            assert res["status"] == 0
            if rep >= 2:
                ms.append(e0.elapsed_time(e1))
        kms = {True: [], False: []}
        for rep in range(1 + 5):
            for check in (True, False):
                res = ctx.bgzf_inflate(d_comp, layout, d_text, comp_bytes=len(comp), text_cap=do, debug_check_crc=check)
                assert res["status"] == 0
                if rep >= 1:
                    kms[check].append(res["kernel_ms"])
    try:
        ctypes.CDLL("libdeflate.so.0"); host_lib = "libdeflate (found on this box: the host path binds it at run time)"
    except OSError:
        host_lib = "zlib (no libdeflate on this box)"
    dev = torch.cuda.get_device_properties(0)
    lines += ["Box: %s, %d CUs; the front-end runs with `-t 16`.  Host inflate library: %s." % (dev.name, dev.multi_processor_count, host_lib), "",
              "Input: %d pairs of %d nt (the reads of `%s` repeated), text written by `synth_fastq.FastqText`: %.0f MB of text in the two files, %.0f MB as BGZF "
              "(members of 65 280 bytes, zlib level 6)." % (args.pairs, L, args.case, text_mb, comp_mb), "",
              "| input -> equivalence classes | M pairs/s from the index being on the device (median of %d, min .. max) | M pairs/s of the whole process up to the ECs, index load included |" % args.rounds,
              "|---|---|---|"]
    for mode in ("host", "device"):
        r, w = [x / 1e6 for x in rates[mode]], [x / 1e6 for x in whole[mode]]
        lines.append("| `--inflate %s -t 16` | %.2f (%.2f .. %.2f) | %.2f |" % (mode, med(r), min(r), max(r), med(w)))
    lines += ["", "The two paths wrote %s `abundance.tsv`." % ("byte-identical" if same else "DIFFERENT"), ""]
    if "device" in notes:
        lines += ["Last device run: `%s`" % notes["device"], ""]
    t = med(ms)
    lines += ["`kamd_bgzf_inflate` alone (HIP events around the call: member list upload, `k_bgzf_inflate` with its CRC-32 and newline count, the per-member result read-back), "
              "%d members, median of 5 after 2 warm-up calls: %.2f ms (%.2f .. %.2f) = %.2f GB/s of text, %.2f GB/s of compressed bytes."
              % (len(mem), t, min(ms), max(ms), do / t / 1e6, len(comp) / t / 1e6), "",
              "`k_bgzf_inflate` itself (HIP events around the launch, median of 5, alternating): %.2f ms with its CRC-32 / newline pass, %.2f ms without "
              "(`kamd_debug_bgzf_inflate`): the check is %.1f %% of the kernel." % (med(kms[True]), med(kms[False]), 100.0 * (med(kms[True]) - med(kms[False])) / med(kms[True])), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
