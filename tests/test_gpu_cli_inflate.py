"""`--inflate device` of the front-end (kallisto_amd/kallisto_amd_quant, kamd_inflate_feed.h) against `--inflate host` of the same binary on the
same BGZF files: byte-identical outputs, the host path's errors.  One-shot runs on the 3000 pairs of the golden case k21_pe."""
import json
import os
import re
import struct
import subprocess
import zlib

import pytest

from tests import common
from tests.test_fastq_input import _bgzf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kallisto_amd", "kallisto_amd_quant")
SMALL_UNITS = {"KAMD_FQ_UNIT_BYTES": "4096", "KAMD_FQ_BATCH_ITEMS": "500"}


def _text(reads, final_newline=True):
    t = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    return t if final_newline else t[:-1]


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


@pytest.fixture(scope="module")
def case():
    assert os.path.exists(EXE), "build kallisto_amd_quant with `make -C kallisto_amd/csrc all`"
    meta, idx_path, r1, r2 = common.load_case("k21_pe")
    return idx_path, r1, r2


ON_DEVICE = "[quant] BGZF input is inflated on the device"
GENERAL_READER = "reading it with the general FASTA/FASTQ reader"


def _device_units(stderr, small_units):
    """The device path ran, and ran to the end: its opening line, its closing `[timing] device inflate: N units` line, no fall-back to the host
    inflate and no restart with the general reader (a declined sample would pass every comparison with the host path).  With small units the
    input is dozens of units, so that tails are carried over."""
    assert ON_DEVICE in stderr, stderr[-2000:]          # (bus prints it behind its "finding pseudoalignments" prompt, not on a line of its own)
    assert "--inflate device:" not in stderr and GENERAL_READER not in stderr, stderr[-2000:]
    m = re.search(r"^\[timing\] device inflate: (\d+) units", stderr, flags=re.M)
    assert m, stderr[-2000:]
    n = int(m.group(1))
    assert n >= (24 if small_units else 1), n
    return n


def _device_ran_until_the_error(stderr):
    assert ON_DEVICE in stderr and "--inflate device:" not in stderr and GENERAL_READER not in stderr, stderr[-2000:]
    assert "[timing] device inflate:" not in stderr


def _quant(idx, out, files, mode, env=None, extra=()):
    return subprocess.run([EXE, "quant", "-i", idx, "-o", str(out), "--plaintext", "--verbose", "-t", "5", "--inflate", mode, *extra, *files],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=120)


def _same_quant(idx, tmp_path, files, env=None, extra=()):
    res = {}
    for mode in ("host", "device"):
        p = _quant(idx, tmp_path / mode, files, mode, env, extra)
        assert p.returncode == 0, (mode, p.stderr.decode()[-2000:])
        if mode == "device":
            _device_units(p.stderr.decode(), bool(env))
        else:
            assert ON_DEVICE not in p.stderr.decode()
        info = json.load(open(tmp_path / mode / "run_info.json"))
        res[mode] = (open(tmp_path / mode / "abundance.tsv", "rb").read(), [info[k] for k in ("n_processed", "n_pseudoaligned", "n_unique")])
    assert res["host"][1] == res["device"][1]
    assert res["host"][0] == res["device"][0]
    return res["device"][1]


@pytest.mark.parametrize("units", ["default", "small"])
def test_quant_paired_device_equals_host(case, tmp_path, units):
    idx, r1, r2 = case
    block = 3000 if units == "small" else 65280          # (a unit is at least one member: dozens of units need members smaller than the file's tenth)
    files = [_write(tmp_path / "r_1.fastq.gz", _bgzf(_text(r1), block=block)), _write(tmp_path / "r_2.fastq.gz", _bgzf(_text(r2), block=block))]
    n = _same_quant(idx, tmp_path, files, SMALL_UNITS if units == "small" else None)
    assert n[0] == len(r1)


def test_quant_single_end_device_equals_host(case, tmp_path):
    idx, r1, _ = case
    files = [_write(tmp_path / "r_1.fastq.gz", _bgzf(_text(r1), block=5000))]
    n = _same_quant(idx, tmp_path, files, SMALL_UNITS, extra=("--single", "-l", "200", "-s", "20"))
    assert n[0] == len(r1)


def test_tails_that_drift_apart_and_a_text_without_the_final_newline(case, tmp_path):
    idx, r1, r2 = case
    files = [_write(tmp_path / "r_1.fastq.gz", _bgzf(_text(r1, final_newline=False), block=97)),
             _write(tmp_path / "r_2.fastq.gz", _bgzf(_text(r2, final_newline=False), block=20000))]
    n = _same_quant(idx, tmp_path, files, SMALL_UNITS)
    assert n[0] == len(r1)


def test_eof_member_in_the_middle(case, tmp_path):
    idx, r1, r2 = case
    h = len(r1) // 2
    files = [_write(tmp_path / "r_1.fastq.gz", _bgzf(_text(r1[:h]), block=3000) + _bgzf(_text(r1[h:]), block=7000)),
             _write(tmp_path / "r_2.fastq.gz", _bgzf(_text(r2)))]
    # (the second half's records are numbered from 0 again: the names do not matter to quant)
    n = _same_quant(idx, tmp_path, files, SMALL_UNITS)
    assert n[0] == len(r1)


def _bus_classes(bus, ec):
    """output.bus + matrix.ec without the numbering of the classes: sorted (barcode, transcripts of the class, count)"""
    names = dict(l.split("\t") for l in ec.decode().splitlines())
    tlen = struct.unpack_from("<I", bus, 16)[0]
    rec = bus[20 + tlen:]
    assert len(rec) % 32 == 0
    out = []
    for o in range(0, len(rec), 32):
        bc, umi, e, cnt, flags, pad = struct.unpack_from("<QQiIII", rec, o)
        out.append((bc, names[str(e)], cnt))
    return sorted(out)


@pytest.mark.parametrize("units", ["default", "small"])
def test_bus_bulk_paired_device_equals_host(case, tmp_path, units):
    """The classes that occur, their transcripts and their counts per barcode are those of `--inflate host`.  The files are not compared byte for
    byte: matrix.ec numbers the classes in the order kamd_ec_download lists them, and that order is not stable from one run to the next of the
    host path itself (three `--inflate host` runs on this input gave three different numberings)."""
    idx, r1, r2 = case
    files = [_write(tmp_path / "r_1.fastq.gz", _bgzf(_text(r1), block=9000)), _write(tmp_path / "r_2.fastq.gz", _bgzf(_text(r2), block=11000))]
    out = {}
    for mode in ("host", "device"):
        p = subprocess.run([EXE, "bus", "-x", "bulk", "--paired", "-i", idx, "-o", str(tmp_path / mode), "--verbose", "-t", "5", "--inflate", mode, *files],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(SMALL_UNITS if units == "small" else {})), timeout=120)
        assert p.returncode == 0, (mode, p.stderr.decode()[-2000:])
        if mode == "device":
            _device_units(p.stderr.decode(), units == "small")
        else:
            assert ON_DEVICE not in p.stderr.decode()
        out[mode] = [open(tmp_path / mode / fn, "rb").read() for fn in ("output.bus", "matrix.ec")]
    assert len(out["device"][0]) > 100
    assert _bus_classes(*out["host"]) == _bus_classes(*out["device"])


def test_mates_with_different_record_counts(case, tmp_path):
    idx, r1, r2 = case
    for a, b in ((r1, r2[:-7]), (r1[:-500], r2)):
        files = [_write(tmp_path / "r_1.fastq.gz", _bgzf(_text(a), block=4000)), _write(tmp_path / "r_2.fastq.gz", _bgzf(_text(b), block=4000))]
        got = {}
        for mode in ("host", "device"):
            p = _quant(idx, tmp_path / mode, files, mode, SMALL_UNITS)
            err = [l for l in p.stderr.decode().splitlines() if l.startswith("Error:")]
            got[mode] = (p.returncode, err)
            if mode == "device":
                _device_ran_until_the_error(p.stderr.decode())
        assert got["host"][0] != 0 and got["host"][1] == ["Error: paired-end files have different numbers of reads"]
        assert got["device"] == got["host"]


def test_a_flipped_payload_bit_is_a_corrupt_block(case, tmp_path):
    idx, r1, _ = case
    data = bytearray(_bgzf(_text(r1), block=30000))
    bsize = struct.unpack_from("<H", data, 16)[0] + 1
    data[bsize + 18 + 2000] ^= 0x10                      # inside the second member's deflate stream
    files = [_write(tmp_path / "r_1.fastq.gz", bytes(data))]
    got = {}
    for mode in ("host", "device"):
        p = _quant(idx, tmp_path / mode, files, mode, extra=("--single", "-l", "200", "-s", "20"))
        got[mode] = (p.returncode != 0, [l for l in p.stderr.decode().splitlines() if "corrupt BGZF block" in l])
        if mode == "device":
            _device_ran_until_the_error(p.stderr.decode())
    assert got["host"][0] and got["host"][1] == [f"Error: {files[0]}: corrupt BGZF block 1"]
    assert got["device"] == got["host"]


def test_plain_gzip_falls_back_to_the_host_path(case, tmp_path):
    idx, r1, _ = case
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    files = [_write(tmp_path / "r_1.fastq.gz", co.compress(_text(r1)) + co.flush())]
    res = {}
    for mode in ("host", "device"):
        p = _quant(idx, tmp_path / mode, files, mode, extra=("--single", "-l", "200", "-s", "20"))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        res[mode] = (open(tmp_path / mode / "abundance.tsv", "rb").read(), p.stderr.decode())
    assert res["host"][0] == res["device"][0]
    line = f"[quant] --inflate device: {files[0]} is not BGZF (or the run uses several contexts); inflating on the host"
    # (written in one piece, but the index thread prints its own lines meanwhile: the line need not begin at the start of a line of stderr)
    assert line + "\n" in res["device"][1] and "--inflate device:" not in res["host"][1]
    assert ON_DEVICE not in res["device"][1]
