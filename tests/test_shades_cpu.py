"""An index with shades (targets named <base>_shade_<variant>) on the CPU: what the index loader makes of it, and the class rule of
kallisto_amd/csrc/kamd_core.h (for_each_in_shaded_set) driven by tests/emu_shade against the reference's goldens on tests/golden/shades_pe."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from tests import bigsets, common, shades


@pytest.fixture(scope="module")
def idx_path(tmp_path_factory):
    return shades.unpack_index(tmp_path_factory.mktemp("shades"))


@pytest.fixture(scope="module")
def ix(idx_path):
    x = shades.EmuIndex(idx_path)
    yield x
    x.close()


@pytest.fixture(scope="module")
def fixture():
    return shades.load_reads()


def test_loader_finds_shades_and_colours(ix, fixture):
    meta = fixture[0]
    assert ix.n_shades == meta["n_shades"] > 0 and ix.n_targets == meta["targets"]
    want = shades.colours_of_names(ix.names)
    assert np.array_equal(ix.colour, want)
    is_shade = ix.colour != shades.NOT_A_SHADE
    assert is_shade.sum() == ix.n_shades
    # every shade directly behind its family: ids interleave, the colour is the nearest earlier target that is no shade
    for s in np.flatnonzero(is_shade):
        assert ix.colour[s] == max(t for t in range(s) if not is_shade[t]) and ix.names[s].startswith(ix.names[ix.colour[s]] + shades.TAG)
    # the cores and the shade lists partition every set, in order; a set with a shade holds its colour (the index builder puts it there)
    n_ecs = len(ix.ec_off) - 1
    for e in range(n_ecs):
        full = ix.ec_ids[ix.ec_off[e]:ix.ec_off[e + 1]]
        core = ix.core_ids[ix.core_off[e]:ix.core_off[e + 1]]
        sh = ix.shade_ids[ix.shade_off[e]:ix.shade_off[e + 1]]
        assert np.array_equal(core, full[~is_shade[full]]) and np.array_equal(sh, full[is_shade[full]])
        assert set(ix.colour[sh].tolist()) <= set(core.tolist())
    # what case.json promises about the fixture: no path is covered by luck
    assert meta["core_size_histogram"] == bigsets.size_histogram(np.diff(ix.core_off))
    sizes = set(np.diff(ix.core_off).tolist())
    for b in (16, 17, 64, 65, 128, 129, 1024, 1025):
        assert b in sizes, f"no core of exactly {b} members"
    for key in ("pairs_with_shade_in_class", "pairs_with_orphan_mate", "pairs_with_more_than_12_sets"):
        assert meta[key] > 0
    assert meta["largest_shade_union"] > 16


@pytest.mark.parametrize("case", common.CASES)
def test_ordinary_indices_have_no_shades(case):
    x = shades.EmuIndex(common.load_case(case)[1])
    try:
        v = x.view
        assert x.n_shades == 0 and not v.shade_colour and not v.core_off and not v.core_ids and not v.shade_off and not v.shade_ids
    finally:
        x.close()


def test_orphan_shade_is_refused(idx_path, tmp_path, ix):
    """a shade whose base target does not come before it: the reference silently takes colour 0, the loader refuses the index"""
    raw = open(idx_path, "rb").read()
    s = int(np.flatnonzero(ix.colour != shades.NOT_A_SHADE)[0])
    base = ix.names[ix.colour[s]].encode()
    rec = struct.pack("<Q", len(base)) + base           # the name record of the base target: length, characters
    assert raw.count(rec) == 1
    bad = tmp_path / "orphan.idx"
    bad.write_bytes(raw.replace(rec, struct.pack("<Q", len(base)) + b"x" + base[1:]))
    L = shades.emu()
    h = C.c_void_p()
    assert L.kamd_index_load(os.fsencode(str(bad)), 2, C.byref(h)) == -3 and not h
    msg = L.kamd_last_error().decode()
    assert "shade" in msg and ix.names[s] in msg


@pytest.mark.parametrize("variant", shades.DUMP_VARIANTS)
def test_per_item_logic_reproduces_reference(variant, ix, fixture):
    meta, r1, r2 = fixture
    exp = shades.load_expected(variant)
    res = shades.emu_quant(ix, r1, r2, common.parse_variant(meta["variants"][variant]))
    assert res["nproc"] == exp["nproc"]
    assert res["ecs"] == exp["ecs"]
    assert np.array_equal(res["flens"], exp["flens"])
    if variant == "pe":   # a class {T} extended by T's shades feeds no fragment length: the sample is smaller than the one of the cores alone
        assert exp["flens"].sum() > 0 and any(len(e) > 1 and all(ix.colour[t] != shades.NOT_A_SHADE for t in e[1:]) for e in exp["ecs"])


def test_flattened_file_keeps_shade_tables(ix, tmp_path):
    """the file carries the tables (format 5), the loader reads them back and checks them against the sets: a file whose tables were tampered
    with is refused"""
    flat = str(tmp_path / "index.kamd")
    ix.save(flat)
    raw = open(flat, "rb").read()
    assert raw[:8] == b"KAMDFLT5"
    ids = ix.shade_ids.astype(np.uint32).tobytes()      # the last array of the file, before the target names
    at = raw.rfind(ids)
    assert at > 0
    bad = tmp_path / "bad.kamd"
    bad.write_bytes(raw[:at] + ids[4:] + ids[:4] + raw[at + len(ids):])     # the shade lists rotated by one entry
    h = C.c_void_p()
    assert shades.emu().kamd_index_load(os.fsencode(str(bad)), 2, C.byref(h)) == -3 and not h
    y = shades.EmuIndex(flat)
    try:
        assert y.n_shades == ix.n_shades and np.array_equal(y.colour, ix.colour)
        for a in ("core_off", "core_ids", "shade_off", "shade_ids", "ec_off", "ec_ids"):
            assert np.array_equal(getattr(y, a), getattr(ix, a)), a
    finally:
        y.close()


def test_set_with_a_shade_but_not_its_colour_is_refused(ix, tmp_path):
    """the reference's builder puts the colour into every set that gets a shade, and the class rule leans on it (an empty core is an empty set, a
    single set's class is the set itself): an index that breaks it is refused.  Here: a flattened file in which the set {colour, shade} of a
    shade's own k-mers names another target in the colour's place, in the sets and in the cores alike"""
    flat = str(tmp_path / "index.kamd")
    ix.save(flat)
    raw = open(flat, "rb").read()
    is_shade = ix.colour != shades.NOT_A_SHADE
    e = next(e for e in range(len(ix.ec_off) - 1) if ix.ec_off[e + 1] - ix.ec_off[e] == 2 and not is_shade[ix.ec_ids[ix.ec_off[e]]]
             and is_shade[ix.ec_ids[ix.ec_off[e] + 1]] and ix.ec_ids[ix.ec_off[e]] > 0)
    ec, core = ix.ec_ids.astype(np.uint32), ix.core_ids.astype(np.uint32)
    a, b = raw.find(ec.tobytes()), raw.find(core.tobytes())
    assert a > 0 and b > 0 and raw.count(ec.tobytes()) == 1 and raw.count(core.tobytes()) == 1
    ec[ix.ec_off[e]] = 0; core[ix.core_off[e]] = 0          # target 0 is no shade and smaller: the set stays sorted
    out = bytearray(raw)
    out[a:a + ec.nbytes] = ec.tobytes(); out[b:b + core.nbytes] = core.tobytes()
    bad = tmp_path / "bad.kamd"
    bad.write_bytes(bytes(out))
    h = C.c_void_p()
    assert shades.emu().kamd_index_load(os.fsencode(str(bad)), 2, C.byref(h)) == -3 and not h


def test_refused_option_combinations(ix):
    from kallisto_amd.api import QuantOpts
    L = shades.emu()
    mk = lambda paired, fld, sd, so, strand=0: QuantOpts(paired, fld, sd, so, strand)
    for o in (mk(0, 200.0, 20.0, 0), mk(1, 200.0, 20.0, 0), mk(1, 200.0, 20.0, 0, 1)):   # --single, paired with -l / -s
        assert L.kamd_index_check_opts(ix.h, C.byref(o)) == -5 and "shades" in L.kamd_last_error().decode()
    for o in (mk(0, 200.0, 20.0, 1), mk(1, 0.0, 0.0, 0), mk(1, 200.0, 20.0, 1, 2)):
        assert L.kamd_index_check_opts(ix.h, C.byref(o)) == 0
    plain = shades.EmuIndex(common.load_case("ref_test_pe")[1])   # an ordinary index takes them all
    try:
        assert L.kamd_index_check_opts(plain.h, C.byref(mk(0, 200.0, 20.0, 0))) == 0
    finally:
        plain.close()


@pytest.mark.parametrize("variant", ["pe", "pe_union"])
def test_rule_on_python_sets_agrees_with_reference(variant, ix, fixture):
    """the host reference of the GPU tests: cores intersected, shades united back by colour, on Python sets over the sets each pair's hits
    carried (tests/emu_shade lists them)"""
    meta, r1, r2 = fixture
    opts = common.parse_variant(meta["variants"][variant])
    res = shades.emu_quant(ix, r1, r2, opts, sets_stride=256)
    assert int(res["n_sets"].max()) < 255
    got, n_multi_shade, memo, rule = {}, 0, {}, shades.ShadeRule(ix.members, ix.colour)
    for i in range(len(r1)):
        row = res["sets"][i]
        if not row[0]:
            continue
        ids = [int(x) for x in row[1:1 + int(res["n_sets"][i])]]
        if opts["union"]:
            sets = [(e & shades.EC_ID_MASK, bool(e & shades.EC_MATE1), bool(e & shades.EC_MATE2)) for e in ids]
        else:
            sets = ids
        key = tuple(ids)
        if key not in memo:   # (pairs of one place carry the same sets)
            e = rule(sets, union=bool(opts["union"]))
            memo[key] = (e, sum(ix.colour[t] != shades.NOT_A_SHADE for t in e) > 1)
        e, multi = memo[key]
        if e:
            got[e] = got.get(e, 0) + 1
            n_multi_shade += multi
    assert got == shades.load_expected(variant)["ecs"]
    assert n_multi_shade > 0
