"""kg_fax.h, the FAX extension's decoder (extensions/FAX/FaxDecoder.cpp) as kg_fax's kernel runs it, compiled for the host with g++ -O2
-ffp-contract=off (the reference's flags) in the driver tools/fax_host_driver.cpp, against tests/golden/fax_ref.npz (made by
tools/make_ref_fax_golden.py from the reference's own statements): per script the lines every block completed, every line's record,
every row byte and the end state -- every scalar and array -- bit for bit.  Then the conditions the golden file must meet so that the
parity tests cannot pass vacuously, every refusal with its neighbours, and the prototypes.  Every comparison is an equality."""
import os
import re
import subprocess

import numpy as np
import pytest

from . import fax_common as fc

ROOT = fc.ROOT
FAX_SYMBOLS = {
    "kg_fax_create": ("int kg_fax_create(kg_ctx *ctx, int nconn, kg_fax **out);", 3),
    "kg_fax_destroy": ("void kg_fax_destroy(kg_fax *q);", 1),
    "kg_fax_start": ("int kg_fax_start(kg_fax *q, int conn, int lpm, int imagewidth, int carrier, int deviation, int bandwidth, int include_headers, int phasing, "
                     "int autostop, int debug,", 13),
    "kg_fax_set_shift": ("int kg_fax_set_shift(kg_fax *q, int conn, float shift);", 3),
    "kg_fax_stop": ("int kg_fax_stop(kg_fax *q, int conn);", 2),
    "kg_fax_max_lines": ("int kg_fax_max_lines(kg_fax *q, const int32_t *conns, int nconn, const int32_t *nblk, int32_t *max_lines, int32_t *max_width);", 6),
    "kg_fax_push": ("int kg_fax_push(kg_fax *q, const int32_t *conns, int nconn, const int32_t *nblk, const int16_t *s16, size_t stride, const double *srate, "
                    "uint8_t *rows,", 12),
    "kg_fax_state": ("int kg_fax_state(kg_fax *q, int conn, kg_fax_info *info, int16_t *samples, uint8_t *demod, uint8_t *prev, uint8_t *out);", 7),
}
BANK = ("_start", "_set_shift", "_stop", "", "_out")


@pytest.fixture(scope="module")
def golden():
    return fc.load()


@pytest.fixture(scope="module")
def pool():
    return fc.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return fc.build_driver(tmp_path_factory.mktemp("fax"))


def test_pool_and_scripts_rebuild(golden, pool):
    """the seeded audio and the scripts are the ones the reference binary was fed"""
    assert fc.digest(pool.tobytes()) == bytes(golden["pool_sha"])
    assert pool.size == fc.POOL and (pool[fc.AT["zeros"]:] == 0).all() and np.abs(pool.astype(np.int32)).max() <= 12000
    sc = fc.scripts()
    assert sorted(sc) == [str(n) for n in golden["script_names"]]
    for k, lines in sc.items():
        assert fc.digest("\n".join(lines).encode()) == bytes(golden["s_%s_script_sha" % k]), k
        assert sum(int(n) for n in golden["s_%s_nlines" % k]) < 256, k        # under the reference's first image allocation


@pytest.mark.parametrize("name", sorted(fc.scripts()))
def test_host_model_equals_the_reference(golden, pool, driver, tmp_path, name):
    got = fc.run_script_exe(driver, fc.scripts()[name], pool, tmp_path)
    fc.check_against_golden(golden, name, got)


def _recs(g, name):
    return np.frombuffer(np.ascontiguousarray(g["s_%s_recs" % name]).tobytes(), fc.rec_dtype)


def _info(g, name):
    return np.frombuffer(g["s_%s_info" % name].tobytes(), fc.info_dtype)[0]


def _rows_of(g, name):
    w = [fc.rows_width(fc.scripts()[name], b) for b in np.repeat(np.arange(g["s_%s_nlines" % name].size), g["s_%s_nlines" % name])]
    r = _recs(g, name)
    out, at = [], 0
    for k in range(r.size):
        if r["flags"][k] & fc.F_ROW_SENT:
            out.append(g["s_%s_rows" % name][at:at + 1 + w[k]])
            at += 1 + w[k]
    assert at == g["s_%s_rows" % name].size
    return out


def golden_conditions(g, size):
    """conditions on the reference's output alone, not measurements: without them the parity tests could pass on a file that never
    leaves the easy path"""
    sc = fc.scripts()
    assert size <= 1024 * 1024
    assert len(sc) >= 12
    types, flags, lpms, widths, ratios = set(), 0, set(), set(), set()
    for name in sc:
        r, st = _recs(g, name), _info(g, name)
        assert int(g["s_%s_nlines" % name].sum()) == r.size >= 1, name
        types |= set(r["type"].tolist())
        flags |= int(np.bitwise_or.reduce(r["flags"]))
        lpms.add(int(st["lpm"]))
        widths.add(int(st["imagewidth"]))
        ratios.add(float(st["ratio"]))
        for row in _rows_of(g, name):
            assert row[0] == 254, name
    assert types == {fc.IMAGE, fc.START, fc.STOP}                                  # every line type
    assert flags == 127                                                           # both autostop messages, phased, rejected, sps_changed, median, a row
    assert {60, 90, 120, 240} <= lpms and len(widths) >= 3 and 1024 in widths
    assert min(ratios) < 1.0 < max(ratios) and 1.0 in ratios                      # a rate ratio on either side of 1
    # the reference's own story at 120 lpm: START counted to 6, phased with a non-zero skip, autostopped, started again
    r = _recs(g, "nominal_120")
    first = int(np.flatnonzero((r["type"] == fc.START) & (r["typecount"] == 6))[0])
    ph = np.flatnonzero(r["flags"] & fc.F_PHASED)
    med = r[(r["flags"] & fc.F_MEDIAN) != 0]
    assert first < 20 and ph.size == 1 and r["skip"][ph[0]] != 0 and med.size >= 1 and not (med["flags"][0] & fc.F_PHASING_REJECTED)
    assert med["ninety_pct"][0] - med["ten_pct"][0] <= 6000 // 6 and (r["phasing_pos"] >= 0).sum() >= 38
    a1, a0 = np.flatnonzero(r["flags"] & fc.F_AUTOSTOPPED_1), np.flatnonzero(r["flags"] & fc.F_AUTOSTOPPED_0)
    assert a1.size >= 1 and a0.size >= 1 and a1[0] < a0[0]
    quiet = r[a1[0] + 1:a0[0]]
    assert quiet.size >= 3 and not (quiet["flags"] & fc.F_ROW_SENT).any() and (np.diff(quiet["imageline"]) == 1).all()      # counted, not decoded
    assert (r[a0[0] + 1:]["flags"] & fc.F_ROW_SENT).any()
    # the skip moved the line boundaries: behind the phasing the lines complete at other offsets than before it
    # the opposite polarity is rejected by the spread test
    rr = _recs(g, "reverse_rejected")
    bad = rr[(rr["flags"] & fc.F_PHASING_REJECTED) != 0]
    assert bad.size >= 1 and (bad["ninety_pct"] - bad["ten_pct"] > 1000).all() and not (rr["flags"] & fc.F_PHASED).any()
    # 90 lpm: the count never holds; 240 lpm without headers: rows only behind the phasing
    r90 = _recs(g, "lpm90_w1900")
    assert (r90["type"] != fc.IMAGE).sum() >= 8 and not (r90["flags"] & (fc.F_AUTOSTOPPED_1 | fc.F_MEDIAN)).any() and (r90["flags"][1:] & fc.F_ROW_SENT).all()
    r240 = _recs(g, "lpm240_hdr0")
    p = int(np.flatnonzero(r240["flags"] & fc.F_PHASED)[0])
    assert not (r240["flags"][:p - 2] & fc.F_ROW_SENT).any() and (r240["flags"][p:] & fc.F_ROW_SENT).any() and _info(g, "lpm240_hdr0")["spl"] == 3000
    assert _info(g, "lpm60_20250")["spl"] == 20250 and (_recs(g, "lpm60_20250")["flags"] & fc.F_MEDIAN).any()
    # a NaN pixel: the end state of all-zero audio holds it, and its rows are zeros; silence then signal recovers
    z = _info(g, "all_zero")
    assert np.isnan(z["Iprev"]) and np.isnan(z["Qprev"]) and all((row[1:] == 0).all() for row in _rows_of(g, "all_zero")) and len(_rows_of(g, "all_zero")) >= 2
    s = _rows_of(g, "silence_then_signal")
    assert (s[0][1:] == 0).all() and (s[-1][1:] != 0).any() and np.isfinite(_info(g, "silence_then_signal")["Iprev"])
    # a debug row and a blended row: debug sends the pixel averages (m_outImage stays zero), the others a blend that differs from them
    assert (g["s_p0a0_debug_out"] == 0).all() and (_recs(g, "p0a0_debug")["flags"] & fc.F_ROW_SENT).all() and _info(g, "p0a0_debug")["skip_header_detection"] == 1
    assert (g["s_nominal_120_out"] != 0).any() and (g["s_nominal_120_out"] != g["s_nominal_120_prev"]).any()
    # the zero previous line behind the counted lines: the first row behind fax_autostopped=0 is the pixel averages scaled down
    rp = _recs(g, "p0a1_120")
    assert (rp["flags"] & fc.F_AUTOSTOPPED_1).any() and (rp["flags"] & fc.F_AUTOSTOPPED_0).any()
    # shifts and the restart
    sh = _recs(g, "shift_mid")
    assert int(0.37 * 6000) in sh["skip"].tolist() or np.diff(sh["off"]).any()
    one = _recs(g, "one_short_240")
    assert g["s_one_short_240_nlines"][:6].sum() == 0 and g["s_one_short_240_nlines"][6] == 1 and one["off"][0] == 1      # 73 + 3000 == 6 * 512 + 1
    # m_SamplesPerSec_frac_prev is carried over a restart: the first line behind the second start (12000.5 -> 12000) says fax_sps_changed,
    # the first behind the third (12000 -> 12000) does not, although Configure ran
    rs, at = _recs(g, "restart_mid_line"), np.concatenate([[0], np.cumsum(g["s_restart_mid_line_nlines"])])
    assert (rs["flags"][at[43]] & fc.F_SPS_CHANGED) and not (rs["flags"][at[107]] & fc.F_SPS_CHANGED) and g["s_restart_mid_line_nlines"][103:107].sum() == 0
    assert _info(g, "restart_mid_line")["lpm"] == 120 and at[107] > at[43] > 0 and at[-1] > at[107]


def test_golden_file_meets_its_conditions(golden):
    golden_conditions(golden, os.path.getsize(os.path.join(fc.GOLD, "fax_ref.npz")))


HEAD = fc._C(120)
REFUSALS = {
    "lpm_0": ([fc._C(0)], 21),
    "lpm_negative": ([fc._C(-120)], 21),
    "deviation_0": ([fc._C(120, dev=0)], 22),
    "bandwidth_3": ([fc._C(120, bw=3)], 23),
    "bandwidth_negative": ([fc._C(120, bw=-1)], 23),
    "width_0": ([fc._C(120, w=0)], 24),
    "spl_below_width": ([fc._C(120, w=6001)], 25),
    "spl_above_bound": ([fc._C(29, nom=12000)], 26),                      # 24827 samples a line
    "rate_0": ([fc._C(120, nom=0)], 27),
    "srate_low": ([fc._C(120, srate=5999.0)], 27),
    "srate_nan": ([fc._C(120, srate=float("nan"))], 27),
    "rate_mid_stream": ([HEAD, "R 24001.0"], 27),
    "shift_negative": ([HEAD, "H -0.25"], 28),
    "shift_above_1": ([HEAD, "H 1.5"], 28),
    "shift_nan": ([HEAD, "H nan"], 28),
    "shift_inf": ([HEAD, "H inf"], 28),
    "block_before_start": (["B 0"], 5),
}
ACCEPTED = {
    "lpm_1_at_400": [fc._C(1, w=24000, nom=400, srate=400.0)],            # 24000 samples a line
    "spl_at_bound": [fc._C(60, nom=24576, srate=24576.0)],
    "spl_equals_width": [fc._C(120, w=6000)],
    "60_lpm_at_20250": [fc._C(60, nom=20250, srate=20250.0)],
    "deviation_negative": [fc._C(120, dev=-400)],
    "srate_half": [fc._C(120, srate=6000.0)],
    "srate_twice": [fc._C(120, srate=24000.0)],
    "shift_0_and_1": [HEAD, "H 0.0", "H 1.0"],
    "width_1": [fc._C(120, w=1)],
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(pool, driver, tmp_path, name):
    lines, status = REFUSALS[name]
    fc.run_script_exe(driver, lines, pool, tmp_path, expect=status)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_neighbours_of_the_refusals_are_taken(pool, driver, tmp_path, name):
    lines = ACCEPTED[name] + fc._B("a120", 0, 30)
    got = fc.run_script_exe(driver, lines, pool, tmp_path)
    spl = int(got["info"]["spl"])
    assert spl == int(float(lines[0].split()[10]) * 60.0 / int(lines[0].split()[1])) and got["info"]["started"] == 1
    assert got["recs"].size >= (1 if 30 * 512 >= 2 * spl else 0)


def test_a_refusal_changes_nothing(pool, driver, tmp_path):
    """refused commands strewn through a script (the driver passes over them with -k) leave every record, every row and the end state as
    they are without them"""
    bad = [fc._C(0), fc._C(120, dev=0), fc._C(120, bw=3), fc._C(120, w=0), fc._C(120, w=6001), fc._C(20), "H -1.0", "H 2.0", "H nan", "R 100.0", "R inf"]
    base = [HEAD] + fc._B("a120", 0, 40) + ["H 0.25"] + fc._B("a120", 40, 20) + ["R 12000.4"] + fc._B("a120", 60, 40)
    mixed = []
    for i, l in enumerate(base):
        mixed += [l] + ([bad[i % len(bad)]] if i % 7 == 0 else [])
    want = fc.run_script_exe(driver, base, pool, tmp_path)
    raw = open(tmp_path / "out.bin", "rb").read()
    fc.run_script_exe(driver, mixed, pool, tmp_path, keep_on=True)
    assert open(tmp_path / "out.bin", "rb").read() == raw and want["recs"].size >= 7 and len(want["rows"]) >= 3
    for l in bad:                                                         # and each of them IS refused
        r = subprocess.run([driver, "/dev/stdin", str(tmp_path / "pool.bin"), str(tmp_path / "o2.bin")], input="\n".join([HEAD, l]) + "\n", text=True)
        assert 21 <= r.returncode <= 28, (l, r.returncode)


def test_lines_bound_holds_for_every_script(golden):
    """kg_fax_max_lines' bound, lines <= (nblk * 1026 + spl - 1) / spl + 1, against what the reference completed in every window of 1, 7 and
    64 blocks of every script"""
    for name, lines in fc.scripts().items():
        nl = golden["s_%s_nlines" % name].astype(np.int64)
        spl = min(int(float(l.split()[10]) * 60.0 / int(l.split()[1])) for l in lines if l[0] == "C")
        c = np.concatenate([[0], np.cumsum(nl)])
        for k in (1, 7, 64):
            if nl.size >= k:
                assert (c[k:] - c[:-k]).max() <= (k * 1026 + spl - 1) // spl + 1, (name, k)


def test_fax_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib, fax
    import flydog_sdr_gps_amd
    assert flydog_sdr_gps_amd.FaxDecoder is fax.FaxDecoder
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lib = _lib.load_library()
    for s, (proto, nargs) in FAX_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert hasattr(lib, s), s
    protos = re.findall(r"\b(kg_fax\w*)\s*\(([^;{}()]*)\)\s*;", bare)
    assert sorted(n for n, _ in protos) == sorted(FAX_SYMBOLS) and not [n for n, a in protos if re.search(r"\bvoid\s*\*", a)]
    for n, a in protos:
        assert len(a.split(",")) == FAX_SYMBOLS[n][1], n
    # every prototype cites the reference lines it replaces
    for s in FAX_SYMBOLS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|void)\s*%s\(" % s, header, flags=re.S)
        assert m and re.search(r":\d+", m.group(1)), (s, "no reference lines in the comment above the prototype")
    bank = dict(re.findall(r"\b(kg_rxbank_fax\w*)\s*\(([^;{}()]*)\)\s*;", bare))
    assert sorted(bank) == sorted("kg_rxbank_fax" + s for s in BANK)
    for s, args in bank.items():
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == len(args.split(",")) and hasattr(lib, s) and not re.search(r"\bvoid\s*\*", args), s
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|kg_fax \*)\s*\*?%s\(" % s, header, flags=re.S)
        assert m and re.search(r":\d+", m.group(1)), (s, "no reference lines in the comment above the prototype")
    h = {k: int(v) for k, v in re.findall(r"\bKG_FAX_([A-Z_0-9]+)\s*=\s*(-?\d+)", header)}
    assert (h["IMAGE"], h["START"], h["STOP"]) == (fax.IMAGE, fax.START, fax.STOP) == (fc.IMAGE, fc.START, fc.STOP)
    assert (h["SPS_CHANGED"], h["AUTOSTOPPED_0"], h["AUTOSTOPPED_1"], h["PHASED"], h["ROW_SENT"], h["PHASING_REJECTED"], h["MEDIAN"]) == (1, 2, 4, 8, 16, 32, 64) \
        == (fax.SPS_CHANGED, fax.AUTOSTOPPED_0, fax.AUTOSTOPPED_1, fax.PHASED, fax.ROW_SENT, fax.PHASING_REJECTED, fax.MEDIAN)
    d = {k: int(v) for k, v in re.findall(r"#define KG_FAX_(\w+)\s+(\d+)", header)}
    assert (d["MAX_SPL"], d["BLK"], d["MSG_DRAW"]) == (fc.MAX_SPL, fc.BLK, 254) == (fax.MAX_SPL, fax.BLK, fax.MSG_DRAW)
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_fax.h")).read()
    assert "DET_CAP = 3000, MAX_SPL = 24576, MSG_DRAW = 254" in src
    assert (fax.rec_dtype, fax.info_dtype) == (fc.rec_dtype, fc.info_dtype)


# ---- seeded random scripts and shape scripts (tests/ext_random.py): what the hand-written scripts leave out
@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er
    return er.load("fax")


def test_random_scripts_host_model_equals_the_fixture(random_ref, pool, driver, tmp_path):
    """every seed's script and every shape script is the one the reference was fed, the host model takes it (exit status 0) and equals
    the reference in every field the fixture keeps: the lines of every block, every line's type, flags and pick, and the digests of the other record fields, the rows and the end state"""
    from . import ext_random as er
    scripts = [er.fax_script(seed) for seed in range(er.NSEED)] + list(er.fax_shapes().values())
    assert int(random_ref["n_script_sha"].size) == len(scripts)
    for k, lines in enumerate(scripts):
        assert fc.nblocks(lines) <= er.MOST_BLOCKS
        er.check_record("fax", k, lines, fc.run_script_exe(driver, lines, pool, tmp_path), er.unpack(random_ref, k))


def test_random_fixture_meets_its_conditions(random_ref):
    """conditions, not measurements: what the 40 seeds must reach between them (ext_random.FAX_CONDITIONS), computed from the fixture
    and the regenerated scripts; none of the 40 was refused by the reference.  The shape scripts count towards none"""
    from . import ext_random as er
    er.check_conditions("fax", random_ref)
    assert os.path.getsize(er.fixture_path("fax")) <= 64 * 1024


def test_random_pushes_reach_every_size():
    """the pushes tests/test_fax_gpu.py makes with the seeds under their partitions and with the shape scripts are decided ahead of
    any run: one holds 256 blocks (the most a push takes), one 45 to 255, one a single block"""
    from . import ext_random_dev as ed
    n = ed.planned_pushes("fax")
    assert max(n) == 256 and any(45 <= k <= 255 for k in n) and 1 in n and min(n) >= 1


def test_random_side_by_side_pushes_are_shared():
    """the pushes tests/test_fax_gpu.py makes with the seeds three at a time on one object are decided ahead of the run
    (fax_common.run_side_by_side): over all the groups at least half of them carry more than one connection"""
    from . import ext_random_dev as ed
    every, both = ed.shared_in_all("fax")
    assert 2 * both >= every, (both, every)
