"""kg_iqd.h, the IQ display extension (extensions/IQ_display/iq_display.cpp with rx/kiwi/pll.h) as kg_iqd's kernel and host schedule
run it, compiled for the host with g++ -O2 -ffp-contract=off (the reference's flags) in the driver tools/iqd_host_driver.cpp, against
tests/golden/iqd_ref.npz (made by tools/make_ref_iqd_golden.py from the reference's own statements): per script every row, which
blocks sent the text message and its four numbers, and the end state bit for bit.  Then the conditions the golden file must meet so
that the parity tests cannot pass vacuously, every refusal with its neighbours, and the prototypes."""
import os
import re

import numpy as np
import pytest

from . import iqd_common as ic

ROOT = ic.ROOT
IQD_SYMBOLS = {
    "kg_iqd_create": ("int kg_iqd_create(kg_ctx *ctx, int nchan, kg_iqd **out);", 3),
    "kg_iqd_destroy": ("void kg_iqd_destroy(kg_iqd *q);", 1),
    "kg_iqd_init": ("int kg_iqd_init(kg_iqd *q, int ch);", 2),
    "kg_iqd_set_run": ("int kg_iqd_set_run(kg_iqd *q, int ch, int run, double rate);", 4),
    "kg_iqd_set_gain": ("int kg_iqd_set_gain(kg_iqd *q, int ch, int gain);", 3),
    "kg_iqd_set_points": ("int kg_iqd_set_points(kg_iqd *q, int ch, int points);", 3),
    "kg_iqd_set_pll_mode": ("int kg_iqd_set_pll_mode(kg_iqd *q, int ch, int pll_mode, int arg);", 4),
    "kg_iqd_set_pll_bandwidth": ("int kg_iqd_set_pll_bandwidth(kg_iqd *q, int ch, float bandwidth);", 3),
    "kg_iqd_set_draw": ("int kg_iqd_set_draw(kg_iqd *q, int ch, int draw);", 3),
    "kg_iqd_set_display_mode": ("int kg_iqd_set_display_mode(kg_iqd *q, int ch, int display_mode);", 3),
    "kg_iqd_clear": ("int kg_iqd_clear(kg_iqd *q, int ch);", 2),
    "kg_iqd_process_dev": ("int kg_iqd_process_dev(kg_iqd *q, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, int ns, const float *d_iq, size_t iq_stride,", 15),
    "kg_iqd_process": ("int kg_iqd_process(kg_iqd *q, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, int ns, const float *iq, size_t iq_stride,", 15),
    "kg_iqd_state": ("int kg_iqd_state(kg_iqd *q, int ch, kg_iqd_info *info, float *iq, uint8_t *plot, uint8_t *map);", 6),
    "kg_iqd_math_dev": ("int kg_iqd_math_dev(kg_ctx *ctx, int fn, const float *d_a, const float *d_b, size_t n, float *d_out);", 6),
}


@pytest.fixture(scope="module")
def golden():
    return ic.load()


@pytest.fixture(scope="module")
def pool():
    return ic.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return ic.build_driver(tmp_path_factory.mktemp("iqd"))


def test_pool_and_scripts_rebuild(golden, pool):
    """the seeded samples and the scripts are the ones the reference binary was fed; amplitudes stay at or below 3e4"""
    assert ic.digest(pool.tobytes()) == bytes(golden["pool_sha"])
    assert pool.size == ic.POOL and np.abs(pool).max() <= 3e4 and np.isfinite(pool.view(np.float32)).all()
    sc = ic.scripts()
    assert sorted(sc) == [str(n) for n in golden["script_names"]]
    for k, lines in sc.items():
        assert lines == [str(l) for l in golden["s_%s_script" % k]], k


@pytest.mark.parametrize("name", sorted(ic.scripts()))
def test_host_model_equals_the_reference(golden, pool, driver, tmp_path, name):
    got = ic.run_script_exe(driver, ic.scripts()[name], pool, tmp_path)
    ic.check_against_golden(golden, name, got)


def test_golden_file_meets_its_conditions(golden, pool):
    """conditions, not measurements: without them the parity tests could pass on a file that never leaves the easy path"""
    from flydog_sdr_gps_amd.iqd import status_dtype
    g, sc = golden, ic.scripts()
    assert len(sc) >= 12
    varied = npll = 0
    for name in sc:
        k = "s_%s_" % name
        assert g[k + "nrows"].sum() >= 1 and g[k + "sent"].sum() >= 1, name                   # a row and a sent status in every script
        edge, total = (int(v) for v in g[k + "edge_bytes"])
        assert total == int(g[k + "len"].sum())
        varied += 2 * edge < total
        offset = ic.pll_offset(g[k + "ints"])                                                  # every script that ends with a PLL on
        if offset is not None:                                                                 # the reference's PLL found the carrier
            df = g[k + "status"].view(status_dtype)["df"]
            assert abs(float(df[-1]) - offset) < 1.0, (name, df)
            npll += 1
    assert 2 * varied >= len(sc) and npll >= 9
    # MSK: not one quiet message -- the loops have settled, every one of the last 30 is within 1 Hz
    df = g["s_msk_status"].view(status_dtype)["df"]
    assert df.size >= 2 * ic.MSK_SETTLED and (np.abs(df[-ic.MSK_SETTLED:] - ic.MSK_OFFSET_HZ) < 1.0).all() and abs(float(df[0]) - ic.MSK_OFFSET_HZ) > 1.0
    ints = lambda name: g["s_%s_ints" % name]
    # what the scripts cover: PLL off, exponents 1 / 2 / 4 / 8 and another one, MSK at 200 baud, both display modes
    assert ints("pll_off")[2] == 0 and [int(ints(n)[2]) for n in ("exp1_cw", "exp2_bpsk_density", "exp4_qpsk", "exp8_psk8_carrier", "exp3_and_mode3")] == [1, 2, 4, 8, 3]
    assert ints("msk")[3] == 1 and ints("msk")[4] == 200 and ints("msk")[2] == 2 and ints("exp8_psk8_carrier")[6] == 1 and ints("exp4_qpsk")[6] == 0
    # auto gain and fixed gains
    assert g["s_msk_floats"][0] == 0 and g["s_exp1_cw_floats"][0] == np.float32(10.0 ** 0.2) and g["s_exp8_psk8_carrier_floats"][0] > 1e4
    # leading silence under auto gain: 0 * inf is NaN and std::min(255.0f, NaN) is 255 -- two blocks and a half of 255 in both draw modes
    r = g["s_silence_auto_rows"]
    assert (r[:4 * 1300] == 255).all()                                    # 1300 silent samples: old and new, re and im
    old, new = r[4 * 1300:4 * 1500].reshape(-1, 4)[:, :2], r[4 * 1300:4 * 1500].reshape(-1, 4)[:, 2:]
    assert (old == 127).all() and len(np.unique(new)) > 20               # the scale is finite from the first sample on: a silent old sample is 127
    d = g["s_silence_auto_density_rows"]
    assert (d[:2 * 1300] == 255).all() and len(np.unique(d[2 * 1300:2 * 1500])) > 20
    # points 1, 5, 300, 512, 1024, 16384 in both draw modes
    lens = {name: set(zip(g["s_%s_cmd" % name].tolist(), g["s_%s_len" % name].tolist())) for name in sc}
    assert lens["points_1"] == {(0, 4), (2, 2)} and lens["points_16384"] == {(0, 65536), (2, 32768)}
    assert (0, 20) in lens["ns7"] and (0, 20) in lens["points_change"] and (0, 1200) in lens["silence_auto"] and (2, 600) in lens["silence_auto"]
    assert (2, 1024) in lens["exp2_bpsk_density"] and (0, 4096) in lens["pll_off"] and (0, 4096) in lens["rate_20250"]
    assert lens["density_5_1024"] == {(2, 10), (2, 2048)}                                        # points 5 and 1024 in density mode
    assert lens["both_instances"] == {(0, 2048), (1, 2048), (2, 1024), (3, 1024)}                # both instances, both draw modes
    assert g["s_points_16384_nrows"].tolist().index(1) == 31                                     # 32 blocks for one points-mode row of 16384
    # points lowered below the ring position (a row behind the very next sample), raised mid-lap, draw = 2 (no row, nsamp goes on)
    pc, n = g["s_points_change_len"].tolist(), g["s_points_change_nrows"].tolist()
    assert pc[:2] == [1200, 400] and n[0] == 1 and n[1] == 6 and 2800 in pc and n[5:7] == [0, 0] and ints("points_change")[1] == 170 + 9 * 512 - 3000
    # clear and run=1 mid-stream; blocks while run = 0 are not handed over
    assert g["s_clear_run_mid_nrows"].tolist()[14:16] == [0, 0] and g["s_clear_run_mid_sent"].tolist()[14:16] == [0, 0]
    # ns = 7 and ns = 170
    assert any(l.startswith("B 0 7 ") for l in sc["ns7"]) and any(l.startswith("B 0 170 ") for l in sc["points_1"])
    # another rate: maNsend = fs / 4, maN capped at fs / 2
    assert ints("rate_20250")[8] == 5062 and ints("exp4_qpsk")[7] == 6000 and ints("exp4_qpsk")[8] == 3000
    assert os.path.getsize(os.path.join(ic.GOLD, "iqd_ref.npz")) <= 400 * 1024


REFUSALS = {
    "negative_exponent": (ic.HEAD + ["M 1 -1"], 11),                      # the division of the power is libgcc's: not ported
    "negative_exponent_mode0": (ic.HEAD + ["M 0 -8"], 11),
    "points_0": (ic.HEAD + ["P 0"], 12),                                  # the reference would send a zero length and never leave the ring
    "points_negative": (ic.HEAD + ["P -5"], 12),
    "points_16385": (ic.HEAD + ["P 16385"], 12),                          # past the arrays
    "rate_0": (["N", "R 1 0"], 13),
    "rate_nan": (["N", "R 1 nan"], 13),
    "block_before_init": (["B 0 512 0"], 14),
    "command_before_init": (["G 50"], 14),
    "block_before_rate": (["N", "G 50", "B 0 512 0"], 14),
}
ACCEPTED = {
    "exponent_0": ic.HEAD + ["M 1 0"] + ic._B("cw", 0, 2),               # PLL off
    "exponent_5": ic.HEAD + ["M 0 5"] + ic._B("cw", 0, 2),
    "msk_negative_baud": ic.HEAD + ["M 2 -50"] + ic._B("msk", 0, 2),
    "mode_9_negative_arg": ic.HEAD + ["M 9 -3"] + ic._B("cw", 0, 2),      # only re-initialises
    "points_1": ic.HEAD + ["P 1"] + ic._B("cw", 0, 1, ns=7),
    "points_16384": ic.HEAD + ["P 16384"] + ic._B("cw", 0, 2),
    "draw_7": ic.HEAD + ["D 7"] + ic._B("cw", 0, 2),
    "rate_1": ["N", "R 1 1"] + ic._B("cw", 0, 2),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(pool, driver, tmp_path, name):
    lines, status = REFUSALS[name]
    ic.run_script_exe(driver, lines, pool, tmp_path, expect=status)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_neighbours_of_the_refusals_are_taken(pool, driver, tmp_path, name):
    got = ic.run_script_exe(driver, ACCEPTED[name], pool, tmp_path)
    want = {"points_1": [7], "points_16384": [0, 0], "draw_7": [0, 0]}.get(name, [0, 1])
    assert got["nrows"].tolist() == want, (name, got["nrows"])
    assert np.isfinite(got["floats"]).all() and np.isfinite(got["pll"]).all()


def test_iqd_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib, iqd
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s, (proto, nargs) in IQD_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert hasattr(lib, s), s
    # every device pointer of the new prototypes is typed
    protos = re.findall(r"\b(kg_iqd\w*)\s*\(([^;{}()]*)\)\s*;", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert len(protos) == len(IQD_SYMBOLS) and not [n for n, a in protos if re.search(r"\bvoid\s*\*", a)]
    # the receiver bank's thirteen
    bank = dict(re.findall(r"\b(kg_rxbank_iqd\w*)\s*\(([^;{}()]*)\)\s*;", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    assert sorted(bank) == sorted("kg_rxbank_iqd" + s for s in ("_init", "_set_run", "_set_gain", "_set_points", "_set_pll_mode", "_set_pll_bandwidth",
                                                                 "_set_draw", "_set_display_mode", "_clear", "", "_map", "_rows", "_status"))
    for s, args in bank.items():
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == len(args.split(",")) and hasattr(lib, s) and not re.search(r"\bvoid\s*\*", args), s
    h = {k: int(v) for k, v in re.findall(r"\bKG_IQD_([A-Z_]+)\s*=\s*(-?\d+)", header)}
    assert (h["POINTS"], h["DENSITY"], h["MATH_HYPOTF"], h["MATH_FMODF"]) == (iqd.POINTS, iqd.DENSITY, iqd.HYPOTF, iqd.FMODF) == (0, 1, 0, 1)
    d = {k: int(v) for k, v in re.findall(r"#define KG_IQD_(\w+)\s+(\d+)", header)}
    assert (d["RING"], d["MAX_NS"]) == (ic.RING, ic.MAX_NS) == (iqd.RING, iqd.MAX_NS)
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_iqd.h")).read()
    for lit in ("RING = 16384, NCH = 2, MAX_NS = 512", "POINTS = 0, DENSITY = 1"):
        assert lit in src, lit
    sizes = {"kg_iqd_status": iqd.status_dtype.itemsize, "kg_iqd_row": iqd.row_dtype.itemsize, "kg_iqd_info": iqd.info_dtype.itemsize}
    assert sizes == {"kg_iqd_status": 24, "kg_iqd_row": 32, "kg_iqd_info": 164}


# ---- seeded random scripts (tests/ext_random.py): the combinations of commands and blocks nobody wrote down
@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er
    return er.load("iqd")


def test_random_scripts_host_model_equals_the_fixture(random_ref, pool, driver, tmp_path):
    """every seed's script is the one the reference was fed, the host model takes it (exit status 0) and equals the reference in every
    field the fixture keeps: rows per block, cmd, len, sent, the end state's scalars, and the digests of the row stream, the status
    records, _iq, _plot and _map"""
    from . import ext_random as er
    for seed in range(er.NSEED):
        lines = er.iqd_script(seed)
        er.check_record("iqd", seed, lines, ic.run_script_exe(driver, lines, pool, tmp_path), er.unpack(random_ref, seed))


def test_random_fixture_meets_its_conditions(random_ref):
    """conditions, not measurements: what the 40 seeds must reach between them (ext_random.IQD_CONDITIONS, 5000 rows), computed from the
    fixture and the regenerated scripts; none of the 40 was refused by the reference"""
    from . import ext_random as er
    er.check_conditions("iqd", random_ref)
    assert os.path.getsize(er.fixture_path("iqd")) <= 64 * 1024


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "device_resident"])
def test_random_side_by_side_plans_share_their_calls(resident):
    """the calls tests/test_iqd_gpu.py makes with the seeds three at a time on one object are decided ahead of the run
    (ext_random_dev.plan_side_by_side): over all the groups at least half of them carry more than one channel"""
    from . import ext_random_dev as ed
    every, both = ed.shared_in_all("iqd", resident)
    assert 2 * both >= every, (both, every)
