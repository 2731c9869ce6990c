"""kg_fftext.h, the FFT extension (extensions/FFT/FFT.cpp: fft_msgs and fft_data) as kg_fftext's kernel and host schedule run it,
compiled for the host with g++ -O2 -ffp-contract=off (the reference's flags) in the driver tools/fftext_host_driver.cpp, against the two
pins of tests/golden/fftext_ref.npz (made by tools/make_ref_fftext_golden.py from the reference's own statements): per script every
block's fate, bin and row, and the final state -- both scales, bins, fi, fft_sec, ncma and all 200 x 1024 sums bit for bit -- and the
100 ms limiter call by call.  Then the conditions the golden file must meet so that the parity tests cannot pass vacuously, every
refusal, and the prototypes."""
import os
import re

import numpy as np
import pytest

from . import fftext_common as fc

ROOT = fc.ROOT
FFTEXT_SYMBOLS = {
    "kg_fftext_create": ("int kg_fftext_create(kg_ctx *ctx, int nchan, kg_fftext **out);", 3),
    "kg_fftext_destroy": ("void kg_fftext_destroy(kg_fftext *fx);", 1),
    "kg_fftext_set_rate": ("int kg_fftext_set_rate(kg_fftext *fx, double sample_rate);", 2),
    "kg_fftext_set_run": ("int kg_fftext_set_run(kg_fftext *fx, int ch, int run, int is_sam, int is_qam);", 5),
    "kg_fftext_set_itime": ("int kg_fftext_set_itime(kg_fftext *fx, int ch, double itime);", 3),
    "kg_fftext_clear": ("int kg_fftext_clear(kg_fftext *fx, int ch);", 2),
    "kg_fftext_restart": ("int kg_fftext_restart(kg_fftext *fx, int ch);", 2),
    "kg_fftext_process_dev": ("int kg_fftext_process_dev(kg_fftext *fx, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const float *d_spec,", 14),
    "kg_fftext_process": ("int kg_fftext_process(kg_fftext *fx, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const float *spec,", 14),
    "kg_fftext_due": ("int kg_fftext_due(kg_fftext *fx, int ch, uint32_t now_ms);", 3),
    "kg_fftext_state": ("int kg_fftext_state(kg_fftext *fx, int ch, kg_fftext_info *info, float *pwr, int32_t *ncma);", 5),
    "kg_rxbank_fftext_set_rate": ("int kg_rxbank_fftext_set_rate(kg_rxbank *bank, double sample_rate);", 2),
    "kg_rxbank_fftext_set_run": ("int kg_rxbank_fftext_set_run(kg_rxbank *bank, int rx, int run);", 3),
    "kg_rxbank_fftext_set_itime": ("int kg_rxbank_fftext_set_itime(kg_rxbank *bank, int rx, double itime);", 3),
    "kg_rxbank_fftext_clear": ("int kg_rxbank_fftext_clear(kg_rxbank *bank, int rx);", 2),
    "kg_rxbank_fftext": ("kg_fftext *kg_rxbank_fftext(kg_rxbank *bank);", 1),
    "kg_rxbank_fftext_max": ("int kg_rxbank_fftext_max(kg_rxbank *bank);", 1),
    "kg_rxbank_fftext_map": ("int kg_rxbank_fftext_map(kg_rxbank *bank, int32_t *rx_of_row, int32_t *blk_of_row, int32_t *bin_of_row);", 4),
    "kg_rxbank_fftext_rows": ("int kg_rxbank_fftext_rows(kg_rxbank *bank, uint8_t **d_rows, size_t *row_stride);", 3),
}


@pytest.fixture(scope="module")
def golden():
    return fc.load()


@pytest.fixture(scope="module")
def pool():
    return fc.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return fc.build_driver(tmp_path_factory.mktemp("fftext"))


def test_pool_and_scripts_rebuild(golden, pool):
    """the seeded spectra and the scripts are the ones the reference binary was fed, and no spectrum holds a NaN"""
    names, spec = pool
    assert names == [str(n) for n in golden["pool_names"]] and len(names) == fc.NPOOL
    assert fc.digest(spec.tobytes()) == bytes(golden["pool_sha"])
    sc = fc.scripts()
    assert sorted(sc) == [str(n) for n in golden["script_names"]]
    for k, lines in sc.items():
        assert lines == [str(l) for l in golden["s_%s_script" % k]], k
    lim = fc.limiter_scripts()
    assert sorted(lim) == [str(n) for n in golden["limiter_names"]]
    for k, clocks in lim.items():
        assert np.array_equal(np.array(clocks, np.uint32), golden["limiter_%s_clock" % k]), k


@pytest.mark.parametrize("name", sorted(fc.scripts()))
def test_host_model_equals_the_reference(golden, pool, driver, tmp_path, name):
    """Pin 1: rows, bins, which blocks were taken, ncma, sums, fi, fft_sec, bins, scales"""
    got = fc.run_script_exe(driver, fc.scripts()[name], pool[1], tmp_path)
    fc.check_against_golden(golden, name, got)


def test_limiter_equals_the_reference(golden, driver, tmp_path):
    """Pin 2: kg_fftext_cf::due call by call (kg_fftext_due through the C ABI: tests/test_fftext_gpu.py, the object needs a device)"""
    g = golden
    for k, clocks in fc.limiter_scripts().items():
        sent, last = fc.run_limiter_exe(driver, clocks, tmp_path)
        assert np.array_equal(sent, g["limiter_%s_sent" % k]), (k, sent, g["limiter_%s_sent" % k])
        assert np.array_equal(last, g["limiter_%s_last" % k]), k
    assert g["limiter_first_at_100_sent"][0] == 0 and g["limiter_first_at_100_sent"][1] == 1        # fires only when now > 100
    assert g["limiter_first_below_sent"][:5].sum() == 0
    assert g["limiter_first_above_sent"][0] == 1 and g["limiter_first_above_last"][0] == 101       # last = now the first time ...
    assert g["limiter_first_above_last"][g["limiter_first_above_sent"] == 1][1] == 201             # ... += 100 from then on
    for k in ("cadence_42_67", "cadence_25_28"):                                                    # about ten a second
        span = (int(g["limiter_%s_clock" % k][-1]) - int(g["limiter_%s_clock" % k][0])) / 1000.0
        assert abs(g["limiter_%s_sent" % k].sum() / span - 10.0) < 1.0, k
    # a gap of several periods: += 100 catches up -- every call fires until last_ms is within 100 ms again; it never jumps to now
    f, l, c = g["limiter_long_gap_sent"], g["limiter_long_gap_last"], g["limiter_long_gap_clock"]
    assert f[12:12 + 30].all() and (np.diff(l[12:12 + 30].astype(np.int64)) == 100).all() and int(l[12]) < int(c[12]) - 3000


def test_golden_file_meets_its_conditions(golden, pool):
    """conditions, not measurements: without them the parity tests could pass on a file that never leaves the easy path"""
    g = golden
    names, spec = pool
    ix = {n: i for i, n in enumerate(names)}
    unwrapped = lambda row: row[np.arange(fc.W) ^ 512]                  # byte of column c
    # the three boost cases: scales as FFT.cpp:211 / :225 give them, and each reaches floor and ceiling
    for name, key in (("wf", "1e4"), ("spec", "1e6"), ("spec_sam", "100"), ("spec_qam", "100")):
        assert np.array_equal(g["s_%s_scales" % name].view(np.uint32), np.array([fc.SCALES[key]] * 2, np.float32).view(np.uint32)), name
    assert g["s_integ_bins3_scales"][0] == fc.SCALES["1e4"]
    for name in ("wf", "spec", "spec_sam"):
        rows = g["s_%s_rows" % name]
        assert rows.shape == (fc.NPOOL, fc.W) and rows.min() == 55 and rows.max() == 255, name
    # spec under isSAM listens to the channel-null filter: every passband block ignored, every other one sent
    assert g["s_spec_sam_sent"].tolist() == [0, 1] * fc.NPOOL and g["s_spec_sam_state"][1] == fc.CHAN_NULL
    assert np.array_equal(g["s_spec_qam_row_sha"], g["s_spec_sam_row_sha"])                       # QAM's boost is the same 100
    assert g["s_integ_sam_sent"].tolist() == [1] * 6 + [0] * 2 and g["s_integ_sam_state"][1] == fc.PASSBAND
    # outside integ the power is re * re alone: re = 0 beside a large (or infinite) im gives the floor, +-inf and overflow the ceiling
    u = unwrapped(g["s_wf_rows"][ix["inf_overflow_zero_re"]])
    assert (u[:192] == 255).all() and (u[256:512] == 55).all()
    u = unwrapped(g["s_wf_rows"][ix["zeros_signs_denormals"]])
    assert (u[:256] == 55).all() and (u[512:640] == 55).all() and (u[768:] == 55).all()
    # ... and under integ it is re * re + im * im: the same columns reach the ceiling (integ_pool gives every pool spectrum a fresh bin
    # or one that holds a single earlier block)
    assert g["s_integ_pool_sent"].all() and len(set(g["s_integ_pool_bins"].tolist())) >= 13
    # the edge sets reach both sides of the (int) truncation at every k from -200 to -1 under their own boost
    for name, key in (("wf", "1e4"), ("spec", "1e6"), ("spec_sam", "100")):
        rows = g["s_%s_rows" % name]
        u = np.concatenate([unwrapped(rows[ix["edge_%s_0" % key]]), unwrapped(rows[ix["edge_%s_1" % key]])])[:201 * 9].reshape(201, 9).astype(int)
        assert (u.max(axis=1) - u.min(axis=1) <= 1).all(), name
        assert (u[:200, 0] == np.arange(55, 255)).all() and (u[:200, 8] == np.arange(56, 256)).all() and (u[200] == 255).all(), name
    # bins = 3 over twelve blocks: the bin wraps round, every bin is added to several times, and the rows of one bin differ
    b = g["s_integ_bins3_bins"].tolist()
    assert g["s_integ_bins3_state"][2] == 3 and set(b) == {0, 1, 2} and b[0] == 0 and any(b[i + 1] < b[i] for i in range(11))
    assert g["s_integ_bins3_ncma"][:3].min() >= 3 and g["s_integ_bins3_ncma"].sum() == 12 and g["s_integ_bins3_pwr_head"].shape == (3, fc.W)
    rows = g["s_integ_bins3_rows"]
    first, last = b.index(0), len(b) - 1 - b[::-1].index(0)
    assert (rows[last].astype(int) >= rows[first].astype(int)).all() and (rows[last] > rows[first]).sum() > 500      # sums only grow
    assert g["s_integ_bins3_20250_state"][2] == 3 and g["s_integ_bins3_20250_times"][1] == 1.0 / (20250.0 * 2 / 1024)
    assert g["s_integ_bins3_times"][1] == 1.0 / (12000.0 * 2 / 1024)
    # bins = 0: every block lands in bin 0
    assert g["s_integ_bins0_state"][2] == 0 and not g["s_integ_bins0_bins"].any() and g["s_integ_bins0_ncma"][0] == 6
    # bins = 205: five blocks dropped at bins 200 .. 204 while fi goes on, then the wrap to bin 0
    sent, b = g["s_integ_bins205_sent"], g["s_integ_bins205_bins"]
    assert g["s_integ_bins205_state"][2] == 205 and sent.size == 210 and sent.sum() == 205 and b.max() == 199
    dropped = np.flatnonzero(sent == 0)
    assert dropped.size == 5 and (np.diff(dropped) == 1).all() and sent[dropped[-1] + 1:].all() and b[-1] < 5 and b[dropped[0] - 1] == 199
    assert g["s_integ_bins205_times"][0] > 210 * 0.0426                                         # fi advanced through the dropped blocks
    assert g["s_integ_bins205_ncma"].sum() == 205 and g["s_integ_bins205_ncma"][0] == 3      # blocks 0 and 1, and one behind the wrap
    # clear and itime mid-stream reset the sums: ncma at the end counts the blocks behind the last clear only
    assert g["s_clear_itime_mid_ncma"].sum() == 2 and g["s_clear_itime_mid_state"][2] == 4
    # wf -> integ without a clear: fi, ncma and the stale pwr[0] carry over (ncma counts the integ blocks before and after)
    assert g["s_wf_to_integ_ncma"].sum() == 9 and g["s_wf_to_integ_bins"].tolist()[4:6] == [0, 0] and g["s_wf_to_integ_state"][3] == 0
    assert abs(g["s_wf_to_integ_times"][0] - 9 * fc.FFT_SEC[12000]) < 1e-9
    # the other instance's blocks interleaved: ignored before anything else (fi does not advance)
    assert g["s_interleaved_sent"].tolist() == [1, 0] * 8 and abs(g["s_interleaved_times"][0] - 8 * fc.FFT_SEC[12000]) < 1e-9
    # off: no message; the command does not latch a reset, itime does
    assert g["s_off_on_sent"].tolist() == [1, 0, 0, 1, 1, 1] and g["s_off_on_state"].tolist() == [fc.SPEC, fc.PASSBAND, 11, 0]
    # the rate is captured at the reset only
    t = g["s_rate_change_times"]
    assert t[1] == fc.FFT_SEC[20250] and g["s_rate_change_state"][2] == 5
    assert os.path.getsize(os.path.join(fc.GOLD, "fftext_ref.npz")) <= 300000


REFUSALS = {
    # what the reference leaves undefined -> the host driver's exit status (10 + the refusal's number)
    "integ_time_never_set": (["R 12000", "S 2 0 2", "B 0 4"], 11),           # fmod(fi, 0) is NaN, (int) of it indexes pwr
    "integ_time_zero": (["R 12000", "I 0", "S 2 0 2", "B 0 4"], 11),
    "integ_time_negative": (["R 12000", "I -0.5", "S 2 0 2", "B 0 4"], 11),
    "integ_time_inf": (["R 12000", "I inf", "S 2 0 2", "B 0 4"], 12),         # bins: (int) inf
    "integ_time_nan": (["R 12000", "I nan", "S 2 0 2", "B 0 4"], 12),
    "wf_time_nan": (["R 12000", "I nan", "S 0 0 2", "B 0 4"], 12),            # the reset computes bins under every function
    "bins_at_2_31": (["R 12000", "I %r" % ((2.0 ** 31 + 1000) * fc.FFT_SEC[12000]), "S 2 0 2", "B 0 4"], 12),
    "bins_far_negative": (["R 12000", "I -1e300", "S 0 0 2", "B 0 4"], 12),
    "run_3": (["R 12000", "S 3 0 2"], 13),
    "run_minus_2": (["R 12000", "S -2 0 2"], 13),
}
ACCEPTED = {
    "bins_below_2_31": ["R 12000", "I %r" % ((2.0 ** 31 - 1000) * fc.FFT_SEC[12000]), "S 2 0 2", "B 0 4"],
    "time_tiny": ["R 12000", "I 1e-300", "S 2 0 2", "B 0 4", "B 0 5"],
    "wf_time_negative": ["R 12000", "I -0.5", "S 0 0 2", "B 0 4"],         # bins = -11, never used outside integ
    "other_instance_before_the_refusal": ["R 12000", "S 2 0 2", "B 1 4"],     # ignored before anything else
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(pool, driver, tmp_path, name):
    lines, status = REFUSALS[name]
    fc.run_script_exe(driver, lines, pool[1], tmp_path, expect=status)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_neighbours_of_the_refusals_are_taken(pool, driver, tmp_path, name):
    got = fc.run_script_exe(driver, ACCEPTED[name], pool[1], tmp_path)
    assert got["sent"].tolist() == ([0] if name.startswith("other") else [1] * fc.nblocks(ACCEPTED[name])) and not got["bins"].any()


def test_fftext_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib, fftext
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s, (proto, nargs) in FFTEXT_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert hasattr(lib, s), s
    # every device pointer of the new prototypes is typed
    protos = re.findall(r"\b(kg_(?:rxbank_)?fftext\w*)\s*\(([^;{}()]*)\)\s*;", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert len(protos) == len(FFTEXT_SYMBOLS) and not [n for n, a in protos if re.search(r"\bvoid\s*\*", a)]
    h = {k: int(v) for k, v in re.findall(r"\bKG_FFTEXT_([A-Z]+)\s*=\s*(-?\d+)", header)}
    assert (h["OFF"], h["WF"], h["SPEC"], h["INTEG"]) == (fc.OFF, fc.WF, fc.SPEC, fc.INTEG) == (fftext.OFF, fftext.WF, fftext.SPEC, fftext.INTEG)
    d = {k: int(v) for k, v in re.findall(r"#define KG_FFTEXT_(\w+)\s+(\d+)", header)}
    assert (d["ROW"], d["MAX_BINS"], d["UPDATE_MS"]) == (fc.W, fc.MAX_BINS, 100) == (fftext.ROW, fftext.MAX_BINS, fftext.UPDATE_MS)
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_fftext.h")).read()
    for lit in ("WIDTH = 1024", "MAX_BINS = 200", "UPDATE_MS = 100", "FUNC_OFF = -1, FUNC_WF = 0, FUNC_SPEC = 1, FUNC_INTEG = 2"):
        assert lit in src, lit


# ---- seeded random scripts (tests/ext_random.py): the combinations of commands and blocks nobody wrote down
@pytest.fixture(scope="module")
def random_ref():
    from . import ext_random as er
    return er.load("fftext")


def test_random_scripts_host_model_equals_the_fixture(random_ref, pool, driver, tmp_path):
    """every seed's script is the one the reference was fed, the host model takes it (exit status 0) and equals the reference in every
    field the fixture keeps: which blocks sent a row and its bin, the end state's scalars and ncma, and the digests of the rows and of
    the 200 x 1024 sums"""
    from . import ext_random as er
    for seed in range(er.NSEED):
        lines = er.fftext_script(seed)
        er.check_record("fftext", seed, lines, fc.run_script_exe(driver, lines, pool[1], tmp_path), er.unpack(random_ref, seed))


def test_random_fixture_meets_its_conditions(random_ref):
    """conditions, not measurements: what the 40 seeds must reach between them (ext_random.FFTEXT_CONDITIONS), computed from the fixture
    and the regenerated scripts; none of the 40 was refused by the reference.  The walk also holds its own answer of which blocks send
    a row to the reference's.  "block dropped past bin 199" is a block for which the reference sent nothing because its bin was 200 or
    above: the long integrations of the generator reach it"""
    from . import ext_random as er
    er.check_conditions("fftext", random_ref)
    assert os.path.getsize(er.fixture_path("fftext")) <= 64 * 1024


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "device_resident"])
def test_random_side_by_side_plans_share_their_calls(resident):
    """the calls tests/test_fftext_gpu.py makes with the seeds three at a time on one object are decided ahead of the run
    (ext_random_dev.plan_side_by_side): over all the groups at least half of them carry more than one channel"""
    from . import ext_random_dev as ed
    every, both = ed.shared_in_all("fftext", resident)
    assert 2 * both >= every, (both, every)
