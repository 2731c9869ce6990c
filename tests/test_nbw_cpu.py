"""kg_nbw.h, the arithmetic of NB_WILD (rx/Teensy/NB_Wild.cpp and the eight scalar CMSIS routines it calls) that kg_post's kernel
runs, compiled for the host with g++ -O2 -ffp-contract=off (the reference's flags) in the driver tools/nbw_host_driver.cpp, against
every scenario of tests/golden/nbw_ref.npz (made by tools/make_ref_nbw_golden.py from the reference's own statements) -- BIT-EXACT:
every output sample or block digest, every state record (thresh, taps, impulse_samples, the carried history), the hits of every
block and the largest float each block handed to the int16 conversion.  Then the conditions the golden file must meet so that the
parity tests cannot pass vacuously, the refusals of the command layer, the header's constants and the C ABI."""
import os
import re

import numpy as np
import pytest

from . import nbw_common as nc

ROOT = nc.ROOT
NBW_SYMBOLS = {"kg_post_nbw_init": "int kg_post_nbw_init(kg_post *post, int chan, const float *nb_param",
               "kg_post_set_nbw": "int kg_post_set_nbw(kg_post *post, int chan, int on);",
               "kg_post_nbw_process_dev": "int kg_post_nbw_process_dev(kg_post *post, const int32_t *chans, int nch, const void *d_in, "
                                          "size_t in_stride, int nsamps, void *d_out,",
               "kg_post_nbw_state": "int kg_post_nbw_state(kg_post *post, const int32_t *chans, int nch, int32_t *ints, float *floats);",
               "kg_rxbank_nbw_select": "int kg_rxbank_nbw_select(kg_rxbank *bank, int rx);"}
NARGS = {"kg_post_nbw_init": 3, "kg_post_set_nbw": 3, "kg_post_nbw_process_dev": 8, "kg_post_nbw_state": 5, "kg_rxbank_nbw_select": 2}


@pytest.fixture(scope="module")
def golden():
    return nc.load()


@pytest.fixture(scope="module")
def streams():
    return nc.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return nc.build_driver(tmp_path_factory.mktemp("nbw"))


@pytest.fixture(scope="module")
def runs(golden, streams, driver, tmp_path_factory):
    """every scenario through the host driver: name -> (output, states, hits, max |float|)"""
    tmp = tmp_path_factory.mktemp("nbw_runs")
    out = {}
    for name in nc.names(golden):
        y, st, hits, mx, rc = nc.run_driver(driver, nc.script(golden, name), nc.scenario_input(golden, name, streams), tmp)
        assert rc == 0, (name, rc)
        out[name] = (y, st, hits, mx)
    return out


def test_pool_rebuilds(golden, streams):
    """the seeded streams are the ones the reference binary was fed"""
    assert sorted(streams) == [str(n) for n in golden["pool_names"]]
    for k, want in zip(sorted(streams), golden["pool_sha"]):
        assert nc.digest(streams[k].tobytes()) == bytes(want), k


def test_scenarios_bit_exact(golden, runs):
    assert len(runs) >= 18
    for name, (y, states, hits, mx) in runs.items():
        nc.check_blocks(name, y, golden, "host driver")
        si = golden[name + "_state_i"]
        assert len(states) == len(si), name
        for k, (iv, th, hist) in enumerate(states):
            assert np.array_equal(iv, si[k]), (name, k, iv, si[k])              # nb_algo and nb_enable[NB_BLANKER] too
            nc.check_state(name, k, iv, th[0], hist, golden, "host driver")
        assert np.array_equal(hits, golden[name + "_hits"]), (name, "hits per block", hits, golden[name + "_hits"])
        assert np.array_equal(mx.view(np.uint32), golden[name + "_max_abs"].view(np.uint32)), (name, "largest float per block")


def test_golden_file_meets_its_conditions(golden, streams):
    """conditions, not measurements: without them the parity tests could pass on a file that never leaves the easy path"""
    g = golden
    assert int(g["defaults_noisy_hits"].max()) == 20 and int(g["defaults_noisy_hits"].min()) >= 1       # the cap of 20 is reached
    assert 0 < np.count_nonzero(g["sparse_hits"]) < g["sparse_hits"].size                              # some blocks hit, some do not
    assert g["limits_40_41_state_i"][-1][:2].tolist() == [40, 41] and g["limits_40_41_hits"].sum() > 0
    assert g["least_1_2_state_i"][-1][:2].tolist() == [1, 2] and g["least_1_2_hits"].sum() > 0
    assert g["even_samples_12_state_i"][-1][1] == 12                                                   # impulse_length = 13
    # a threshold that never triggers: the pure delay of order + PL = 13
    x = nc.scenario_input(g, "never_triggers", streams)
    assert g["never_triggers_hits"].sum() == 0 and np.array_equal(g["never_triggers_out"][13:], x[:-13]) and not g["never_triggers_out"][:13].any()
    # silence: no hit, the input delayed, no NaN; then signal with hits
    assert g["silence_then_signal_hits"][:6].sum() == 0 and g["silence_then_signal_hits"][6:].sum() > 0
    assert not g["silence_then_signal_state_h"][0].any()
    # clicks at the block edges: a hit in each of the eight blocks that hold one, for both vectors
    for name in ("edge_clicks", "edge_clicks_40_41"):
        assert np.count_nonzero(g[name + "_hits"]) == 8, (name, g[name + "_hits"])
    # two clicks closer than impulse_length + order = 17: both found in one block
    assert g["close_clicks_hits"].max() >= 2
    # the re-init zeroes the history and changes the delay
    assert g["reinit_midstream_state_i"][:, 0].tolist() == [10, 20, 20, 20]
    assert g["reinit_midstream_state_h"][0].any() and not g["reinit_midstream_state_h"][1].any()
    # the three messages from a fresh state pass through unusable vectors
    assert g["three_messages_fresh_state_i"][:4, :2].tolist() == [[0, 0], [0, 0], [10, 0], [10, 7]]
    assert g["three_messages_fresh_state_t"][:4].tolist() == [0.0, 3.0, 3.0, 3.0]
    # 12000 and 20250 share streams and give the same samples: the stage has no rate
    assert {int(g[n + "_rate"]) for n in nc.names(g)} == {12000, 20250}
    assert np.array_equal(g["sparse_out_sha"], g["sparse_20250_out_sha"])
    # a repair left int16 and the conversion wrapped as the x86 binary's does
    assert int(g["leaves_int16"]) == 1 and g["loud_defaults_max_abs"].max() > 32767.0
    for name in nc.names(g):
        assert np.isfinite(g[name + "_max_abs"]).all(), name
    assert os.path.getsize(os.path.join(nc.GOLD, "nbw_ref.npz")) <= os.path.getsize(os.path.join(nc.GOLD, "nrs_ref.npz"))


def test_conversion_wraps_as_the_reference(golden, runs):
    """the block of loud_defaults whose repair left int16: the driver's samples are the reference's (digests), and some sample differs
    from saturation"""
    name = "loud_defaults"
    over = np.flatnonzero(golden[name + "_max_abs"] > 32767.0)
    assert over.size
    y = runs[name][0]
    b = int(over[0])
    blk = y[b * nc.BLK:(b + 1) * nc.BLK].astype(np.int32)
    assert np.abs(np.diff(blk)).max() > 32768


def test_command_refusals(driver, tmp_path):
    """the stage is never switched on over a vector NB_Wild.cpp cannot run on, and storing is never refused while it is off"""
    x = np.zeros(512, np.int16)
    run = lambda lines: nc.run_driver(driver, lines + ["B 512 0"], x, tmp_path)[4]
    assert run(["A 2", "E 0 1"]) == 6                                   # never initialised: taps 0
    assert run(["A 2", "P 0 0 3", "P 0 1 10", "E 0 1"]) == 6            # impulse_samples 0
    assert run(["A 2", "P 0 0 3", "P 0 1 0", "P 0 2 7", "E 0 1"]) == 6  # taps 0
    assert run(["A 2", "P 0 0 3", "P 0 1 41", "P 0 2 7", "E 0 1"]) == 6
    assert run(["A 2", "P 0 0 3", "P 0 1 10", "P 0 2 42", "E 0 1"]) == 6
    assert run(["A 2", "P 0 0 3", "P 0 1 10", "P 0 2 1", "E 0 1"]) == 6
    assert run(["A 2", "P 0 0 nan", "P 0 1 10", "P 0 2 7", "E 0 1"]) == 6
    assert run(["A 2", "P 0 0 inf", "P 0 1 10", "P 0 2 7", "E 0 1"]) == 6
    assert run(["A 2", "P 0 0 3", "P 0 1 300", "P 0 2 7", "E 0 1"]) == 6  # outside s1_t
    assert run(["A 2", "P 0 0 3", "P 0 1 10", "P 0 2 7", "E 0 1"]) == 0
    assert run(["A 2", "P 0 0 3", "P 0 1 40", "P 0 2 41", "E 0 1"]) == 0
    assert run(["A 2", "P 0 0 3", "P 0 1 1", "P 0 2 2", "E 0 1"]) == 0
    assert run(["A 2", "P 0 0 3", "P 0 1 10", "P 0 2 7", "E 0 1", "P 0 1 0"]) == 6      # unusable while on
    assert run(["A 2", "P 0 0 3", "P 0 1 10", "P 0 2 7", "E 0 1", "E 0 0", "P 0 1 0"]) == 0
    assert run(["A 1", "P 0 1 0", "E 0 1"]) == 0                        # other algos: not this stage's business


def test_random_scripts_are_accepted(driver, tmp_path):
    """the scripts tools/fuzz_parity.py draws never ask for what the library refuses (exit status 6), whatever the seed: the soak
    compares outputs, the refusals have their own tests.  Among them are scripts with a parameter change after a new connection."""
    after_c = 0
    for seed in range(150):
        lines = nc.random_script(np.random.default_rng(seed))
        nb = sum(1 for l in lines if l[0] == "B")
        rc = nc.run_driver(driver, lines, np.zeros(nb * nc.BLK, np.int16), tmp_path)[4]
        assert rc == 0, (seed, rc, lines)
        if "C" in lines:
            after_c += any(l.startswith("P 0 ") for l in lines[lines.index("C"):])
    assert after_c >= 5


def test_all_zero_input_is_the_pure_delay(driver, tmp_path):
    """R[0] = 0 makes k NaN and every comparison false: the output equals the input and no NaN reaches it"""
    x = np.zeros(4 * 512, np.int16)
    x[700] = 1234                                                       # one sample, then silence again: block 1 is not all zero
    y, st, hits, mx, rc = nc.run_driver(driver, ["A 2", "P 0 0 0.95", "P 0 1 10", "P 0 2 7", "E 0 1"] + ["B 512 0"] * 4, x, tmp_path)
    assert rc == 0 and hits[0] == 0 and hits[2] == 0 and hits[3] == 0 and np.isfinite(mx).all()
    assert not y[:512].any() and not y[1024 + 13:].any()


def test_header_constants_equal_the_reference(golden):
    text = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    h = {k: int(v) for k, v in re.findall(r"\bKG_(NBW?_[A-Z_]+)\s*=\s*(\d+)", text)}
    ref = dict(zip((str(n) for n in golden["const_names"]), (float(v) for v in golden["const_values"])))
    assert h["NB_WILD"] == ref["NB_WILD"] and h["NB_BLANKER"] == ref["NB_BLANKER"] and h["NB_PARAMS"] == ref["NOISE_PARAMS"]
    assert (h["NBW_THRESH"], h["NBW_TAPS"], h["NBW_SAMPLES"]) == (ref["NB_THRESH"], ref["NB_TAPS"], ref["NB_SAMPLES"])
    assert h["NBW_HIST"] == 2 * ref["MAX_ORDER"] + 2 * ((ref["MAX_IMPULSE_LEN"] - 1) // 2) == nc.HIST
    assert h["NBW_MAX_SAMPLES"] % ref["FASTFIR_OUTBUF_SIZE"] == 0
    from flydog_sdr_gps_amd import post
    assert (post.NB_THRESH, post.NB_TAPS, post.NB_SAMPLES) == (ref["NB_THRESH"], ref["NB_TAPS"], ref["NB_SAMPLES"]) == (0, 1, 2)
    assert (post.NBW_BLOCK, post.NBW_MAX_ORDER, post.NBW_MAX_IMPULSE_LEN, post.NBW_HIST) == \
        (ref["FASTFIR_OUTBUF_SIZE"], ref["MAX_ORDER"], ref["MAX_IMPULSE_LEN"], nc.HIST)
    assert post.nbw_delay(10, 7) == 13 and post.nbw_delay(40, 41) == 60 and post.nbw_delay(1, 2) == 2 and post.nbw_delay(16, 12) == 22
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_nbw.h")).read()
    for lit in ("BLOCK = %d" % ref["FASTFIR_OUTBUF_SIZE"], "MAX_ORDER = %d" % ref["MAX_ORDER"], "MAX_IMPULSE_LEN = %d" % ref["MAX_IMPULSE_LEN"],
                "N_IMPULSE_COUNT = %d" % ref["N_IMPULSE_COUNT"], "P_THRESH = %d, P_TAPS = %d, P_SAMPLES = %d" % (ref["NB_THRESH"], ref["NB_TAPS"], ref["NB_SAMPLES"])):
        assert lit in src, lit
    assert ref["DIM_WBUF"] == ref["FASTFIR_OUTBUF_SIZE"] + nc.HIST == 632


def test_nbw_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s, proto in NBW_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == NARGS[s], s
        assert hasattr(lib, s), s
    assert "#define KG_ABI_VERSION 4" in header or re.search(r"KG_ABI_VERSION\s*=?\s*4\b", header)
