"""The tracking channels without a GPU: kg_trk.h, the closed form the kernel runs, compiled for the host as one lane
(tools/trk_host_driver.cpp), against the LITERAL clock-by-clock model (tools/trk_model.cpp) -- every epoch record, every GPS_CHAN byte,
every replica word EQUAL -- on every scenario of tests/trk_common.py and on seeded random scripts; the model's C/A generator against
prn.py; CloseLoop on its corner cases; the C ABI; and the lock check: the model acquires (through the oracle and the
kg_acq_chan_start arithmetic), locks and returns the data bits of a synthetic scene."""
import os
import re

import numpy as np
import pytest

from . import trk_common as tc

ROOT = tc.ROOT
NARGS = {"kg_trk_create": 5, "kg_trk_destroy": 1, "kg_trk_set_sat": 3, "kg_trk_set_e1b_code": 4, "kg_trk_set_rate_lo": 3, "kg_trk_set_rate_cg": 3,
         "kg_trk_set_gain_lo": 4, "kg_trk_set_gain_cg": 4, "kg_trk_set_polarity": 3, "kg_trk_set_mask": 2, "kg_trk_sampler_reset": 1,
         "kg_trk_pause": 3, "kg_trk_set_loop": 3, "kg_trk_process_bits_dev": 7, "kg_trk_process_bits": 7, "kg_trk_get_chan": 3,
         "kg_trk_get_clocks": 3}


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("trk")
    return tc.build(d, "trk_model"), tc.build(d, "trk_host_driver"), d


def test_model_ca_chips_equal_prn_py(tools):
    """all 36 L1 / QZSS rows of sats.py, 1023 chips: the model's CACODE (C++ and its Python restatement) and the closed form's table"""
    from flydog_sdr_gps_amd import prn, sats, trk
    model, host, tmp = tools
    rows = [i for i, s in enumerate(sats.SATS) if s[3] != sats.E1B]
    assert len(rows) == 36
    lines = ["N 1 216 577"]
    for i in rows:
        lines += ["S 0 %d" % trk.codegen_init(i), "Q 0"]
    got_m, got_h = tc.run_lines(model, lines, tmp), tc.run_lines(host, lines, tmp)
    assert len(got_m) == len(got_h) == 36
    for k, i in enumerate(rows):
        _, t1, t2, _ = sats.SATS[i]
        want = "".join(str(int(c)) for c in prn.cacode(t1, t2))
        assert got_m[k][2] == want, ("model", sats.SATS[i])
        assert got_h[k][2] == want, ("closed form", sats.SATS[i])
        assert "".join(str(int(c)) for c in tc.ca_chips_literal(trk.codegen_init(i))) == want, sats.SATS[i]


REFUSED = {"refused_cmds": [13, 15, 19]}          # scenario -> the steps the command layer refuses (KG_ERR_STATE, nothing changed)


@pytest.mark.parametrize("name", sorted(tc.scenarios()))
def test_closed_form_equals_literal_model(tools, name):
    """a refused command changes nothing: the model is given the script without it"""
    model, host, tmp = tools
    sc = tc.scenarios()[name]
    got = tc.run_tool(host, sc, tmp)
    assert got["refused"] == REFUSED.get(name, []), name
    want = tc.run_tool(model, tc.without(sc, got["refused"]), tmp)
    assert sum(len(r) for r in want["records"]) >= sc.nchan and want["dumps"], name       # the scenario produced epochs
    tc.assert_equal(got, want, name)


def test_code_loop_leaving_the_range_stops_the_channel(tools):
    """the model's channel 0 writes 2^27 - 1 at its second service; the closed form stops there (the driver's exit status 7)"""
    model, host, tmp = tools
    sc = tc.fault_scenario()
    rates = [r[8] for r in tc.run_tool(model, sc, tmp)["records"][0]]
    assert rates[0] == tc.RATE_MIN and rates[1] == tc.RATE_MIN - 1
    with pytest.raises(AssertionError) as e:
        tc.run_tool(host, sc, tmp)
    assert e.value.args[0][:2] == ("fault", 7), e.value.args


def test_scenarios_reach_what_they_are_for(tools):
    """conditions on the model's own runs, so that the parity cases cannot pass on a file that never leaves the easy path"""
    from flydog_sdr_gps_amd import trk
    model, _, tmp = tools
    S = tc.scenarios()
    run = lambda n: tc.run_tool(model, S[n], tmp)
    chan = lambda hexes, ch: np.frombuffer(bytes.fromhex(hexes[ch]), trk.chan_dtype)[0]
    # integrator extremes: the early arm sits at +8184 and at -8184 (16368 clocks, lsb set on every other one)
    r = np.array(run("replica")["records"][0])
    assert r[:, 3].max() == 8184 and r[:, 3].min() == -8184, r[:, 3]
    # the nav ring wrapped: more than MAX_NAV_BITS E1B bits were saved
    w = run("e1b_nav130")
    assert len(w["records"][0]) >= 130 and chan(w["dumps"][0][0], 0)["nav_bits"] == len(w["records"][0]) - 128
    # pieces and one call are the same stream: the same records, the same final state
    a, b = run("one_call"), run("pieces")
    assert a["records"] == b["records"] and a["dumps"][-1] == b["dumps"][-1]
    # a pause of 16367 really shifts the epoch: channel 2's first epoch after it comes later than channel 0's
    p = run("pauses")
    assert len(p["records"][2]) < len(p["records"][0])
    # the masked half kept its phase through the second reset
    m = run("reset_masked")
    reps = m["dumps"][1][2]
    assert reps[0] != reps[1] or reps[2] != reps[3]
    # loop off: the NCO words stay as set, then move
    lo = np.array(run("loop_off")["records"][0])
    assert (lo[:5, 7] == tc.LO_NOM).all() and (lo[:5, 8] == tc.NOM).all() and (lo[5:, 7] != tc.LO_NOM).any()
    # C/A noise exercises the glitch counter; the E1B polarities differ in their code rate
    assert chan(run("ca_taps")["dumps"][0][0], 0)["nav_glitch"] > 0
    rates = [np.array(run("e1b_pol%d" % k)["records"][0])[-1, 8] for k in (0, 1, 2)]
    assert len(set(int(v) for v in rates)) == 3


def test_random_scripts(tools):
    """seeded scripts of every command between process calls of 1 .. 90000 clocks: every one runs and equals the model; the commands
    the library refuses (a pause, a code rate or a reset that would make a paused channel hold ms0 set) change nothing, so the model
    gets the script without them -- and some scripts do hold such commands"""
    model, host, tmp = tools
    refused = 0
    for seed in range(60):
        sc = tc.random_scenario(seed)
        got = tc.run_tool(host, sc, tmp)
        refused += len(got["refused"])
        tc.assert_equal(got, tc.run_tool(model, tc.without(sc, got["refused"]), tmp), sc.name)
    assert refused >= 3


def test_close_loop(tools):
    """CloseLoop on negative errors, ki = 0, kp - ki = 0 and 64-bit wrap, against Python integers"""
    model, host, tmp = tools
    M = (1 << 64) - 1
    cases = [(1 << 60, -1, 0, 0), (1 << 60, -12345678901, 11, 12), (0, -1, 20, 7), (M, 1, 0, 0), (M - 5, 3, 1, 62), (1 << 63, -(1 << 39), 24, 7),
             ((1 << 28) << 32, (1 << 39) - 1, 20, 7), (123456789 << 32, -(1 << 39), 0, 63), (5, 7, 63, 0), (M, -1, 63, 63)]
    lines = ["T %d %d %d %d" % c for c in cases]
    for exe in (model, host):
        got = tc.run_lines(exe, lines, tmp)
        for (f, e, ki, kpm), g in zip(cases, got):
            eki = ((e & M) << ki) & M
            nf = (f + eki) & M
            nco = ((nf + ((eki << kpm) & M)) & M) >> 32
            assert (int(g[1]), int(g[2])) == (nf, nco), (exe, f, e, ki, kpm)


def test_trk_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s, n in NARGS.items():
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == n, s
        assert hasattr(lib, s), s
    assert "#define KG_ABI_VERSION 4" in header
    # device pointers carry their element types (tests/test_containment_coverage_cpu.py lists the untyped ones only)
    proto = re.search(r"int kg_trk_process_bits_dev\(([^;]*)\);", header).group(1)
    assert "const uint8_t *d_bits" in proto and "kg_trk_epoch *d_epochs" in proto and "int32_t *d_counts" in proto and "void" not in proto
    import flydog_sdr_gps_amd as pkg
    assert pkg.Tracker is pkg.trk.Tracker and pkg.trk.epoch_dtype.itemsize == 48


@pytest.fixture(scope="module")
def lock_run(tools, oracle):
    from flydog_sdr_gps_amd import handoff, trk
    model, _, tmp = tools
    chips, bits = tc.lock_bits()
    acq, _ = oracle.correlate(oracle.code_fft(chips), oracle.sample_bits(bits[:8192]))
    start = handoff.chan_start(0, acq["dop"], acq["idx"] * handoff.DECIM, tc.LOCK_T0 / trk.FS)
    return acq, start, tc.run_tool(model, tc.lock_scenario(bits, start), tmp)


def test_lock_check_on_the_model(lock_run):
    """PRN 1 at +1500 Hz, 300.5 chips, 55 dB-Hz, 50 bps: acquired, started, locked over the last 200 epochs, the sent bits returned
    up to one global sign.  Margin seen: min (pp - pe) / pp = 0.59, min (pp - pl) / pp = 0.51 over those epochs; at
    52 dB-Hz 0.40 / 0.41, still locked."""
    from flydog_sdr_gps_amd import trk
    acq, start, w = lock_run
    assert acq["valid"] and abs(acq["dop"] * 249.755859375 - tc.LOCK_DOPPLER) < 125 and abs(acq["idx"] / 4 - tc.LOCK_TAU) <= 1
    assert 1 <= start.ca_pause <= 16368
    r = np.array(w["records"][0])
    assert len(r) >= tc.LOCK_MS - 6
    assert (r[-200:, 9] & trk.UNLOCKED).sum() == 0
    pp = r[-200:, 1].astype(float) ** 2 + r[-200:, 2].astype(float) ** 2
    pe = r[-200:, 3].astype(float) ** 2 + r[-200:, 4].astype(float) ** 2
    pl = r[-200:, 5].astype(float) ** 2 + r[-200:, 6].astype(float) ** 2
    print("lock margin: min (pp-pe)/pp %.3f, min (pp-pl)/pp %.3f" % (((pp - pe) / pp).min(), ((pp - pl) / pp).min()))
    # the carrier and code loops sit at the scene's Doppler
    lo_hz = r[-200:, 7].astype(float).mean() / 2.0 ** 32 * trk.FS - trk.FC
    cg_hz = r[-200:, 8].astype(float).mean() / 2.0 ** 32 * trk.FS - trk.CPS
    assert abs(lo_hz - tc.LOCK_DOPPLER) < 5 and abs(cg_hz - tc.LOCK_DOPPLER * trk.CPS / 1575.42e6) < 2
    # the data bits: the last 12 saved ones are 12 consecutive sent bits, or their complement, ending at the scene's last bit
    ch = np.frombuffer(bytes.fromhex(w["dumps"][0][0][0]), trk.chan_dtype)[0]
    got = trk.nav_bits_of(ch, 12)
    sent = tc.LOCK_DATA[:tc.LOCK_MS // 20]
    ends = [e for e in (len(sent) - 1, len(sent)) if np.array_equal(got, sent[e - 12:e]) or np.array_equal(got, 1 - sent[e - 12:e])]
    assert ends, (got, sent)
    assert int(ch["nav_bits"]) >= 15
