"""The tracking MODEL (tools/trk_model.cpp) against what a tracking channel must do on a signal -- every other trk test holds the
closed form and the kernel EQUAL to the model, and equality says nothing about a tap, latch order, sign or shift count that all three
share.  Scenes come from tests/trk_common.py (scene(): several satellites, gaps); every bar comes from the scene:

    carrier    |mean LO error over the last quarter| < 5 Hz (a fifth of the nearest C/A false lock at half the bit rate, 25 Hz)
    code       ca_unlocked is 0 on every epoch of the last quarter (the 48 dB-Hz case: on at most 1 %)
    data       the last K saved nav bits are the sent ones up to one global sign, ending at the scene's last or second-to-last bit
    no signal  ca_unlocked is set on at least half of the tail's epochs (three independent powers leave the prompt the largest a third
               of the time: over 200 epochs an expectation of 133 and an sd of 6.7, so 100 is five sd below)

Each case runs the model once, then the host closed form (tools/trk_host_driver.cpp) is held equal to that run.  One report line per
channel is printed (profiles/trk_signal_model.txt is that output).

Not asserted, written down: the Costas loop's pull-in limit on E1B.  With one symbol per 4 ms epoch it is 1 / (4 T) = 62.5 Hz, with a
false lock at 1 / (2 T) = 125 Hz in which ca_unlocked stays 0 (the firmware has no wider discriminator), so the E1B cases keep the
offset from the bin's centre at or below 30 Hz."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from . import trk_common as tc

CASES = {n: c for n, c in tc.signal_cases().items() if c["epochs"] is not None}
CARRIER_HZ = 5.0


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("trk_signal")
    return tc.build(d, "trk_model"), tc.build(d, "trk_host_driver"), d


def both(tools, sc):
    """the model's run and the closed form's, side by side; a command the closed form refuses changes nothing, so the model then gets
    the script without it"""
    model, host, tmp = tools
    with ThreadPoolExecutor(2) as ex:
        w = ex.submit(tc.run_tool, model, sc, tmp)
        h = tc.run_tool(host, tc.Scenario(sc.name + "_host", sc.nchan, sc.steps, bits=sc.bits, lo_delay=sc.lo_delay, cg_delay=sc.cg_delay,
                                          codes=sc.codes), tmp)
        w = w.result()
    if h["refused"]:
        w = tc.run_tool(model, tc.without(sc, h["refused"]), tmp)
    return w, h


@pytest.fixture(scope="module")
def runs(tools, oracle):
    """name -> (scenario, truths, acquisition, the model's run, the closed form's run), each case run once"""
    cache = {}

    def get(name):
        if name not in cache:
            sc, truths, acq = tc.case_scenario(CASES[name], oracle=oracle)
            cache[name] = (sc, truths, acq) + both(tools, sc)
        return cache[name]
    return get


def reports(name, truths, w):
    out = []
    for ch, tr in enumerate(truths):
        if tr is not None:
            out.append(tc.signal_report(w["records"][ch], w["dumps"][-1][0][ch], tr))
            print(tc.report_line(name, ch, out[-1]))
        else:
            out.append(None)
    return out


def assert_no_signal(name, ch, records, part):
    u, n = tc.unlocked_of(records, part)
    print("trk_signal %-18s ch %d  no signal: unlocked %d/%d" % (name, ch, u, n))
    assert n >= 100 and 2 * u >= n, (name, ch, u, n)


def assert_tracks(case, ch, rep, data=True):
    name = case["name"]
    assert abs(rep["lo_tail"]) < CARRIER_HZ, (name, ch, rep)
    u, n = rep["unlocked"]
    assert n >= 40 and u <= case["max_unlocked"] * n, (name, ch, rep)
    if data:
        assert rep["match"] is not None, (name, ch, rep)


def test_scene_with_one_satellite_is_scene_bits():
    """scene() on lock_bits()' arguments: byte for byte trk.scene_bits; and on an E1B satellite (boc, one bit per epoch)"""
    from flydog_sdr_gps_amd import trk
    chips, want = tc.lock_bits()
    got = tc.scene([tc.sv(chips, tc.LOCK_TAU, tc.LOCK_DOPPLER, tc.LOCK_CN0, tc.LOCK_DATA)], tc.LOCK_MS * tc.CA_EPOCH, tc.LOCK_SEED)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    e = tc.e1b_code(1)
    n = (1 << 20) + 12345                                                       # more than one block, not a multiple of 8
    want = trk.scene_bits(e, n, 1777.25, -2227.8, 50.0, tc.sat_data(3), seed=9, theta=0.2, boc=True, bit_epochs=1)
    assert np.array_equal(tc.scene([tc.sv(e, 1777.25, -2227.8, 50.0, tc.sat_data(3), boc=True, bit_epochs=1, theta=0.2)], n, 9), want)
    # a gap takes the satellite out and leaves the noise draw alone: outside the gap the bytes are the same
    gap = tc.scene([tc.sv(e, 1777.25, -2227.8, 50.0, tc.sat_data(3), boc=True, bit_epochs=1, theta=0.2)], n, 9, gaps=((80000, 160000),))
    assert np.array_equal(gap[:10000], want[:10000]) and np.array_equal(gap[20000:], want[20000:]) and not np.array_equal(gap, want)


@pytest.mark.parametrize("name", ["ca_pull_p100", "ca_pull_m120", "ca_pull_p60_48", "e1b_p0", "e1b_p30", "qzss_m1000"])
def test_pull_in_and_track(runs, name):
    """cases 1, 2 and 4: the NCOs start at the centre of the acquisition bin and the scene lies beside it (C/A +100 Hz, -120 Hz, and
    +60 Hz at 48 dB-Hz; E1B 0 and +30 Hz; QZSS at -1000 Hz + 25 Hz): the carrier loop pulls in, the code stays locked, the bits come out.
    Convergence seen (profiles/trk_signal_model.txt): +100 Hz within 400 of 1500 epochs, -120 Hz within 1500 of 3000, 48 dB-Hz within
    2000 of 4000."""
    sc, truths, _, w, h = runs(name)
    rep = reports(name, truths, w)[0]
    if name.startswith("ca_pull"):                                              # the loop had to move: it started outside the bar
        word = [s for s in sc.steps if s[0] == "L"][-1][2]
        assert abs(tc.lo_hz([(0,) * 7 + (word,)])[0] - truths[0]["doppler_hz"]) >= 60
    assert_tracks(CASES[name], 0, rep)
    tc.assert_equal(h, w, name)


def test_e1b_polarity(tools):
    """case 3: the E1B scene of case 2, 40 epochs, one per X step with a dump after each.  err = ACF + |ACF| (polarity 1) is never
    negative and ACF - |ACF| (polarity 2) never positive, so ch_CA_FREQ only rises / only falls from dump to dump; under polarity 0
    it does both"""
    from flydog_sdr_gps_amd import trk
    case = CASES["e1b_p0"]
    bits = tc.scene(case["svs"], 40 * tc.E1B_EPOCH, case["seed"])
    for pol in (0, 1, 2):
        steps = tc.start_at_bin(0, tc.E1B_MODE, -9, True, code=0, pol=pol) + [("R",)] + [("X", tc.E1B_EPOCH), ("D",)] * 40
        sc = tc.Scenario("e1b_signal_pol%d" % pol, 1, steps, bits=bits, codes=[tc.e1b_code(1)])
        w, h = both(tools, sc)
        f = np.array([int(np.frombuffer(bytes.fromhex(d[0][0]), trk.chan_dtype)[0]["ca_freq"]) for d in w["dumps"]], object)
        d = np.array([int(b) - int(a) for a, b in zip(f[:-1], f[1:])], object)
        up, down = int(sum(x > 0 for x in d)), int(sum(x < 0 for x in d))
        print("trk_signal e1b polarity %d: ca_freq rose %d times, fell %d times in %d dumps" % (pol, up, down, len(f)))
        assert len(f) == 40
        assert (up >= 1 and down == 0) if pol == 1 else (down >= 1 and up == 0) if pol == 2 else (up >= 1 and down >= 1), (pol, up, down)
        tc.assert_equal(h, w, sc.name)


EDGE_PAUSE = {"edge_ca_tau0": lambda p: p == tc.CA_EPOCH, "edge_ca_tau_end": lambda p: 1 <= p <= 8,
              "edge_e1b_tau0": lambda p: p == tc.E1B_EPOCH, "edge_e1b_tau1777": lambda p: 1 <= p <= tc.E1B_EPOCH}


@pytest.mark.parametrize("name", sorted(EDGE_PAUSE))
def test_handoff_edges(runs, name):
    """case 5: acquired by the oracle on the first 8192 bytes and started through the kg_acq_chan_start arithmetic 65536 clocks after the
    reset, as the lock check is: ca_shift 0 (a pause of one whole epoch, C/A 16368 and E1B 65472) and ca_shift one sample before the
    epoch's end (a pause of 4).  The acquisition's index is 4 tau + 0.3 rounded (seen on 100 scenes), so tau = 1022.7 is what gives
    index 4091; at 1022.8 it gives 0 on 19 scenes of 20."""
    sc, truths, (acq, start), w, h = runs(name)
    v = CASES[name]["svs"][0]
    L = v["chips"].size
    assert acq["valid"] and acq["dop"] == round(v["doppler_hz"] / tc.BIN_HZ), acq
    assert abs((acq["idx"] / 4 - v["code_phase"] + L / 2) % L - L / 2) <= 1, acq
    print("trk_signal %-18s acquired bin %d idx %d ca_pause %d" % (name, acq["dop"], acq["idx"], start.ca_pause))
    assert EDGE_PAUSE[name](start.ca_pause), start.ca_pause
    assert_tracks(CASES[name], 0, reports(name, truths, w)[0])
    tc.assert_equal(h, w, name)


def test_loss_of_signal(runs):
    """case 6: 500 epochs of PRN 1 at 55 dB-Hz, then noise: locked while it is there, ca_unlocked up on at least half of the epochs
    after it, the prompt's mean |ip| below a quarter"""
    sc, truths, _, w, h = runs("loss")
    r = w["records"][0]
    rep = reports("loss", truths, w)[0]                                         # tail: epochs 300-500
    assert len(r) >= 890
    assert_tracks(CASES["loss"], 0, rep, data=False)
    assert rep["unlocked"] == (0, 200)
    assert_no_signal("loss", 0, r, slice(520, 900))
    ip = np.abs(np.array([e[1] for e in r], np.float64))
    print("trk_signal loss               mean |ip| %.0f over 300-500, %.0f over 700-900" % (ip[300:500].mean(), ip[700:900].mean()))
    assert ip[700:900].mean() < ip[300:500].mean() / 4
    tc.assert_equal(h, w, "loss")


def test_wrong_prn(runs):
    """case 7: a channel on PRN 1, a scene holding PRN 7 only (same bin, 55 dB-Hz)"""
    sc, truths, _, w, h = runs("wrong_prn")
    assert truths == [None] and len(w["records"][0]) >= 395
    assert_no_signal("wrong_prn", 0, w["records"][0], CASES["wrong_prn"]["tail"])
    tc.assert_equal(h, w, "wrong_prn")


def test_bank_on_one_stream(runs):
    """case 8: PRN 1 (52 dB-Hz, bin 6 + 40 Hz), PRN 7 (50, bin -13 - 55), QZSS 194 (52, bin 2 + 80) and an E1B code (50, bin -9 + 20) in
    one stream of 1500 C/A epochs; six channels: those four, PRN 4 (absent), and PRN 1 once more with the LO gain lowered by one"""
    sc, truths, _, w, h = runs("bank")
    rep = reports("bank", truths, w)
    assert [t is None for t in truths] == [False, False, False, False, True, False]
    for ch in (0, 1, 2, 3, 5):
        assert_tracks(CASES["bank"], ch, rep[ch])
    r = w["records"][4]
    assert_no_signal("bank", 4, r, slice(len(r) - len(r) // 4, None))
    # the two PRN 1 channels differ (another gain), and reach the same carrier
    assert w["records"][0] != w["records"][5]
    tc.assert_equal(h, w, "bank")
