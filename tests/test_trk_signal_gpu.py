"""The tracking kernel (kg_trk) against the LITERAL model (tools/trk_model.cpp) on SIGNALS: every epoch record, every GPS_CHAN byte,
every replica word EQUAL, on shortened forms of the scenes on which tests/test_trk_signal_cpu.py holds the model to what a tracking
channel must do -- a C/A carrier pull-in in pieces of 100001 clocks, E1B in lock, a bank of six channels on one stream of four
satellites, a loss of signal, E1B end to end through kg_acq_* and kg_acq_chan_start -- and on the seeded random scripts the host closed
form runs.  Each test has one reach condition on the model's run, so that it cannot pass without leaving the easy path."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Searcher, handoff, sats, trk
from . import trk_common as tc

pytestmark = pytest.mark.gpu

CASES = tc.signal_cases()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("trk_signal_gpu")
    return tc.build(d, "trk_model"), d


def run_both(gpu_ctx, model, name):
    exe, tmp = model
    sc, truths, _ = tc.case_scenario(CASES[name], gpu=True)
    want = tc.run_tool(exe, sc, tmp)
    got = tc.run_gpu(gpu_ctx, sc)
    assert got["refused"] == []
    tc.assert_equal(got, want, name)
    return sc, truths, want


def test_ca_pull_in(gpu_ctx, model):
    """PRN 1 at 55 dB-Hz, 100 Hz above the centre of bin 6, 800 epochs in X steps of 100001 clocks: the LO word moves by more than
    50 Hz and ends within 5 Hz of the scene, and the glitch counter ran (the sign of ip turns with the beat until the loop is in)"""
    sc, truths, want = run_both(gpu_ctx, model, "ca_pull_p100")
    assert sum(s[0] == "X" for s in sc.steps) == 800 * tc.CA_EPOCH // 100001 + 1
    lo = tc.lo_hz(want["records"][0])
    assert lo.max() - lo.min() > 50 and abs(lo[-50:].mean() - truths[0]["doppler_hz"]) < 5, (lo[0], lo[-1])
    ch = np.frombuffer(bytes.fromhex(want["dumps"][-1][0][0]), trk.chan_dtype)[0]
    assert int(ch["nav_glitch"]) >= 10, ch


def test_e1b_in_lock(gpu_ctx, model):
    """the stand-in E1B code with BOC(1,1) at 50 dB-Hz, 30 Hz above the centre of bin -9, 200 epochs: locked over the last 50"""
    _, _, want = run_both(gpu_ctx, model, "e1b_p30")
    assert len(want["records"][0]) >= 198 and tc.unlocked_of(want["records"][0], slice(-50, None)) == (0, 50)


def test_bank_on_one_stream(gpu_ctx, model):
    """PRN 1, PRN 7, QZSS 194 and an E1B code in one stream at 55 dB-Hz, each within 30 Hz of its bin; six channels in one call of 600
    C/A epochs: those four, PRN 4 (absent), PRN 1 again with the LO gain lowered by one.  Every channel with a satellite is locked
    over its last quarter"""
    _, truths, want = run_both(gpu_ctx, model, "bank_gpu")
    for ch, tr in enumerate(truths):
        r = want["records"][ch]
        if tr is not None:
            u, n = tc.unlocked_of(r, slice(len(r) - len(r) // 4, None))
            assert u == 0 and n >= (37 if tr["e1b"] else 149), (ch, u, n)


def test_loss_of_signal(gpu_ctx, model):
    """300 epochs of PRN 1, then 200 of noise: locked over epochs 200-300, ca_unlocked up on at least half of the last 150"""
    _, _, want = run_both(gpu_ctx, model, "loss")
    r = want["records"][0]
    assert len(r) >= 495 and tc.unlocked_of(r, slice(200, 300)) == (0, 100)
    u, n = tc.unlocked_of(r, slice(-150, None))
    assert n == 150 and 2 * u >= n, u


def test_e1b_end_to_end(gpu_ctx, model, oracle):
    """tau = 1777.25 chips, 20 Hz above the centre of bin -9, 150 epochs: Searcher.set_code(boc=True) and search() on the first 8192
    bytes give the oracle's lo_shift and ca_shift; handoff.chan_start(1, ...) and the Tracker equal the model"""
    exe, tmp = model
    case = CASES["edge_e1b_tau1777"]
    sc, truths, (want_acq, want_start) = tc.case_scenario(case, gpu=True, oracle=oracle)
    chips = case["svs"][0]["chips"]
    s = Searcher(gpu_ctx)
    try:
        s.set_code(0, chips, boc=True)
        out = s.search([0], packed=sc.bits[:8192])[0]
    finally:
        s.close()
    assert out.valid and (out.lo_shift, out.ca_shift) == (want_acq["dop"], want_acq["idx"] * handoff.DECIM) and out.lo_shift == -9
    start = handoff.chan_start(1, out.lo_shift, out.ca_shift, tc.LOCK_T0 / trk.FS)
    assert 1 <= start.ca_pause <= sats.E1B_LIMIT * handoff.DECIM
    sc = tc.start_acquired("e1b_e2e", sc.bits, case["chans"][0]["word"], True, start, tc.LOCK_T0, 150 * tc.E1B_EPOCH, codes=sc.codes)
    want = tc.run_tool(exe, sc, tmp)
    got = tc.run_gpu(gpu_ctx, sc)
    assert got["refused"] == []
    tc.assert_equal(got, want, "E1B end to end")
    r = want["records"][0]
    assert len(r) >= 147 and tc.unlocked_of(r, slice(-50, None)) == (0, 50)


def test_random_scripts(gpu_ctx, model):
    """tc.random_scenario(0 .. 19) -- every command between process calls of 1 .. 90000 clocks, which the 64 lanes share out -- equal
    to the model; a command the library refuses changes nothing, so the model gets the script without it.  The 20 scripts together
    hold at least one refused command and at least one E1B channel"""
    exe, tmp = model
    refused = e1b = 0
    for seed in range(20):
        sc = tc.random_scenario(seed)
        got = tc.run_gpu(gpu_ctx, sc)
        refused += len(got["refused"])
        e1b += sum(s[0] == "S" and bool(s[2] & tc.E1B_MODE) for s in sc.steps)
        tc.assert_equal(got, tc.run_tool(exe, tc.without(sc, got["refused"]), tmp), sc.name)
    assert refused >= 1 and e1b >= 1, (refused, e1b)
