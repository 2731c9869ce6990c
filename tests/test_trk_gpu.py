"""The tracking kernel (kg_trk) against the LITERAL clock-by-clock model (tools/trk_model.cpp): every epoch record, every GPS_CHAN
byte and every replica word EQUAL, on every scenario of tests/trk_common.py (C/A with taps, QZSS g2_init, E1B with polarity 0 / 1 /
2, the ends of the accepted code rate, a negative LO rate, pauses of 0 / 1 / 16367, a reset with half the channels masked, all-ones /
all-zeros / replica streams, 12 channels with distinct settings, other delay pairs, set_loop off, one call against pieces of 1 / 7 /
8191 / 100001 clocks cut inside a byte, at an ms0 and between ms0 and each delay, 130 E1B nav bits); a C/A scene with a mid-bit sign
flip; each refusal, with nothing changed; and end to end: the lock check's scene through kg_acq_*, kg_acq_chan_start and kg_trk_*,
equal to the model's run that passed the lock check on the CPU."""
import os
import subprocess

import numpy as np
import pytest

from flydog_sdr_gps_amd import KiwiGpuError, Searcher, handoff, trk
from . import trk_common as tc

pytestmark = pytest.mark.gpu

INVALID, STATE = -2, -5


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("trk_gpu")
    return tc.build(d, "trk_model"), d


@pytest.mark.parametrize("name", sorted(tc.scenarios()))
def test_kernel_equals_literal_model(gpu_ctx, model, name):
    """a command refused with KG_ERR_STATE (scenario refused_cmds: a code rate, a pause and a reset that would make a paused channel
    hold ms0 set) changes nothing: the bank processes on and equals the model run on the script without those commands"""
    exe, tmp = model
    sc = tc.scenarios()[name]
    got = tc.run_gpu(gpu_ctx, sc)
    assert got["refused"] == ([13, 15, 19] if name == "refused_cmds" else []), name
    tc.assert_equal(got, tc.run_tool(exe, tc.without(sc, got["refused"]), tmp), name)


def test_code_loop_leaving_the_range_stops_the_channel(gpu_ctx, model):
    """channel 0's own loop writes 2^27 - 1 at its second service: it stops there, its count says so in that call and in the next,
    kg_trk_get_chan and (after a command) the process call answer KG_ERR_STATE, channel 1 goes on equal to the model, and
    kg_trk_set_rate_cg starts channel 0 again"""
    exe, tmp = model
    sc = tc.fault_scenario()
    want = tc.run_tool(exe, sc, tmp)
    n1, n2, n3 = 4 * 32736, 2 * 32736, 6 * 32736
    t = trk.Tracker(gpu_ctx, 2)
    try:
        for s in sc.steps[:sc.steps.index(("R",))]:
            {"S": t.set_sat, "G": t.set_rate_cg, "L": t.set_rate_lo, "l": t.set_gain_lo, "g": t.set_gain_cg}[s[0]](*s[1:])
        t.sampler_reset()
        a = t.process(sc.bits, n1)
        assert t.stopped == [0] and len(a[0]) == 2 and int(a[0][1]["cg_rate"]) == tc.RATE_MIN - 1
        _raises(STATE, t.get_chan, 0)
        assert int(t.get_chan(1)["nav_ms"]) >= 0
        b = t.process(sc.bits[n1 // 8:], n2)                                    # no command between: the count still says it
        assert t.stopped == [0] and len(b[0]) == 0 and len(b[1]) > 0
        t.set_loop(1, 1)
        _raises(STATE, t.process, sc.bits[(n1 + n2) // 8:], n3)                 # after a command the call refuses, nothing consumed
        assert t.get_clocks()[0] == n1 + n2
        t.set_rate_cg(0, tc.NOM)
        c = t.process(sc.bits[(n1 + n2) // 8:], n3)
        assert t.stopped == [] and len(c[0]) >= 10 and int(t.get_chan(0)["nav_ms"]) >= 0
        got1 = [tc.record_tuple(e) for part in (a, b, c) for e in part[1]]
        assert got1 == want["records"][1]
    finally:
        t.close()


def test_pieces_equal_one_call(gpu_ctx):
    S = tc.scenarios()
    a, b = tc.run_gpu(gpu_ctx, S["one_call"]), tc.run_gpu(gpu_ctx, S["pieces"])
    assert a["records"] == b["records"] and a["dumps"][-1] == b["dumps"][-1]


def test_mid_bit_sign_flip_counts_a_glitch(gpu_ctx, model):
    """a C/A signal at 50 dB-Hz whose data sign flips in the middle of a bit (8000 clocks into epoch 110 of 160): Inav changes once
    after pull-in, and ch_NAV_GLITCH counts one more than on the same scene without the flip -- in the model, and equal on the GPU"""
    from flydog_sdr_gps_amd import prn, sats
    exe, tmp = model
    _, t1, t2, _ = sats.SATS[6]
    chips = prn.cacode(t1, t2)
    n = 160 * tc.CA_EPOCH
    lo, cg = trk.gains(False)
    steps = [("S", 0, trk.codegen_init(6)), ("G", 0, tc.NOM), ("L", 0, tc.LO_NOM), ("l", 0) + lo, ("g", 0) + cg, ("R",), ("X", n), ("D",)]
    runs = {}
    for name, flips in (("flip", (110 * tc.CA_EPOCH + 8000,)), ("noflip", ())):
        bits = trk.scene_bits(chips, n, 0.25, 0.0, 50.0, np.zeros(8, np.uint8), seed=31, flips=flips)
        sc = tc.Scenario(name, 1, steps, bits=bits)
        runs[name] = (sc, tc.run_tool(exe, sc, tmp))
    got = tc.run_gpu(gpu_ctx, runs["flip"][0])
    tc.assert_equal(got, runs["flip"][1], "flip")
    chan = lambda w: np.frombuffer(bytes.fromhex(w["dumps"][0][0][0]), trk.chan_dtype)[0]
    inav = (np.array(got["records"][0])[:, 9] >> 1) & 1
    change = np.flatnonzero(np.diff(inav[60:])) + 61
    assert change.size == 1 and 109 <= change[0] <= 113, change
    assert int(chan(got)["nav_glitch"]) == int(chan(runs["noflip"][1])["nav_glitch"]) + 1


def _raises(status, fn, *a):
    with pytest.raises(KiwiGpuError) as e:
        fn(*a)
    assert e.value.status == status, (e.value.status, str(e.value))


def test_refusals_change_nothing(gpu_ctx, model):
    exe, tmp = model
    for bad in ((0, 0, 0), (13, 0, 0), (1, 1, 577), (1, 216, 8184), (1, 300, 299), (1, -5, 577)):
        _raises(INVALID, trk.Tracker, gpu_ctx, *bad)
    sc = tc.scenarios()["neg_lo"]
    one = np.zeros(4, np.uint8)

    class Pestered(trk.Tracker):
        """every process call is preceded by one refusal of each kind"""
        def process(self, bits, nclocks):
            before = [self.get_chan(ch).tobytes() for ch in range(self.nchan)], self.get_clocks()[1].tolist()
            _raises(INVALID, self.set_rate_cg, 0, (1 << 27) - 1)
            _raises(INVALID, self.set_rate_cg, 0, 1 << 29)
            _raises(INVALID, self.set_rate_cg, 1, tc.NOM)                       # no such channel
            _raises(INVALID, self.set_sat, 0, 0x1000)
            _raises(INVALID, self.set_sat, 0, (11 << 4) + 3)                    # a tap outside g2[10:1]
            _raises(INVALID, self.set_sat, 0, 5)
            _raises(INVALID, self.set_e1b_code, 0, np.zeros(4091, np.uint8))
            _raises(INVALID, self.set_e1b_code, 0, np.full(4092, 2, np.uint8))
            _raises(INVALID, self.set_gain_lo, 0, 64, 0)
            _raises(INVALID, self.set_gain_cg, 0, 0, -1)
            _raises(INVALID, self.set_polarity, 0, 3)
            _raises(INVALID, self.pause, 0, 65536)
            _raises(INVALID, super().process, one, 0)
            ep = np.zeros((1, 4), trk.epoch_dtype)
            cnt = np.zeros(1, np.int32)
            n = 3 * 8184
            _raises(INVALID, lambda: trk.check(self.lib.kg_trk_process_bits(self.h, trk.ptr(np.zeros(n // 8 + 2, np.uint8)), n, trk.ptr(ep), 4, 4,
                                                                           trk.ptr(cnt)), "kg_trk_process_bits"))      # cap 4 < 3 + 2
            after = [self.get_chan(ch).tobytes() for ch in range(self.nchan)], self.get_clocks()[1].tolist()
            assert before == after
            return super().process(bits, nclocks)

    tc.assert_equal(tc.run_gpu(gpu_ctx, sc, Pestered), tc.run_tool(exe, sc, tmp), "neg_lo with refusals between")

    # a channel run before set_sat, before its reset, in E1B mode without a code, without a code rate
    t = trk.Tracker(gpu_ctx, 2)
    try:
        bits = np.zeros(64, np.uint8)
        t.set_sat(0, tc.CA1); t.set_rate_cg(0, tc.NOM); t.sampler_reset()
        _raises(INVALID, t.process, bits, 100)                                  # channel 1 has no satellite
        t.set_sat(1, tc.E1)
        _raises(INVALID, t.process, bits, 100)                                  # not reset since
        t.sampler_reset()
        _raises(INVALID, t.process, bits, 100)                                  # E1B without a code
        t.set_e1b_code(1, tc.e1b_code(1))
        _raises(INVALID, t.process, bits, 100)                                  # channel 1 has no code rate
        t.set_rate_cg(1, tc.NOM)
        assert t.get_clocks()[0] == 0
        t.process(bits, 10)                                                     # ms0 was set by edge 7, nchip is still 0, the service is due
        _raises(STATE, t.pause, 0, 100)                                         # refused at the command, nothing changed ...
        t.process(bits[1:], 100)                                                # ... so the bank runs on (equality: scenario refused_cmds)
        assert t.get_clocks()[0] == 110
    finally:
        t.close()


def test_end_to_end_acquire_start_track(gpu_ctx, model, oracle):
    exe, tmp = model
    chips, bits = tc.lock_bits()
    s = Searcher(gpu_ctx)
    try:
        s.set_code(0, chips)
        out = s.search([0], packed=bits[:8192])[0]
    finally:
        s.close()
    want, _ = oracle.correlate(oracle.code_fft(chips), oracle.sample_bits(bits[:8192]))
    assert (out.lo_shift, out.ca_shift) == (want["dop"], want["idx"] * handoff.DECIM)
    start = handoff.chan_start(0, out.lo_shift, out.ca_shift, tc.LOCK_T0 / trk.FS)
    sc = tc.lock_scenario(bits, start)
    ref = tc.run_tool(exe, sc, tmp)
    got = tc.run_gpu(gpu_ctx, sc)
    tc.assert_equal(got, ref, "lock scene")
    r = np.array(got["records"][0])
    assert len(r) >= tc.LOCK_MS - 6 and (r[-200:, 9] & trk.UNLOCKED).sum() == 0


def test_track_dropin_example(gpu_ctx, model, tmp_path):
    """examples/track_dropin.cpp (include/kiwigpu.h only) on the lock check's scene: the acquisition line, and the GPS_CHAN it
    uploads at the end, are those of the model's run"""
    exe, tmp = model
    drop = os.path.join(tc.ROOT, "examples", "track_dropin")
    assert os.path.exists(drop), "examples/track_dropin is not built (run __graft_entry__.build())"
    chips, bits = tc.lock_bits()
    path = str(tmp_path / "scene.bits")
    bits[:tc.LOCK_MS * tc.CA_EPOCH // 8].tofile(path)
    p = subprocess.run([drop, path, "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    lines = [l.split() for l in p.stdout.decode().splitlines()]
    acq, last = lines[0], lines[-1]
    start = handoff.chan_start(0, int(acq[4]), int(acq[6]), tc.LOCK_T0 / trk.FS)
    assert (int(acq[8], 16), int(acq[10], 16), int(acq[12])) == (start.lo_rate, start.ca_rate, start.ca_pause)
    ref = tc.run_tool(exe, tc.lock_scenario(bits, start), tmp)
    ch = np.frombuffer(bytes.fromhex(ref["dumps"][0][0][0]), trk.chan_dtype)[0]
    assert (int(last[1]), int(last[3]), int(last[5])) == (int(ch["nav_bits"]), int(ch["nav_glitch"]), 0)
    assert abs(float(last[7]) - tc.LOCK_DOPPLER) < 30
