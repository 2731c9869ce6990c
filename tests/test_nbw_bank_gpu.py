"""The receiver bank (kg_rxbank) with the Wild noise blanker on some receivers (RxBank.set_nb(rx, nb.NB_WILD, ...) ->
kg_rxbank_nbw_select, kg_rxbank_set_nb_param -> kg_post_nbw_init, kg_rxbank_set_nb_enable -> kg_post_set_nbw): their mono16 rows and
ADPCM payloads equal a standalone kg_post with the same settings (+ the ADPCM coder) fed the bank's own CFastFIR output rows; an IQ
receiver skips the stage; the other receivers' rows are byte-identical to a bank run without any NB call; and the command-state
transitions: select, the three parameter messages, enable, the legacy gate command, another algo, join."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Post, nb, post, wire

pytestmark = pytest.mark.gpu

N = 1 << 22
STEPS = 3
LO, HI = -4900.0, 4900.0
# receiver -> (mode, Wild vector or None, NR on top)
PLAN = {0: (post.MODE_SSB, [0.95, 10, 7], None),
        1: (post.MODE_AM, [0.95, 40, 41], None),
        2: (post.MODE_SSB, None, None),
        3: (post.MODE_IQ, [0.95, 10, 7], None),
        4: (post.MODE_SAM, [1.5, 16, 12], None),
        5: (post.MODE_SSB, [0.95, 10, 7], (post.NR_WDSP, {0: [64, 16, 1e-4, 0.1]}, (1, 0)))}
NRX = len(PLAN)


def _run(with_nb):
    from flydog_sdr_gps_amd import synth
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NRX, 0, N)
    bank = RxBank(NRX, N)
    rows = {rx: [] for rx in range(NRX)}
    try:
        bank.configure(mix)
        for rx, (mode, vec, nr) in PLAN.items():
            bank.set_audio(rx, mix[rx][2], LO, HI, mode=mode)
            if nr is not None:
                bank.set_nr(rx, *nr)
            if with_nb and vec is not None:
                bank.set_nb(rx, nb.NB_WILD, vec, (1, 0))
        adc = synth.adc_stream(N, 0x5EED0057)
        d_adc = bank.ctx.alloc(adc.nbytes)
        bank.ctx.upload(d_adc, adc)
        live = list(range(NRX))
        for step in range(STEPS):
            bank.step(d_adc)
            bank.sync()
            _, nfir, _, _ = bank.audio_map()
            g = {k: bank.fetch(k, live) for k in ("firo", "s16", "pay", "iq_pay")}
            for rx in live:
                for blk in range(int(nfir[rx]) // 512):
                    sl = slice(512 * blk, 512 * (blk + 1))
                    rows[rx].append({"firo": np.ascontiguousarray(g["firo"][rx, sl]).view(np.complex64).ravel(), "s16": g["s16"][rx, sl].copy(),
                                     "pay": g["pay"][rx, 256 * blk:256 * (blk + 1)].copy(),
                                     "iq_pay": g["iq_pay"][rx, 2048 * blk:2048 * (blk + 1)].copy()})
        states = bank.post.nbw_state(live)
        cmd = [bank.nb_cmd_state(rx) for rx in live]
        bank.ctx.free(d_adc)
        return rows, bank.fs, states, cmd
    finally:
        bank.close()


def test_wild_blanker_receivers_in_the_bank(gpu_ctx):
    rows, fs, states, cmd = _run(True)
    plain, _, pstates, _ = _run(False)
    nominal = 12000 if abs(fs - 12000.0) < abs(fs - 20250.0) else 20250
    nblk = 0
    for rx, (mode, vec, nr) in PLAN.items():
        assert len(rows[rx]) >= 2 and len(rows[rx]) == len(plain[rx]), rx
        ints, flts = cmd[rx]
        if vec is None:
            assert not ints.any() and not pstates["hist"][rx].any()
        else:
            assert ints[0] == nb.NB_WILD and list(ints[1:9]) == [1, 0, 0, 0, 1, 0, 0, 0] and not ints[9:].any(), (rx, ints)
            assert flts[0, 0, :3].tolist() == [np.float32(v) for v in vec] and not flts[1].any(), (rx, "nothing goes to the waterfall side")
        if vec is None or mode in post.STEREO_MODES:
            for a, b in zip(rows[rx], plain[rx]):
                key = "iq_pay" if mode in post.STEREO_MODES else "pay"
                assert np.array_equal(a[key], b[key]) and np.array_equal(a["firo"].view(np.uint32), b["firo"].view(np.uint32)), (rx, key)
                if key == "pay":
                    assert np.array_equal(a["s16"], b["s16"]), rx
            assert not states["hist"][rx].any(), (rx, "the state of a receiver that does not run the stage advanced")
            continue
        P = Post(gpu_ctx, nchan=1)                      # what RxBank.set_audio + set_nr + set_nb configure, standalone
        ad = wire.Adpcm(gpu_ctx, nchan=1)
        try:
            P.sam_setup(0, nominal)
            P.set_sam_mparam(0, 0)
            P.set_am_passband(0, LO, HI, fs)
            P.set_agc(0, True, False, -100, 50, 6, 1000, fs)
            P.set_smeter(0, fs)
            P.set_mode(0, mode)
            P.reset(0)
            if nr is not None:
                P.set_nr_algo(0, nr[0])
                for t, vals in nr[1].items():
                    for k, v in enumerate(vals):
                        P.set_nr_param(0, t, k, v)
                for t in (0, 1):
                    if nr[2][t]:
                        P.set_nr_enable(0, t, nr[2][t])
            for k in range(3):                          # the three messages, each an nb_Wild_init from the vector so far
                P.nbw_init(0, vec[:k + 1])
            P.set_nbw(0, 1)
            changed = 0
            for k, (r, q) in enumerate(zip(rows[rx], plain[rx])):
                s16, _, _ = P.process([0], r["firo"][None, :])
                assert np.array_equal(r["s16"], s16[0]), (rx, k, "mono16")
                want = np.asarray(ad.encode([0], s16)).reshape(-1)
                assert np.array_equal(r["pay"], want), (rx, k, "ADPCM")
                assert np.array_equal(r["firo"].view(np.uint32), q["firo"].view(np.uint32)), (rx, k)
                changed += not np.array_equal(r["s16"], q["s16"])
                nblk += 1
            assert changed == len(rows[rx]), (rx, changed)          # at least the delay of order + PL
            a = P.nbw_state([0])
            assert np.array_equal(a["ints"][0], states["ints"][rx]) and a["ints"][0].tolist() == [int(vec[1]), int(vec[2]), 1], rx
            assert np.array_equal(a["hist"][0].view(np.uint32), states["hist"][rx].view(np.uint32)) and a["hist"].any(), rx
        finally:
            ad.close()
            P.close()
    assert nblk >= 8, nblk


def test_bank_command_state_transitions(gpu_ctx):
    from flydog_sdr_gps_amd import synth
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](2, 0, N)
    bank = RxBank(2, N)
    try:
        bank.configure(mix)
        for rx in range(2):
            bank.set_audio(rx, mix[rx][2], LO, HI)
        L, h, fr = bank.lib, bank.h, float(np.float32(bank.fs))
        st = lambda rx=0: bank.nb_cmd_state(rx)
        sw = lambda rx=0: bank.post.nbw_state([rx])["ints"][0].tolist()
        assert L.kg_rxbank_set_nb_algo(h, 0, nb.NB_WILD) == -2                       # that entry point keeps its refusal
        assert st()[0][0] == nb.NB_OFF
        assert L.kg_rxbank_nbw_select(h, 2) == -2 and L.kg_rxbank_nbw_select(h, -1) == -2
        # enables set under another algo are cleared by the select, on both sides; no state is touched
        bank.set_nb(0, nb.NB_STD, [100.0, 50.0], (1, 1))
        assert list(st()[0][:9]) == [nb.NB_STD, 1, 1, 0, 0, 1, 1, 0, 0]
        s_std = bank.nb.state(0)
        assert L.kg_rxbank_nbw_select(h, 0) == 0
        ints, flts = st()
        assert ints[0] == nb.NB_WILD and not ints[1:9].any() and sw() == [0, 0, 0]
        assert all(np.array_equal(x, y) for x, y in zip(bank.nb.state(0), s_std))
        wf_before, pending_before = flts[1].copy(), ints[9:].copy()
        # enabling before a usable vector exists: refused, nothing changed
        assert L.kg_rxbank_set_nb_enable(h, 0, nb.NB_BLANKER, 1) == -5
        assert not st()[0][1:9].any()
        # the three messages: each stores its value and runs nb_Wild_init from the whole stored vector (gate 100 / threshold 50 of
        # the NB_STD time are still in it); nothing goes to the waterfall side
        assert L.kg_rxbank_set_nb_param(h, 0, nb.NB_BLANKER, post.NB_THRESH, 0.95, fr) == 0
        assert sw() == [50, 0, 0] and bank.post.nbw_state([0])["thresh"][0] == np.float32(0.95)
        assert L.kg_rxbank_set_nb_enable(h, 0, nb.NB_BLANKER, 1) == -5               # taps 50: outside the arrays
        assert L.kg_rxbank_set_nb_param(h, 0, nb.NB_BLANKER, post.NB_TAPS, 10.0, fr) == 0
        assert sw() == [10, 0, 0]
        assert L.kg_rxbank_set_nb_param(h, 0, nb.NB_BLANKER, post.NB_SAMPLES, 7.0, fr) == 0
        assert sw() == [10, 7, 0]
        ints, flts = st()
        assert flts[0, 0, :3].tolist() == [np.float32(0.95), 10.0, 7.0] and np.array_equal(flts[1], wf_before) and np.array_equal(ints[9:], pending_before)
        # a parameter of another type is stored and initialises nothing
        assert L.kg_rxbank_set_nb_param(h, 0, nb.NB_WF, 0, 3.0, fr) == 0 and sw() == [10, 7, 0]
        # the enable drives the stage's switch; NB_WF's does not
        assert L.kg_rxbank_set_nb_enable(h, 0, nb.NB_WF, 1) == 0 and sw() == [10, 7, 0]
        assert L.kg_rxbank_set_nb_enable(h, 0, nb.NB_BLANKER, 1) == 0 and sw() == [10, 7, 1]
        assert list(st()[0][:9]) == [nb.NB_WILD, 1, 1, 0, 0, 1, 1, 0, 0]
        # with the stage on, a message that would make the vector unusable is refused and nothing changes
        assert L.kg_rxbank_set_nb_param(h, 0, nb.NB_BLANKER, post.NB_TAPS, 0.0, fr) == -2
        assert sw() == [10, 7, 1] and st()[1][0, 0, 1] == 10.0
        adc = synth.adc_stream(N, 0x5EED0058)
        d_adc = bank.ctx.alloc(adc.nbytes)
        bank.ctx.upload(d_adc, adc)

        def step_block():
            """steps until receiver 0 completes a 512-sample sound block, so that the stage had a block to run on (a step of N ADC
            samples brings fewer than 512 audio samples, and the first block completes in the second step)"""
            for _ in range(3):
                bank.step(d_adc)
                bank.sync()
                if bank.audio_map()[1][0] >= 512:
                    return
            raise AssertionError("no sound block in three steps")

        step_block()
        h1 =bank.post.nbw_state([0])["hist"][0].copy()
        assert h1[:26].any() and not bank.post.nbw_state([1])["hist"].any()
        assert all(np.array_equal(x, y) for x, y in zip(bank.nb.state(0), s_std)), "the NB_STD audio blanker ran under NB_WILD"
        # the legacy gate command: stored values and the enable only, never nb_Wild_init
        bank.set_nb_gate(0, 0, 40)
        assert sw() == [10, 7, 0] and st()[0][1] == 0 and st()[1][0, 0, :3].tolist() == [0.0, 40.0, 7.0]
        assert np.array_equal(bank.post.nbw_state([0])["hist"][0].view(np.uint32), h1.view(np.uint32))
        step_block()                                                                # off: the state stays
        assert np.array_equal(bank.post.nbw_state([0])["hist"][0].view(np.uint32), h1.view(np.uint32))
        bank.set_nb_gate(0, 100, 40)
        assert sw() == [10, 7, 1] and st()[0][1] == 1                               # on again with the vector of the last init
        assert np.array_equal(bank.post.nbw_state([0])["hist"][0].view(np.uint32), h1.view(np.uint32))
        step_block()
        h2 =bank.post.nbw_state([0])["hist"][0].copy()
        assert not np.array_equal(h2.view(np.uint32), h1.view(np.uint32))
        # another algo: the enables cleared, the stage off, its state kept
        assert L.kg_rxbank_set_nb_algo(h, 0, nb.NB_STD) == 0
        assert sw() == [10, 7, 0] and not st()[0][1:9].any() and st()[0][0] == nb.NB_STD
        assert L.kg_rxbank_set_nb_enable(h, 0, nb.NB_BLANKER, 1) == 0 and sw() == [10, 7, 0]      # NB_STD's enable is not the Wild switch
        # back, on, then a new connection: join clears the command state and the switch, the Wild state stays
        assert L.kg_rxbank_nbw_select(h, 0) == 0
        assert L.kg_rxbank_set_nb_enable(h, 0, nb.NB_BLANKER, 1) == 0 and sw() == [10, 7, 1]
        bank.join(0, (mix[0][0], mix[0][1]), mix[0][2], lo=LO, hi=HI)
        ints, flts = st()
        assert not ints.any() and not flts.any() and sw() == [10, 7, 0]
        assert np.array_equal(bank.post.nbw_state([0])["hist"][0].view(np.uint32), h2.view(np.uint32))
        step_block()
        assert np.array_equal(bank.post.nbw_state([0])["hist"][0].view(np.uint32), h2.view(np.uint32))
        bank.ctx.free(d_adc)
    finally:
        bank.close()
