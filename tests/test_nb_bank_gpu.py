"""The receiver bank (kg_rxbank) with the standard noise blanker (RxBank.set_nb / set_nb_gate -> kg_rxbank_set_nb_*): the blanked
receivers' CFastFIR input and output equal a standalone kg_nb -> kg_fir pipeline fed the bank's own unpacked records, their
waterfall rows equal a standalone kg_wf with the blanker fed the bank's frames in order; every other receiver's rows, payloads and
CFastFIR output are byte-identical to a bank run without any NB call.  The command layer's coupling (deferred setup, zoom change,
join) and its refusals."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import FastFir, KiwiGpuError, NoiseBlanker, Waterfall, nb, synth, wf

pytestmark = pytest.mark.gpu

N = 1 << 22
STEPS = 3
NRX = 8
# receiver -> ("set", algo, params, (blanker, wf)) or ("gate", nb, th) after `SET nb algo=1`; None: no NB call
PLAN = {0: ("set", nb.NB_STD, [100.0, 50.0], (1, 1)),         # audio + waterfall
        1: ("set", nb.NB_STD, [300.0, 20.0], (1, 0)),         # audio only: the waterfall needs NB_WF too
        2: None,
        3: ("set", nb.NB_STD, [2000.0, 60.0], (1, 1)),
        4: ("set", nb.NB_OFF, [100.0, 50.0], (1, 1)),         # NB_OFF: no setup, params never reach the waterfall, nothing runs
        5: ("gate", 150, 30),                                 # legacy `SET nb= th=` under NB_STD: audio only
        6: None,
        7: ("set", nb.NB_STD, [100.0, 50.0], (0, 1))}         # NB_WF alone: nothing runs
AUDIO_ON = {0, 1, 3, 5}
WF_ON = {0, 3}


def adc():
    x = synth.adc_stream(N, 0x5EED0077).astype(np.float64)
    t = np.arange(N)
    for s in range(40000, N, 700001):                         # strong bursts at the audio NCOs' frequency: impulse noise
        x[s:s + 20000] += 26000.0 * np.sin(2 * np.pi * 0.0123 * t[s:s + 20000])
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _configure(bank, with_nb):
    from flydog_sdr_gps_amd.rxbank import MIXES
    mix = MIXES["light"](NRX, 0, N)
    bank.configure(mix)
    for rx in range(NRX):
        bank.set_audio(rx, mix[rx][2], -4900.0, 4900.0)
        p = PLAN[rx]
        if not with_nb or p is None:
            continue
        if p[0] == "set":
            bank.set_nb(rx, p[1], p[2], p[3])
        else:
            bank.set_nb(rx, nb.NB_STD)
            bank.set_nb_gate(rx, p[1], p[2])
    return mix


def _run(with_nb):
    from flydog_sdr_gps_amd.rxbank import RxBank
    bank = RxBank(NRX, N)
    out = []
    try:
        mix = _configure(bank, with_nb)
        a = adc()
        d_adc = bank.ctx.alloc(a.nbytes)
        bank.ctx.upload(d_adc, a)
        live = list(range(NRX))
        for step in range(STEPS):
            bank.step(d_adc)
            bank.sync()
            nrec, nfir, _, _ = bank.audio_map()
            rx_of, off, _ = bank.frame_map()
            g = {k: bank.fetch(k, live) for k in ("xin", "firo", "pay", "rows", "wf_iq")}
            frames = {}
            for f, (r, o) in enumerate(zip(rx_of, off)):
                o = int(o) - int(r) * bank.bufs.wf_iq_stride
                frames[int(r)] = (g["rows"][r].copy(), g["wf_iq"][r, o:o + 8192].copy())
            out.append({"nrec": nrec.copy(), "nfir": nfir.copy(), "xin": g["xin"].copy(), "firo": g["firo"].copy(), "pay": g["pay"].copy(),
                        "frames": frames})
        bank.ctx.free(d_adc)
        return out, bank.fs, mix
    finally:
        bank.close()


def test_nb_receivers_in_the_bank(gpu_ctx):
    got, fs, mix = _run(True)
    plain, _, _ = _run(False)
    for rx in range(NRX):
        a_changed = w_changed = 0
        if rx in AUDIO_ON:
            p = PLAN[rx]
            prm = p[2] if p[0] == "set" else [p[1], p[2]]
            B = NoiseBlanker(gpu_ctx, nchan=1, max_in=1 << 16)
            F = FastFir(gpu_ctx, nchan=1, max_in=1 << 16)
            try:
                B.setup(0, np.float32(fs), prm)
                fmax = int(fs / 2 - 1)                    # RxBank.set_audio's clamp of the cuts (rx_sound_cmd.cpp:248-250)
                assert F.setup(0, max(-4900.0, float(-fmax)), min(4900.0, float(fmax)), 0.0, fs)
                for s in range(STEPS):
                    n = int(got[s]["nrec"][rx])
                    assert n == int(plain[s]["nrec"][rx]) and n > 0
                    want = B.process(0, plain[s]["xin"][rx, :n])
                    assert np.array_equal(got[s]["xin"][rx, :n].view(np.uint32), want.view(np.uint32)), (rx, s, "rx_in")
                    a_changed += not np.array_equal(got[s]["xin"][rx, :n], plain[s]["xin"][rx, :n])
                    fo = F.process(0, np.ascontiguousarray(want).view(np.complex64).ravel())
                    nf = int(got[s]["nfir"][rx])
                    assert nf == len(fo), (rx, s)
                    assert np.array_equal(got[s]["firo"][rx, :nf].view(np.uint32), fo.view(np.float32).reshape(-1, 2).view(np.uint32)), (rx, s)
            finally:
                F.close()
                B.close()
            assert a_changed == STEPS, rx
        else:
            for s in range(STEPS):                      # (what the step wrote: a row's tail beyond the counts is never written)
                n, nf = int(got[s]["nrec"][rx]), int(got[s]["nfir"][rx])
                assert (n, nf) == (int(plain[s]["nrec"][rx]), int(plain[s]["nfir"][rx]))
                for k, m in (("xin", n), ("firo", nf), ("pay", nf // 2)):
                    assert np.array_equal(got[s][k][rx, :m].view(np.uint8), plain[s][k][rx, :m].view(np.uint8)), (rx, s, k)
        if rx in WF_ON:
            W = Waterfall(gpu_ctx, nchan=1)
            try:
                W.set_tables()
                W.set_channel(0, mix[rx][0], interp=wf.WF_MAX, window_func=wf.WINF_HANNING, cic_comp=True, overlapped=mix[rx][1])
                W.nb_setup(0, PLAN[rx][2])
                W.set_nb(0, True)
                for s in range(STEPS):
                    row, iq = got[s]["frames"][rx]
                    assert np.array_equal(iq, plain[s]["frames"][rx][1]), (rx, s, "wf_iq")
                    assert np.array_equal(row, W.frames([0], iq[None])[0]), (rx, s, "row")
                    w_changed += not np.array_equal(row, plain[s]["frames"][rx][0])
            finally:
                W.close()
            assert w_changed >= 1, rx
        else:
            for s in range(STEPS):
                assert np.array_equal(got[s]["frames"][rx][0], plain[s]["frames"][rx][0]), (rx, s, "row")


def test_bank_command_coupling_zoom_and_join(gpu_ctx):
    from flydog_sdr_gps_amd.rxbank import RxBank, MIXES
    bank = RxBank(2, N)
    try:
        mix = MIXES["light"](2, 0, N)
        bank.configure(mix)
        for rx in range(2):
            bank.set_audio(rx, mix[rx][2], -4900.0, 4900.0)
        a = adc()
        d_adc = bank.ctx.alloc(a.nbytes)
        bank.ctx.upload(d_adc, a)
        st = lambda: bank.nb_cmd_state(0)[0]
        # refusals at the command, nothing changed
        for fn, args, code in [(bank.lib.kg_rxbank_set_nb_algo, (0, nb.NB_WILD), -2), (bank.lib.kg_rxbank_set_nb_algo, (0, 3), -2),
                               (bank.lib.kg_rxbank_set_nb_enable, (0, nb.NB_CLICK, 1), -2), (bank.lib.kg_rxbank_set_nb_enable, (0, 4, 1), -2),
                               (bank.lib.kg_rxbank_set_nb_param, (0, 4, 0, 1.0, 12000.0), -2),
                               (bank.lib.kg_rxbank_set_nb_param, (0, 0, 8, 1.0, 12000.0), -2)]:
            assert fn(bank.h, *args) == code, (fn, args)
        assert bank.lib.kg_rxbank_set_nb_algo(bank.h, 0, nb.NB_STD) == 0
        assert bank.lib.kg_rxbank_set_nb_enable(bank.h, 0, nb.NB_BLANKER, 1) == -5          # never set up
        assert bank.lib.kg_rxbank_set_nb_param(bank.h, 0, 0, 0, 1e30, float(bank.fs)) == -2  # gate outside int
        assert list(st()) == [nb.NB_STD] + [0] * 13
        # params under NB_OFF stay on the audio side; `SET nb algo=` clears both sides' enables
        bank.set_nb(1, nb.NB_OFF, [100.0, 50.0], (1, 1))
        i1, f1 = bank.nb_cmd_state(1)
        assert list(i1[1:9]) == [1, 1, 0, 0, 1, 1, 0, 0] and not i1[9:].any() and f1[0, 0, :2].tolist() == [100.0, 50.0] and not f1[1].any()
        bank.set_nb(1, nb.NB_STD)
        assert not bank.nb_cmd_state(1)[0][1:9].any()
        # the waterfall's setup waits for both enables and happens before the next frame
        bank.set_nb(0, nb.NB_STD, [100.0, 50.0], (1, 0))
        assert list(st()[9:]) == [1, 0, 0, 0, 0]                      # change pending, no setup
        bank.step(d_adc); bank.sync()
        assert list(st()[9:]) == [1, 0, 0, 0, 0]
        bank.set_nb(0, nb.NB_STD, [100.0, 50.0], (1, 1))
        bank.step(d_adc); bank.sync()
        assert list(st()[9:]) == [0, 0, 0, 0, 1]
        s_before = bank.wf.nb_state(0)
        # a param change with NB_WF off: deferred, the blanker untouched by the steps
        bank.lib.kg_rxbank_set_nb_enable(bank.h, 0, nb.NB_WF, 0)
        bank.lib.kg_rxbank_set_nb_param(bank.h, 0, 0, 1, 70.0, float(bank.fs))
        bank.step(d_adc); bank.sync()
        assert all(np.array_equal(x, y) for x, y in zip(bank.wf.nb_state(0), s_before))
        assert list(st()[9:]) == [1, 0, 0, 0, 1]
        bank.lib.kg_rxbank_set_nb_enable(bank.h, 0, nb.NB_WF, 1)
        bank.step(d_adc); bank.sync()
        assert list(st()[9:]) == [0, 0, 0, 0, 1]
        # a zoom change with both on: the blanker is set up again before the next frame -- its state after that frame equals a fresh
        # blanker's after the same frame
        p2 = wf.WfParams.for_zoom(mix[0][0].zoom + 1, mix[0][0].start)
        bank.set_wf(0, p2, mix[0][1])
        assert st()[9] == 1
        bank.step(d_adc); bank.sync()
        assert st()[9] == 0
        rx_of, off, _ = bank.frame_map()
        f = list(rx_of).index(0)
        iq = bank.fetch("wf_iq", [0])[0, int(off[f]):int(off[f]) + 8192]
        W = Waterfall(gpu_ctx, nchan=1)
        d_iq, d_o = gpu_ctx.alloc(iq.nbytes), gpu_ctx.alloc(8192 * 8)
        try:
            W.set_tables()
            W.set_channel(0, p2)
            W.nb_setup(0, [100.0, 70.0])
            gpu_ctx.upload(d_iq, np.ascontiguousarray(iq))
            W.nb_frames([0], d_iq, d_o, [0], 8192)
            want = W.nb_state(0)
        finally:
            gpu_ctx.free(d_iq); gpu_ctx.free(d_o)
            W.close()
        got = bank.wf.nb_state(0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        # join: the command state of both sides cleared, the blankers' states kept
        s_audio = bank.nb.state(0)
        bank.join(0, (p2, mix[0][1]), mix[0][2], lo=-4900.0, hi=4900.0)
        ints, flts = bank.nb_cmd_state(0)
        assert not ints.any() and not flts.any()
        assert all(np.array_equal(x, y) for x, y in zip(bank.wf.nb_state(0), got))
        assert all(np.array_equal(x, y) for x, y in zip(bank.nb.state(0), s_audio))
        bank.step(d_adc); bank.sync()                                   # nothing blanked any more: both states stay
        assert all(np.array_equal(x, y) for x, y in zip(bank.nb.state(0), s_audio))
        bank.ctx.free(d_adc)
    finally:
        bank.close()
