"""The receiver bank (kg_rxbank) with spectral noise reduction on some receivers (RxBank.set_nr(rx, post.NR_SPECTRAL, ...) ->
kg_post_nrs_select; RxBank.set_audio passes the cuts on to kg_post_nrs_passband): their mono16 rows and ADPCM payloads equal a
standalone kg_post with the same settings (+ the ADPCM coder) fed the bank's own CFastFIR output rows; IQ and SAS receivers skip
the stage; the other receivers' rows are byte-identical to a bank run without any NR call."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Post, post, wire

pytestmark = pytest.mark.gpu

N = 1 << 22
STEPS = 3
LO, HI = -4900.0, 4900.0
SPEC = post.NR_SPECTRAL
# receiver -> (mode, NR algo, params {type: [...]}, enables (denoise, auto-notch)) -- None: no NR call
PLAN = {0: (post.MODE_SSB, SPEC, {0: [1, 0.95, 1000]}, (0, 0)),
        1: (post.MODE_AM, SPEC, {1: [2, 0.9, 100]}, (0, 0)),
        2: (post.MODE_SSB, None, None, None),
        3: (post.MODE_IQ, SPEC, {0: [1, 0.95, 1000]}, (0, 0)),
        4: (post.MODE_SAM, SPEC, {0: [1, 0.99, 30]}, (0, 0)),
        5: (post.MODE_AM, None, None, None),
        6: (post.MODE_SSB, post.NR_WDSP, {0: [64, 16, 1e-4, 0.1]}, (1, 0)),
        7: (post.MODE_SAS, SPEC, {1: [1, 0.95, 1000]}, (0, 0))}
NRX = len(PLAN)


def _run(with_nr):
    from flydog_sdr_gps_amd import synth
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NRX, 0, N)
    bank = RxBank(NRX, N)
    rows = {rx: [] for rx in range(NRX)}
    try:
        bank.configure(mix)
        for rx, (mode, algo, params, en) in PLAN.items():
            bank.set_audio(rx, mix[rx][2], LO, HI, mode=mode)
            if with_nr and algo is not None:
                bank.set_nr(rx, algo, params, en)
        adc = synth.adc_stream(N, 0x5EED0053)
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
        states = bank.post.nrs_state(live)
        bank.ctx.free(d_adc)
        return rows, bank.fs, states
    finally:
        bank.close()


def test_spectral_nr_receivers_in_the_bank(gpu_ctx):
    rows, fs, states = _run(True)
    plain, _, _ = _run(False)
    nominal = 12000 if abs(fs - 12000.0) < abs(fs - 20250.0) else 20250
    fmax = int(fs / 2 - 1)                              # the handler clamps the cuts first (rx_sound_cmd.cpp:248-250), as set_audio does
    lo, hi = max(LO, float(-fmax)), min(HI, float(fmax))
    nblk = 0
    for rx, (mode, algo, params, en) in PLAN.items():
        assert len(rows[rx]) >= 2 and len(rows[rx]) == len(plain[rx]), rx
        if algo != SPEC or mode in post.STEREO_MODES:
            if algo == post.NR_WDSP:
                assert any(not np.array_equal(a["s16"], b["s16"]) for a, b in zip(rows[rx], plain[rx])), rx
                continue
            for a, b in zip(rows[rx], plain[rx]):
                key = "iq_pay" if mode in post.STEREO_MODES else "pay"
                assert np.array_equal(a[key], b[key]) and np.array_equal(a["firo"].view(np.uint32), b["firo"].view(np.uint32)), (rx, key)
                if key == "pay":
                    assert np.array_equal(a["s16"], b["s16"]), rx
            if algo == SPEC:
                assert list(states["ints"][rx, :2]) == [1, 0], (rx, "a stereo receiver's spectral state advanced")
            continue
        P = Post(gpu_ctx, nchan=1)                      # what RxBank.set_audio + set_nr configure, standalone
        ad = wire.Adpcm(gpu_ctx, nchan=1)
        try:
            P.sam_setup(0, nominal)
            P.set_sam_mparam(0, 0)
            P.set_am_passband(0, LO, HI, fs)
            P.set_agc(0, True, False, -100, 50, 6, 1000, fs)
            P.set_smeter(0, fs)
            P.set_mode(0, mode)
            P.reset(0)
            P.nrs_setup(nominal)
            P.nrs_passband(0, lo, hi)
            P.nrs_select(0)
            for t, vals in params.items():
                for k, v in enumerate(vals):
                    P.set_nr_param(0, t, k, v)
            changed = 0
            for k, (r, q) in enumerate(zip(rows[rx], plain[rx])):
                s16, _, _ = P.process([0], r["firo"][None, :])
                assert np.array_equal(r["s16"], s16[0]), (rx, k, "mono16")
                want = np.asarray(ad.encode([0], s16)).reshape(-1)
                assert np.array_equal(r["pay"], want), (rx, k, "ADPCM")
                assert np.array_equal(r["firo"].view(np.uint32), q["firo"].view(np.uint32)), (rx, k)
                changed += not np.array_equal(r["s16"], q["s16"])
                nblk += 1
            assert changed == len(rows[rx]), (rx, changed)
            a, b = P.nrs_state([0]), states
            assert np.array_equal(a["ints"][0], b["ints"][rx]) and np.array_equal(a["scalars"][0].view(np.uint32), b["scalars"][rx].view(np.uint32)), rx
            assert np.array_equal(a["arrays"][0].view(np.uint32), b["arrays"][rx].view(np.uint32)), rx
            assert a["ints"][0, 0] >= 2 and (a["ints"][0, 0] == 3 or a["ints"][0, 1] == 2 * len(rows[rx])), rx
        finally:
            ad.close()
            P.close()
    assert nblk >= 6, nblk


def test_bank_refuses_spectral_on_a_passband_it_cannot_run_on(gpu_ctx):
    from flydog_sdr_gps_amd._lib import KiwiGpuError
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](2, 0, N)
    bank = RxBank(2, N)
    try:
        bank.configure(mix)
        bank.set_audio(0, mix[0][2], 0.0, 300.0)            # bins 1..13 at 12 kHz
        with pytest.raises(KiwiGpuError):
            bank.set_nr(0, SPEC, {0: [1, 0.95, 1000]})
        bank.set_audio(0, mix[0][2], 300.0, 2700.0)
        bank.set_nr(0, SPEC, {0: [1, 0.95, 1000]})
        assert list(bank.post.nrs_state([0])["ints"][0]) == [1, 0, 12, 116]
    finally:
        bank.close()
