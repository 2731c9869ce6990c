"""The receiver bank (kg_rxbank) with noise reduction on some receivers (RxBank.set_nr -> kg_post_set_nr_*): their mono16 rows
and ADPCM payloads equal a standalone kg_post with the same NR settings (+ the ADPCM coder) fed the bank's own CFastFIR output rows;
the other receivers' rows are byte-identical to a bank run without any NR call."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Post, post, wire

pytestmark = pytest.mark.gpu

N = 1 << 22
STEPS = 3
# receiver -> (mode, NR algo, params {type: [...]}, enables (denoise, auto-notch)) -- None: no NR call
PLAN = {0: (post.MODE_SSB, post.NR_WDSP, {1: [64, 16, 1e-4, 0.1], 0: [64, 16, 1e-4, 0.1]}, (1, 1)),
        1: (post.MODE_AM, post.NR_ORIG, {0: [0, 0, 0], 1: [0, 0, 0]}, (1, 1)),
        2: (post.MODE_SSB, None, None, None),
        3: (post.MODE_IQ, post.NR_WDSP, {0: [64, 16, 1e-4, 0.1]}, (1, 0)),
        4: (post.MODE_SAM, post.NR_WDSP, {1: [128, 2, 2.048e-4, 0.2]}, (0, 1)),
        5: (post.MODE_AM, None, None, None),
        6: (post.MODE_SSB, post.NR_ORIG, {0: [20, 0.01, 0.97]}, (1, 0)),
        7: (post.MODE_SAS, post.NR_ORIG, {1: [0, 0, 0]}, (0, 1))}
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
            bank.set_audio(rx, mix[rx][2], -4900.0, 4900.0, mode=mode)
            if with_nr and algo is not None:
                bank.set_nr(rx, algo, params, en)
        adc = synth.adc_stream(N, 0x5EED0052)
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
        bank.ctx.free(d_adc)
        return rows, bank.fs
    finally:
        bank.close()


def test_nr_receivers_in_the_bank(gpu_ctx):
    rows, fs = _run(True)
    plain, _ = _run(False)
    nblk = 0
    for rx, (mode, algo, params, en) in PLAN.items():
        assert len(rows[rx]) >= 2 and len(rows[rx]) == len(plain[rx]), rx
        active = algo in (post.NR_WDSP, post.NR_ORIG) and mode not in post.STEREO_MODES and (en[0] or en[1])
        if not active:
            for a, b in zip(rows[rx], plain[rx]):
                key = "iq_pay" if mode in post.STEREO_MODES else "pay"
                assert np.array_equal(a[key], b[key]) and np.array_equal(a["firo"].view(np.uint32), b["firo"].view(np.uint32)), (rx, key)
                if key == "pay":
                    assert np.array_equal(a["s16"], b["s16"]), rx
            continue
        P = Post(gpu_ctx, nchan=1)                      # what RxBank.set_audio + set_nr configure, standalone
        ad = wire.Adpcm(gpu_ctx, nchan=1)
        try:
            P.sam_setup(0, 12000 if abs(fs - 12000.0) < abs(fs - 20250.0) else 20250)
            P.set_sam_mparam(0, 0)
            P.set_am_passband(0, -4900.0, 4900.0, fs)
            P.set_agc(0, True, False, -100, 50, 6, 1000, fs)
            P.set_smeter(0, fs)
            P.set_mode(0, mode)
            P.reset(0)
            P.set_nr_algo(0, algo)
            for t, vals in params.items():
                for k, v in enumerate(vals):
                    P.set_nr_param(0, t, k, v)
            for t in (0, 1):
                if en[t]:
                    P.set_nr_enable(0, t, en[t])
            changed = 0
            for k, (r, q) in enumerate(zip(rows[rx], plain[rx])):
                s16, _, _ = P.process([0], r["firo"][None, :])
                assert np.array_equal(r["s16"], s16[0]), (rx, k, "mono16")
                want = np.asarray(ad.encode([0], s16)).reshape(-1)
                assert np.array_equal(r["pay"], want), (rx, k, "ADPCM")
                changed += not np.array_equal(r["s16"], q["s16"])
                nblk += 1
            assert changed == len(rows[rx]), (rx, changed)
        finally:
            ad.close()
            P.close()
    assert nblk >= 8, nblk
