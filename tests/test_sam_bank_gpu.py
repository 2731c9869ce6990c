"""The receiver bank (kg_rxbank) with receivers in the synchronous-AM family: SAM / SAU / channel-null SAM blocks leave as ADPCM rows,
SAS / QAM blocks as IQ payload rows of their (L, R) pair (IS_STEREO, rx/rx_sound.cpp:1047-1049), in either byte order.  Each SAM
receiver's rows equal a standalone kg_post (+ the ADPCM coder / IQ payload kernel) fed the bank's own CFastFIR output rows; the other
receivers' rows are byte-identical to a bank run in which the SAM receivers are SSB receivers."""
import os
import sys

import numpy as np
import pytest

from flydog_sdr_gps_amd import Post, post, wire

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 1 << 22
STEPS = 3
# receiver -> (mode, SAM_mparam, little_endian)
PLAN = {0: (post.MODE_SAM, 0, 0), 1: (post.MODE_SAU, 4, 0), 2: (post.MODE_SAS, 8, 1), 3: (post.MODE_QAM, 12, 0),
        4: (post.MODE_SAM, post.CHAN_NULL_LSB | post.DC_BLOCK, 0), 5: (post.MODE_SSB, 0, 0), 6: (post.MODE_AM, 0, 0),
        7: (post.MODE_SAS, 0, 0), 8: (post.MODE_SAL, 0, 1), 9: (post.MODE_IQ, 0, 1)}
NR = len(PLAN)


def _run(with_sam):
    from flydog_sdr_gps_amd import synth
    from flydog_sdr_gps_amd.rxbank import MIXES, RxBank
    mix = MIXES["light"](NR, 0, N)
    bank = RxBank(NR, N)
    rows = {rx: [] for rx in range(NR)}
    try:
        bank.configure(mix)
        for rx, (mode, mp, le) in PLAN.items():
            if not with_sam and mode in post.SAM_MODES:
                mode, mp = post.MODE_SSB, 0
            bank.set_audio(rx, mix[rx][2], -4900.0, 4900.0, mode=mode, sam_mparam=mp)
            bank.set_little_endian(rx, le)
        adc = synth.adc_stream(N, 0x5EED0051)
        d_adc = bank.ctx.alloc(adc.nbytes)
        bank.ctx.upload(d_adc, adc)
        live = list(range(NR))
        for step in range(STEPS):
            bank.step(d_adc)
            bank.sync()
            _, nfir, _, _ = bank.audio_map()
            g = {k: bank.fetch(k, live) for k in ("firo", "s16", "pay", "agc", "iq_pay")}
            for rx in live:
                for blk in range(int(nfir[rx]) // 512):
                    sl = slice(512 * blk, 512 * (blk + 1))
                    rows[rx].append({"firo": np.ascontiguousarray(g["firo"][rx, sl]).view(np.complex64).ravel(), "s16": g["s16"][rx, sl].copy(),
                                     "pay": g["pay"][rx, 256 * blk:256 * (blk + 1)].copy(), "agc": g["agc"][rx, sl].copy(),
                                     "iq_pay": g["iq_pay"][rx, 2048 * blk:2048 * (blk + 1)].copy()})
        bank.ctx.free(d_adc)
        return rows, bank.fs
    finally:
        bank.close()


def test_sam_receivers_in_the_bank(gpu_ctx):
    rows, fs = _run(True)
    plain, _ = _run(False)
    nblk = 0
    for rx, (mode, mp, le) in PLAN.items():
        assert len(rows[rx]) >= 2, (rx, len(rows[rx]))
        if mode not in post.SAM_MODES:
            assert len(rows[rx]) == len(plain[rx])
            for a, b in zip(rows[rx], plain[rx]):
                key = "iq_pay" if mode in post.STEREO_MODES else "pay"
                assert np.array_equal(a[key], b[key]) and np.array_equal(a["firo"].view(np.uint32), b["firo"].view(np.uint32)), (rx, mode, key)
                if key == "pay":
                    assert np.array_equal(a["s16"], b["s16"]), rx
            continue
        P = Post(gpu_ctx, nchan=1)                      # what RxBank.set_audio configures, standalone
        ad = wire.Adpcm(gpu_ctx, nchan=1)
        try:
            P.sam_setup(0, 12000 if abs(fs - 12000.0) < abs(fs - 20250.0) else 20250)
            P.set_sam_mparam(0, mp)
            P.set_am_passband(0, -4900.0, 4900.0, fs)
            P.set_agc(0, True, False, -100, 50, 6, 1000, fs)
            P.set_smeter(0, fs)
            P.set_mode(0, mode)
            P.reset(0)
            for k, r in enumerate(rows[rx]):
                s16, _, agc = P.process([0], r["firo"][None, :])
                if mode in post.STEREO_MODES:
                    want = np.asarray(wire.snd_iq_payload(gpu_ctx, agc, le)).reshape(-1)
                    assert np.array_equal(r["iq_pay"], want), (rx, mode, k, "IQ payload of the (L, R) pair")
                else:
                    assert np.array_equal(r["s16"], s16[0]), (rx, mode, k, "mono16")
                    want = np.asarray(ad.encode([0], s16)).reshape(-1)
                    assert np.array_equal(r["pay"], want), (rx, mode, k, "ADPCM")
                if mode == post.MODE_SAS or mode == post.MODE_QAM or mp & 3:
                    assert np.array_equal(r["agc"].view(np.uint32).ravel(), agc[0].view(np.uint32).ravel()), (rx, mode, k, "agc pair")
                nblk += 1
        finally:
            ad.close()
            P.close()
    assert nblk >= 14, nblk
