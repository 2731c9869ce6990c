"""kg_post's synchronous-AM family (KG_POST_SAM .. KG_POST_QAM) against c2s_sound()'s own SAM arm (rx/rx_sound.cpp:791-806 ->
rx/wdsp/SAM_demod.cpp), with the reference's S-meter, CAgc, de-emphasis, payload and header statements around it
(tests/golden/sam_ref.npz, made by tools/make_ref_sam_golden.py from tools/ref/ref_sam_main.cpp): per CFastFIR block sMeterAvg_dB and
its taps, out_samps_s2, agc_samps_c (the AGC output, or the stereo / nulled pair written over it), wdsp_SAM_carrier() and
s->isChanNull; per packet every payload byte (ADPCM, raw, IQ pairs in either byte order) and the header -- BIT-EXACT (agc_samps_c
and the payloads through SHA-256 digests of their bytes, which the golden file keeps instead of the bytes).
Then: a batch of mixed-mode channels equals each channel run alone, channel lists that change between calls, argument errors."""
import os

import numpy as np
import pytest

from flydog_sdr_gps_amd import Post, post, wire
from flydog_sdr_gps_amd._lib import KiwiGpuError
from tests.script_common import digest_u8 as digest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# rx/mode.h:69-70 -> KG_POST_*
M_IQ, M_DRM, M_NBFM, M_NNFM, M_SAM, M_QAM = 7, 8, 6, 16, 11, 15
KG_MODE = {0: post.MODE_AM, 1: post.MODE_AM, 6: post.MODE_NBFM, 16: post.MODE_NBFM, 7: post.MODE_IQ, 8: post.MODE_IQ,
           11: post.MODE_SAM, 12: post.MODE_SAU, 13: post.MODE_SAL, 14: post.MODE_SAS, 15: post.MODE_QAM}
STEREO = (7, 8, 14, 15)                                   # IS_STEREO (rx/mode.h:45-55)
FLAG_MODE_IQ, FLAG_COMPRESSED, FLAG_LITTLE_ENDIAN = 0x08, 0x10, 0x80   # rx_sound.cpp:461-468
S_METER_CAL = np.float32(-13)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_scenario(ctx, g, name):
    """Drives one kg_post channel, the ADPCM coder and the payload / header kernels by the scenario's script; asserts equality
    with what the reference's statements produced (agc_samps_c and the payloads through their SHA-256 digests, as the golden file
    keeps them).  -> (packets, blocks, samples)"""
    rate = float(g[name + "_rate"][0])
    snd_rate = 12000 if abs(rate - 12000.0) < abs(rate - 20250.0) else 20250
    x = g[name + "_in"].astype(np.float32).view(np.complex64)
    rec_all, s16_all, agc_sha = g[name + "_rec"], g[name + "_s16"], g[name + "_agc_sha"]
    pkt_len, pkt_head, pkt_sha = g[name + "_pkt_len"], g[name + "_pkt_head"], g[name + "_pkt_sha"]
    P = Post(ctx, nchan=1)
    ad = wire.Adpcm(ctx, nchan=1)
    try:
        P.sam_setup(0, snd_rate)                          # wdsp_SAM_demod_init() at the server's snd_rate
        P.set_smeter(0, rate); P.set_mode(0, post.MODE_SSB); P.reset(0)
        P.squelch_setup(0, rate); P.squelch_set(0, 0, 0)
        mode, comp, le = 2, 1, False
        pos = npkt = nblk = seq = s16pos = nagc = 0
        for line in (str(l) for l in g[name + "_script"]):
            f = line.split()
            op = f[0]
            if op == "R":
                assert float(f[1]) == rate
            elif op == "A":
                P.set_agc(0, *[int(v) for v in f[1:7]], rate)
            elif op == "L":
                P.cfir_init_lp(0, post.CFIR_AM, 0, 1.0, 50.0, float(f[1]), float(f[2]), rate)
            elif op == "E":
                r12k = abs(rate - 12000.0) < abs(rate - 20250.0)
                P.set_de_emp(0, int(f[1]), 0, snd_rate_12k=r12k, frate=rate)
                P.set_de_emp(0, int(f[2]), 1, snd_rate_12k=r12k, frate=rate)
            elif op == "M":
                mode = int(f[1])
                P.set_mode(0, KG_MODE.get(mode, post.MODE_SSB))
            elif op == "G":
                P.sam_pll(0, int(f[1]))
            elif op == "N":
                P.set_sam_mparam(0, int(f[1]))
            elif op == "W":
                comp, le = int(f[1]), bool(int(f[2]))
            else:
                assert op == "P", line
                stereo, sam = mode in STEREO, M_SAM <= mode <= M_QAM
                payload, dbm = [], None
                for n in (int(v) for v in f[1:]):
                    s16, _, agc = P.process([0], x[pos:pos + n][None, :])
                    pos += n
                    avg, taps = P.smeter([0])
                    car, null, _ = P.sam_state([0])
                    rec = rec_all[nblk]
                    where = (name, npkt, nblk, mode, n)
                    assert bits(np.float32(avg[0])) == bits(rec[0]), (where, "sMeterAvg_dB", avg[0], rec[0])
                    assert np.float32(taps[0, 0]) + S_METER_CAL == rec[2], (where, "S-meter tap j = 0")
                    if n >= 2:
                        assert np.float32(taps[0, 1]) + S_METER_CAL == rec[3], (where, "S-meter tap j = n / 2")
                    assert bits(np.float32(car[0])) == bits(rec[5]), (where, "wdsp_SAM_carrier", car[0], rec[5])
                    assert int(null[0]) == int(rec[6]), (where, "isChanNull", null[0], rec[6])
                    if not stereo:
                        want = s16_all[s16pos:s16pos + n].astype(np.int32)
                        s16pos += n
                        got = s16[0].astype(np.int32)
                        assert np.array_equal(got, want), (where, "out_samps_s2", int(np.abs(got - want).max()), int(np.argmax(got != want)))
                    if stereo or sam:
                        assert np.array_equal(digest(np.ascontiguousarray(agc[0], np.complex64).tobytes()), agc_sha[nagc]), (where, "agc_samps_c")
                        nagc += 1
                    if stereo:
                        payload.append(np.asarray(wire.snd_iq_payload(ctx, agc[0][None, :], le)).reshape(-1))
                    elif comp:
                        payload.append(np.asarray(ad.encode([0], s16[0][None, :])).reshape(-1))
                    else:
                        payload.append(np.asarray(wire.snd_payload(ctx, s16[0][None, :], le)).reshape(-1))
                    dbm = np.float32(rec[1])
                    nblk += 1
                hsize, bc = (int(v) for v in pkt_len[npkt])
                payload = np.concatenate(payload).astype(np.uint8)
                assert payload.size == bc and np.array_equal(digest(payload.tobytes()), pkt_sha[npkt]), (name, npkt, mode, "payload", payload.size, bc)
                seq += 1
                flags = (FLAG_MODE_IQ if stereo else 0) | (FLAG_COMPRESSED if comp and not stereo else 0) | (FLAG_LITTLE_ENDIAN if le else 0)
                hdr = np.asarray(wire.snd_header(ctx, flags, seq, float(dbm)), np.uint8)
                assert hsize == (20 if stereo else 10) and np.array_equal(hdr[:10], pkt_head[npkt, :10]), (name, npkt, mode, "header", hdr[:10],
                                                                                                          pkt_head[npkt, :10])
                npkt += 1
        assert pos == x.size and nblk == len(rec_all) and s16pos == s16_all.size and nagc == len(agc_sha) and npkt == len(pkt_len), name
        return npkt, nblk, pos
    finally:
        ad.close()
        P.close()


def test_sam_family_matches_the_references_own_statements(gpu_ctx):
    g = np.load(os.path.join(GOLD, "sam_ref.npz"))
    packets = blocks = samples = 0
    for name in (str(n) for n in g["names"]):
        p, b, s = run_scenario(gpu_ctx, g, name)
        packets, blocks, samples = packets + p, blocks + b, samples + s
    assert packets >= 40 and blocks >= 100 and samples >= 50000, (packets, blocks, samples)


# ---- a batch of mixed modes in one launch = each channel alone ------------------------------------------------------------
NCH = 72
BATCH_MODES = [post.MODE_SAM, post.MODE_SAU, post.MODE_SAL, post.MODE_SAS, post.MODE_QAM, post.MODE_SSB, post.MODE_AM, post.MODE_NBFM,
               post.MODE_IQ]


def _station(rng, n, rate, f0, k):
    t = (np.arange(n) + k * n) / rate
    env = 1.0 + 0.4 * np.sin(2 * np.pi * 700.0 * t) + 0.3 * np.cos(2 * np.pi * 1300.0 * t + 0.5)
    x = 4000.0 * env * np.exp(2j * np.pi * f0 * t) + 30.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def _setup(P, ch, k, rate):
    mode = BATCH_MODES[k % len(BATCH_MODES)]
    P.sam_setup(ch, 12000 if rate < 15000 else 20250)
    P.set_agc(ch, k % 5 != 4, k & 1, -100 + (k % 3) * 10, 50, 6, 1000, rate)
    P.set_smeter(ch, rate)
    P.set_am_passband(ch, -4900, 4900, rate)
    P.squelch_setup(ch, rate); P.squelch_set(ch, 0, 0)
    P.set_mode(ch, mode)
    P.reset(ch)
    P.set_sam_mparam(ch, [0, 4, 8, 12, 1, 2, 9, 14][k % 8])
    P.sam_pll(ch, [1, 0, 2][k % 3])
    if k % 7 == 3:
        P.set_de_emp(ch, 1, 0, snd_rate_12k=rate < 15000, frate=rate)


def test_mixed_batch_and_changing_lists_equal_each_channel_alone(gpu_ctx):
    rng = np.random.default_rng(0x5A5)
    n = 512
    rates = [12000.0 if k % 4 else 20250.0 for k in range(NCH)]
    f0 = rng.uniform(-80, 80, NCH)
    lists = [np.arange(NCH), np.arange(0, NCH, 2), rng.permutation(NCH)[:50], np.arange(NCH)[::-1]]
    B = Post(gpu_ctx, nchan=NCH)
    try:
        for k in range(NCH):
            _setup(B, k, k, rates[k])
        xs = [[_station(rng, n, rates[k], f0[k], step) for k in range(NCH)] for step in range(len(lists))]
        batch = []
        for step, lst in enumerate(lists):
            lst = np.ascontiguousarray(lst, np.int32)
            s16, dem, agc = B.process(lst, np.stack([xs[step][k] for k in lst]))
            car, null, phz = B.sam_state(lst)
            avg, _ = B.smeter(lst)
            batch.append({int(k): (s16[i], agc[i], car[i], null[i], phz[i], avg[i]) for i, k in enumerate(lst)})
    finally:
        B.close()
    for k in range(0, NCH, 1):
        A = Post(gpu_ctx, nchan=1)
        try:
            _setup(A, 0, k, rates[k])
            mode = BATCH_MODES[k % len(BATCH_MODES)]
            for step, lst in enumerate(lists):
                if k not in batch[step]:
                    continue
                s16, _, agc = A.process([0], xs[step][k][None, :])
                car, null, phz = A.sam_state([0])
                avg, _ = A.smeter([0])
                b = batch[step][k]
                where = (k, mode, step)
                if mode not in post.STEREO_MODES:
                    assert np.array_equal(s16[0], b[0]), (where, "s16")
                if mode != post.MODE_SSB:
                    assert np.array_equal(bits(agc[0].view(np.float32)), bits(b[1].view(np.float32))), (where, "agc")
                assert bits(np.float32(car[0])) == bits(np.float32(b[2])) and null[0] == b[3], (where, "carrier / isChanNull")
                assert bits(np.float32(phz[0])) == bits(np.float32(b[4])) and bits(np.float32(avg[0])) == bits(np.float32(b[5])), where
        finally:
            A.close()


def test_sam_state_semantics(gpu_ctx):
    """A fresh channel is at snd_rate 12000, PLL MED, reset: a SAM mode runs without any set-up; the mode change into the family
    resets the PLL, a change inside it does not; every mode change clears isChanNull."""
    rng = np.random.default_rng(3)
    x = _station(rng, 512, 12000.0, 40.0, 0)[None, :]
    P = Post(gpu_ctx, nchan=1)
    try:
        P.set_mode(0, post.MODE_SAM)
        P.set_sam_mparam(0, post.CHAN_NULL_LSB)
        P.process([0], x)
        car, null, phz = P.sam_state([0])
        assert null[0] == 1 and phz[0] != 0
        P.set_mode(0, post.MODE_SAU)                 # inside the family: no reset
        assert P.sam_state([0])[0][0] == car[0] and P.sam_state([0])[1][0] == 0 and P.sam_state([0])[2][0] == phz[0]
        P.set_mode(0, post.MODE_SSB)
        P.set_mode(0, post.MODE_QAM)                 # non-SAM -> SAM: PLL_RESET
        assert tuple(v[0] for v in P.sam_state([0])) == (0.0, 0, 0.0)
        P.process([0], x)
        assert P.sam_state([0])[2][0] != 0
        P.sam_pll(0, post.PLL_RESET)
        assert P.sam_state([0])[2][0] == 0
    finally:
        P.close()


def test_argument_errors(gpu_ctx):
    P = Post(gpu_ctx, nchan=2)
    try:
        with pytest.raises(KiwiGpuError):
            P.set_mode(0, 9)
        with pytest.raises(KiwiGpuError):
            P.sam_pll(0, 3)
        with pytest.raises(KiwiGpuError):
            P.sam_pll(1, -2)
        with pytest.raises(KiwiGpuError):
            P.sam_setup(0, 44100)
        with pytest.raises(KiwiGpuError):
            P.sam_setup(2, 12000)
        P.set_mode(1, post.MODE_SAU)
        P.set_de_emp(1, 1, 0)                          # the filter is designed: fine
        P.set_deemp(0, False, 1)                       # de-emphasis on without coefficients: refused for the mono SAM modes
        P.set_mode(0, post.MODE_SAL)
        with pytest.raises(KiwiGpuError):
            P.process([0], np.zeros((1, 64), np.complex64))
        P.set_mode(0, post.MODE_SAS)                   # stereo: no de-emphasis, accepted
        P.process([0, 1], np.zeros((2, 64), np.complex64))
    finally:
        P.close()
