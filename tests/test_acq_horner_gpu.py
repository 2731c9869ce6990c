"""GPU parity of the C/A correlator's Horner combine (acq_correlate_kernel: the row part of the combine twiddle folded
into pass 2, the rest a Horner chain over k2 from P - 1 down) against the CPU oracle, on the shapes where its walk differs:
every residue (k2 - dop) mod P with both signs of dop and of floor((k2 - dop) / P), the spread walk (fewer than eight
(block, SV) pairs) and the grouped walk with claimed cells, windows that end inside a 256-lag row or before the last rows,
and P = 16 (fifteen Horner steps per cell).

Bars as tests/test_acq_gpu.py: every cell's peak index, the winning Doppler bin and `valid` equal; snr, max_pwr and tot_pwr
within 1e-5 relative."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Searcher, acq, prn, sats, synth
from tests.fixtures import oracle_next_rows

pytestmark = pytest.mark.gpu

RTOL = 1e-5
N10, FFT10 = acq.NSAMPLES_10MS, acq.FFT_LEN_10MS


def ca(sat):
    _, t1, t2, _ = sats.SATS[sat]
    return prn.cacode(t1, t2)


def check(res, cells, want, wcells, tag):
    assert np.array_equal(cells["idx"], wcells["idx"]), tag
    assert np.array_equal(res["dop"], want["dop"]), tag
    assert np.array_equal(res["idx"], want["idx"]), tag
    assert np.array_equal(res["valid"], want["valid"]), tag
    for k in ("snr", "max_pwr", "tot_pwr"):
        err = float(np.max(np.abs(cells[k] - wcells[k]) / np.abs(wcells[k])))
        print("%s: %s max rel err %.3g" % (tag, k, err))
    np.testing.assert_allclose(res["snr"], want["snr"], rtol=RTOL, err_msg=tag)
    np.testing.assert_allclose(cells["snr"], wcells["snr"], rtol=RTOL, err_msg=tag)
    np.testing.assert_allclose(cells["max_pwr"], wcells["max_pwr"], rtol=RTOL, err_msg=tag)
    np.testing.assert_allclose(cells["tot_pwr"], wcells["tot_pwr"], rtol=RTOL, err_msg=tag)


def test_p4_spread_walk_every_residue(gpu_ctx, oracle):
    """One block, two C/A SVs (one injected, one absent), dop -5..6: two pairs -> the cells are dealt round-robin."""
    lo, hi = -5, 6
    s = Searcher(gpu_ctx, max_sats=4, dop_lo=lo, dop_hi=hi)
    try:
        svs = [0, 1]
        for sat in svs:
            s.set_code(sat, ca(sat))
        bits = synth.gps_scene_bits([(ca(0), 100.25, 700.0, 0.3)], seed=11)
        s.sample(bits)
        res, cells = s.correlate_many(svs)
        codes = np.stack([oracle.code_fft(ca(sat)) for sat in svs])
        want, wcells = oracle.correlate_many(codes, oracle.sample_bits(bits), [sats.L1_LIMIT] * 2, dop_lo=lo, dop_hi=hi,
                                             nthreads=4, nexts=oracle_next_rows(oracle, s, svs))
        check(res[0], cells[0], want, wcells, "P=4 spread")
        assert int(res[0, 0]["dop"]) == 3 and int(res[0, 0]["idx"]) == 401      # +700 Hz, 100.25 chips
        assert res[0, 0]["snr"] >= 16 > res[0, 1]["snr"]
    finally:
        s.close()


def test_p4_grouped_walk_claims_and_windows(gpu_ctx, oracle):
    """3 blocks x 3 SVs = nine pairs: the grouped walk with claimed cells; windows of 4092 (partial last row), 4096 (all
    rows whole) and 1000 lags (rows beyond the window)."""
    lo, hi = -5, 6
    s = Searcher(gpu_ctx, max_sats=4, max_blocks=3, dop_lo=lo, dop_hi=hi)
    try:
        svs, limits = [0, 1, 2], [4092, 4096, 1000]
        for sat, limit in zip(svs, limits):
            s.set_code(sat, ca(sat), limit=limit)
        codes = np.stack([oracle.code_fft(ca(sat)) for sat in svs])
        scenes = [[(ca(0), 100.25, 700.0, 0.3)], [(ca(1), 900.5, -1000.0, 1.1)], [(ca(2), 200.75, 250.0, 2.0), (ca(0), 10.0, -500.0, 0.7)]]
        allbits = [synth.gps_scene_bits(sc, seed=21 + b) for b, sc in enumerate(scenes)]
        for b, bits in enumerate(allbits):
            s.sample(bits, block=b)
        res, cells = s.correlate_many(svs, nblocks=3)
        nexts = oracle_next_rows(oracle, s, svs)
        for b, bits in enumerate(allbits):
            want, wcells = oracle.correlate_many(codes, oracle.sample_bits(bits), limits, dop_lo=lo, dop_hi=hi, nthreads=4, nexts=nexts)
            check(res[b], cells[b], want, wcells, "P=4 grouped, block %d" % b)
            assert np.all(cells[b]["idx"] < np.asarray(limits)[:, None])
    finally:
        s.close()


def test_p16_every_residue(gpu_ctx, oracle):
    """10 ms / 65536 points: one block, two SVs, dop -9..8 -- every residue mod 16, fifteen Horner steps per cell."""
    lo, hi = -9, 8
    s = Searcher(gpu_ctx, max_sats=4, dop_lo=lo, dop_hi=hi, nsamples=N10, fft_len=FFT10)
    try:
        svs = [0, 1]
        for sat in svs:
            s.set_code(sat, ca(sat))
        bits = synth.gps_scene_bits([(ca(0), 100.25, 250.0, 0.3)], seed=31, n=N10)
        s.sample(bits)
        res, cells = s.correlate_many(svs)
        codes = np.stack([oracle.code_fft(ca(sat), fft_len=FFT10) for sat in svs])
        data = oracle.sample_bits(bits, nsamples=N10, fft_len=FFT10)
        want, wcells = oracle.correlate_many(codes, data, [sats.L1_LIMIT] * 2, dop_lo=lo, dop_hi=hi, nthreads=4,
                                             nexts=oracle_next_rows(oracle, s, svs))
        check(res[0], cells[0], want, wcells, "P=16")
        assert int(res[0, 0]["dop"]) == 4 and int(res[0, 0]["idx"]) == 401      # +250 Hz / 62.44 Hz, 100.25 chips
    finally:
        s.close()
