"""The device transforms against the double-precision DFT, at fp32 accuracy.

The parity tests hold every output behind one of our own FFTs to 1e-5 of the maximum against the CPU oracle: 50 to 80 times
looser than a plain fp32 transform, and measured against another rounded transform.  Here the truth is numpy.fft in complex128
on the exact inputs the kernel transformed, and the bar is the error of the oracle's own fp32 radix-4 transform (prec=0) on the
same input against the same truth, computed on the CPU while the test runs (tests/dft_truth.py: bars, inputs, truths;
tests/test_dft_truth_cpu.py: the yardstick pinned, the bar shown to fail on planted defects).

A  forward 16384 / 65536 (acq_fft_sub_kernel, acq_fft_combine_kernel), data and code side
B  backward transforms inside acq_correlate_kernel<4> / <16> and acq_correlate8_kernel<4> / <16>
C  the waterfall's 8192 points (wf_frame_kernel, through kg_wf_debug_frame's pwr)
D  CFastFIR's 1024-point pair (fir_coef_fft_kernel, fir_block_kernel)

Every comparison goes through tests.errlog.record: the kernel's error, the fp32 oracle's, the bar (profiles/dft_truth.txt)."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import FastFir, Searcher, Waterfall, WfParams, acq, prn, sats, synth, wf
from tests import dft_truth as T
from tests.fixtures import e1b_chips

pytestmark = pytest.mark.gpu

SHAPES = {16384: (acq.NSAMPLES, acq.FFT_LEN, 4), 65536: (acq.NSAMPLES_10MS, acq.FFT_LEN_10MS, 16)}


@pytest.fixture(scope="module")
def searchers(gpu_ctx):
    """max_sats = 2 and only row 0 ever written: the row a negative Doppler bin reads into stays zero"""
    s = {16384: Searcher(gpu_ctx, max_sats=2, dop_lo=-2, dop_hi=2),
         65536: Searcher(gpu_ctx, max_sats=2, dop_lo=-2, dop_hi=2, nsamples=acq.NSAMPLES_10MS, fft_len=acq.FFT_LEN_10MS)}
    yield s
    for v in s.values():
        v.close()


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- A ------------------------------------------------------------------------------------------------------------------------
_white_a = {}


def white_a(oracle, n):
    """the fp32 oracle's (e_rms, e_max) on the family's white-noise input at this length"""
    if n not in _white_a:
        nsamples, fft_len, _ = SHAPES[n]
        ref32, td = oracle.sample_iq16(T.iq16_noise(nsamples, 1), prec=0, want_td=True, nsamples=nsamples, fft_len=fft_len)
        _white_a[n] = T.spectrum_errors(ref32, T.dft(td))
    return _white_a[n]


def data_side(s, oracle, n, name, iq=None, bits=None):
    """Sample() of one block: the decimated sequence bit-equal to the oracle's, then its spectrum against the DFT of that
    sequence -- the decimators stay out of the comparison"""
    nsamples, fft_len, _ = SHAPES[n]
    if iq is not None:
        s.sample_iq16(iq)
        ref32, td = oracle.sample_iq16(iq, prec=0, want_td=True, nsamples=nsamples, fft_len=fft_len)
    else:
        s.sample(bits)
        ref32, td = oracle.sample_bits(bits, prec=0, want_td=True, nsamples=nsamples, fft_len=fft_len)
    assert bits_equal(s.get_data_td(), td), name
    failures = T.check_spectrum("A%d %s" % (n, name), s.get_data_fft(), ref32, T.dft(td), white_a(oracle, n))
    assert not failures, (n, name, failures)
    return td


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_forward_transform_of_signals(searchers, oracle, n):
    s, (nsamples, fft_len, _) = searchers[n], SHAPES[n]
    data_side(s, oracle, n, "noise", iq=T.iq16_noise(nsamples, 1))
    data_side(s, oracle, n, "carrier -60 dB", iq=T.iq16_carrier(nsamples, fft_len, fft_len // 8 + 3, 2))
    td = data_side(s, oracle, n, "dc", iq=T.iq16_dc(nsamples))
    assert np.all(td[:1000] == td[0]) and td[0] != 0
    td = data_side(s, oracle, n, "alternating", iq=T.iq16_alternating(nsamples))
    assert np.all(td[:1000:2] == td[0]) and np.all(td[1:1000:2] == td[1]) and abs(td[0] - td[1]) > 1000
    rng = np.random.default_rng(3)
    data_side(s, oracle, n, "1-bit noise", bits=rng.integers(0, 256, nsamples // 8).astype(np.uint8))
    chips = prn.cacode(2, 6)
    data_side(s, oracle, n, "1-bit scene", bits=synth.gps_scene_bits([(chips, 100.25, 700.0, 0.3)], seed=7, n=nsamples))


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_forward_transform_of_impulses(searchers, oracle, n):
    """One int16 pair in a block of zeros, so that the decimated sequence is one entry (tests.dft_truth.iq16_impulse) and the
    spectrum one twiddle product per bin: every residue of the split, the first, the last and a carry value of each radix-16
    digit of the 4096-point index."""
    s, (nsamples, fft_len, radix) = searchers[n], SHAPES[n]
    for t, pure in T.acq_impulse_indices(nsamples, fft_len, radix):
        iq, _ = T.iq16_impulse(nsamples, t)
        td = data_side(s, oracle, n, "impulse %d" % t, iq=iq)
        nz = np.flatnonzero(td)
        assert nz[-1] == t and (nz.size == 1) == pure, (t, nz)


@pytest.mark.parametrize("n", sorted(SHAPES))
@pytest.mark.parametrize("boc", [False, True], ids=["ca", "e1b"])
def test_code_transform(searchers, oracle, n, boc):
    s, (_, fft_len, _) = searchers[n], SHAPES[n]
    chips = e1b_chips()[1] if boc else prn.cacode(*sats.SATS[0][1:3])
    s.set_code(0, chips, boc=boc)
    td, _ = oracle.code_replica(chips, boc=boc, fft_len=fft_len)
    ref32 = oracle.code_fft(chips, boc=boc, prec=0, fft_len=fft_len)
    failures = T.check_spectrum("A%d code %s" % (n, "E1B" if boc else "C/A"), s.get_code_fft(0), ref32, T.dft(td), white_a(oracle, n))
    assert not failures, failures


# ---- B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", T.corr_limits(16384))
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_correlator_cells(searchers, oracle, n, limit):
    """limit <= 4096: acq_correlate_kernel<4> (16384) / <16> (65536); above: acq_correlate8_kernel.  Spectra go in exact with
    set_data_fft / set_code_fft; the truth is tests.dft_truth.cell_truth on those values.  Powers are compared where the truth
    exceeds POWER_FRAC of its transform's peak (tests.dft_truth), indices where the truth's top two are more than TIE apart."""
    from tests.errlog import record
    s, radix = searchers[n], SHAPES[n][2]
    rows = []
    for name, kind, data, code in T.corr_inputs(n, radix):
        s.set_data_fft(data)
        s.set_code_fft(0, code, limit=limit)
        _, cells = s.correlate_many([0])
        _, ref = oracle.correlate(code, data, limit=limit, dop_lo=-2, dop_hi=2, prec=0)
        rows.append((name, kind, cells[0, 0].copy(), ref, T.cells_truth(data, code, limit)))
    worst = lambda c, truth, k: float(np.nan_to_num(T.power_errors(c, truth, k)).max())      # 0 where no cell is strong enough
    kept = sum(int(np.isfinite(T.power_errors(ref, truth, "max_pwr")).sum()) for _, _, _, ref, truth in rows)
    assert kept >= 0.95 * 5 * len(rows), kept
    white_max = max(worst(ref, truth, "max_pwr") for _, kind, _, ref, truth in rows if kind == "scene")
    bad, checked, left = [], 0, 0
    tot = {}
    for name, kind, got, ref, truth in rows:
        ok, b = T.judge("B%d limit %d %s max_pwr" % (n, limit, name), worst(got, truth, "max_pwr"), worst(ref, truth, "max_pwr"), white_max)
        if not ok:
            bad.append((name, "max_pwr", worst(got, truth, "max_pwr"), b))
        g, r = tot.setdefault(kind, [0.0, 0.0])
        tot[kind] = [max(g, worst(got, truth, "tot_pwr")), max(r, worst(ref, truth, "tot_pwr"))]
        if T.index_checked(kind, limit):
            for i, t in enumerate(truth):
                checked += 1
                if t["gap"] < T.TIE:
                    left += 1
                elif int(got["idx"][i]) != t["idx"]:
                    bad.append((name, "idx", i, int(got["idx"][i]), t["idx"]))
    # tot_pwr: the maximum over the cells of the test, per kind of input (a line pattern's periodic terms push the reference's
    # sequential sum to 1e-4; lumped together that would be the bar of the noisy scenes too)
    for kind, (g, r) in sorted(tot.items()):
        record("dft_truth B%d limit %d %s tot_pwr | fp32 ref %.3e" % (n, limit, kind, r), 1.0 + g, 1.0, T.TOT_FACTOR * r)
        if g > T.TOT_FACTOR * r:
            bad.append((kind, "tot_pwr", g, T.TOT_FACTOR * r))
    assert not bad, bad
    assert left <= 0.05 * checked


# ---- C ------------------------------------------------------------------------------------------------------------------------
WF_FRAMES = {
    # name: (window, frame, strong fraction for the per-bin relative error, bins of the weak tone or None)
    "noise -30 dBFS, Hanning": (wf.WINF_HANNING, lambda: T.wf_noise(5), 1e-2, None),
    "full-scale carrier, no window": (wf.WINF_NONE, lambda: T.wf_tones([(400, 0.0)]), 0.5, None),
    "two tones 80 dB apart, Blackman-Harris": (wf.WINF_BLACKMAN_HARRIS, lambda: T.wf_tones([(300, -1.0), (1200, -81.0)]), 0.5,
                                               np.arange(1198, 1203)),
}


@pytest.fixture(scope="module")
def wf_engine(gpu_ctx):
    w = Waterfall(gpu_ctx, nchan=2)
    w.set_tables(wf.window_functions(), wf.cic_comp_table())
    yield w
    w.close()


def wf_errors(pwr, truth, frac, weak_tone):
    """(relative error of the strong bins, magnitude error of all the others against the frame's largest, relative error of
    the weak tone's bins)"""
    strong = truth > frac * truth.max()
    return (T.pwr_rel(pwr, truth, frac), T.floor_err(pwr, truth, ~strong),
            T.pwr_rel(pwr[weak_tone], truth[weak_tone]) if weak_tone is not None else 0.0)


@pytest.mark.parametrize("zoom", [0, 3])
@pytest.mark.parametrize("frame", sorted(WF_FRAMES))
def test_waterfall_power(wf_engine, oracle, frame, zoom):
    """pwr[] of compute_frame(): |X[i]|^2 of the windowed samples (exact float products, oracle.wf_window_iq), times the CIC
    compensation where the zoomed channel applies it (oracle/kiwi_oracle_wf.c)."""
    window_func, make, frac, weak_tone = WF_FRAMES[frame]
    windows, cic = wf.window_functions(), wf.cic_comp_table()
    p = WfParams.for_zoom(zoom, 1.0e6 * zoom)
    wf_engine.set_channel(zoom != 0, p, interp=wf.WF_MAX, window_func=window_func, cic_comp=True)
    dc_bins = 4 if (zoom == 0 and window_func == wf.WINF_BLACKMAN_HARRIS) else 2
    comp = cic if zoom > 1 else None

    def three(iq, win):
        samps = oracle.wf_window_iq(iq, windows[win])
        truth = T.wf_pwr_truth(samps, p.fft_used, dc_bins if win == window_func else 2, comp)
        m, d = wf.build_maps(p.fft_used, p.plot_width, p.plot_width_clamped)
        sc = np.full(1024, p.fft_scale, np.float32)
        ref = oracle.wf_compute_frame(samps, p.zoom, win, wf.WF_MAX, True, False, p.fft_used, p.plot_width, p.plot_width_clamped,
                                      m, d, sc, (sc / np.float32(2)).astype(np.float32), p.fft_offset, cic, prec=0)[1]
        return samps, truth, ref

    iq = make()
    _, truth, ref = three(iq, window_func)
    _, w_truth, w_ref = three(T.wf_noise(5), wf.WINF_HANNING)              # the family's white-noise frame on this channel
    white = wf_errors(w_ref, w_truth, 1e-2, None)
    got = wf_engine.debug_frame(zoom != 0, iq)[1][:p.fft_used]
    e_got, e_ref = wf_errors(got, truth, frac, weak_tone), wf_errors(ref, truth, frac, weak_tone)
    bad = []
    for k, what in enumerate(("strong bins", "floor", "weak tone")):
        if k == 2 and weak_tone is None:
            continue
        # the white-noise term of a bar is the white frame's error in the same metric; the weak tone's bins have none
        ok, b = T.judge("C zoom %d %s: %s" % (zoom, frame, what), e_got[k], e_ref[k], white[k] if k < 2 else 0.0)
        if not ok:
            bad.append((what, e_got[k], b))
    assert not bad, bad


# ---- D ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fir(gpu_ctx):
    f = FastFir(gpu_ctx, nchan=2, max_in=4096)
    yield f
    f.close()


FIR_BANDS = [(300.0, 2700.0, 0.0, 12000.0), (-4900.0, 4900.0, 0.0, 12000.0), (-200.0, 200.0, 500.0, 20250.0)]


@pytest.fixture(scope="module")
def fir_white(oracle):
    """the fp32 oracle's error on a 1024-point transform of white noise"""
    x = T.white(1024, 21)
    return T.spectrum_errors(oracle.fft(x, prec=0), T.dft(x))


@pytest.mark.parametrize("band", FIR_BANDS, ids=lambda b: "%g..%g+%g@%g" % b)
def test_fir_coefficient_transform(fir, oracle, fir_white, band):
    """fir_coef_fft_kernel: get_coef after setup against the DFT of the float time-domain taps"""
    assert fir.setup(0, *band)
    _, _, taps = oracle.fir_design(*band, prec=0)
    ref32 = oracle.fir_design(*band, prec=0)[1]
    failures = T.check_spectrum("D coef %g..%g" % band[:2], fir.get_coef(0), ref32, T.dft(taps), fir_white)
    assert not failures, failures


@pytest.mark.parametrize("hop", [512, 170])
@pytest.mark.parametrize("coef_name", ["allpass", "passband"])
def test_fir_processing(fir, oracle, coef_name, hop):
    """fir_block_kernel with a caller-supplied spectrum (kg_fir_set_coef): overlap-save in complex128 with exactly that float
    spectrum.  The all-pass makes the forward and the backward transform a pure round trip."""
    coef = T.fir_allpass() if coef_name == "allpass" else oracle.fir_design(300.0, 2700.0, 0.0, 12000.0)[1]
    fir.set_coef(1, coef)
    rows = []
    for name, x in T.fir_inputs():
        x = x[:(x.size // hop) * hop]
        fir.reset(1)
        st = oracle.fir_new_state()
        got = np.concatenate([fir.process(1, x[k:k + hop]) for k in range(0, x.size, hop)])
        ref = np.concatenate([oracle.fir_process(st, coef, x[k:k + hop], prec=0)[0] for k in range(0, x.size, hop)])
        truth = T.fir_truth(coef, x)
        assert got.size == ref.size == truth.size == (x.size // 512) * 512
        rows.append((name, got, ref, truth))
    white = T.spectrum_errors(rows[0][2], rows[0][3])
    bad = []
    for name, got, ref, truth in rows:
        f = T.check_spectrum("D %s hop %d %s" % (coef_name, hop, name), got, ref, truth, white)
        if f:
            bad.append((name, f))
    assert not bad, bad
