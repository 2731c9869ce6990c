"""The double-precision DFT as the truth behind every device transform, and the bars that hold a kernel to fp32 accuracy
(tests/test_dft_truth_cpu.py, tests/test_dft_truth_gpu.py).  Test infrastructure; never imported by the product package.

Truth       numpy.fft in complex128 on the exact float (or int16) inputs, unnormalised as the kernels are; powers, sums of
            powers in float64.
Yardstick   the oracle's own fp32 radix-4 transform (prec=0) on the SAME input against the SAME truth, computed while the test
            runs.  Never the kernel.
Bars        spectra and single powers: e_gpu <= SPEC_FACTOR * max(e_ref32 on this input, e_ref32 on the family's white-noise
            input at the same length).  One factor 2: a radix-16 Stockham transform with fused 2u - s steps and a Horner combine
            is another tree with one more rounding per fused pair; the other: the maximum of a few thousand roundings against a
            yardstick that is itself one draw.  The white-noise term keeps the bar from collapsing where the radix-4 oracle
            happens to be exact (impulses, DC).
            tot_pwr: <= TOT_FACTOR * the oracle's own error, both as the maximum over all cells of the test: a blocked sum of
            non-negative terms has the smaller worst case (depth * u against n * u for the reference's sequential sum).
            peak index: equal to the float64 argmax wherever the truth's top two powers are more than TIE apart (relative).
The 1e-5 bars of the parity tests (OLD_BAR) stay the contract with the reference; these are the accuracy budget."""
import functools

import numpy as np

OLD_BAR = 1e-5
SPEC_FACTOR = 4.0
TOT_FACTOR = 2.0
TIE = 1e-4

c64, c128 = np.complex64, np.complex128


# ---- truth ---------------------------------------------------------------------------------------------------------------
def dft(x):
    return np.fft.fft(np.asarray(x).astype(c128))


def idft(X):
    """the backward transform, unnormalised (FFTW_BACKWARD)"""
    X = np.asarray(X).astype(c128)
    return np.fft.ifft(X) * X.size


def power(y):
    y = np.asarray(y).astype(c128)
    return y.real ** 2 + y.imag ** 2


# ---- metrics -------------------------------------------------------------------------------------------------------------
def e_rms(got, truth):
    truth = np.asarray(truth, c128)
    return float(np.linalg.norm(np.asarray(got).astype(c128) - truth) / np.linalg.norm(truth))


def e_max(got, truth):
    truth = np.asarray(truth, c128)
    return float(np.abs(np.asarray(got).astype(c128) - truth).max() / np.abs(truth).max())


def pwr_rel(got, truth, frac=0.0):
    """max |got / truth - 1| over the entries where truth exceeds frac * max(truth)"""
    got, truth = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(truth, np.float64))
    keep = truth > frac * truth.max()
    assert keep.any()
    return float(np.abs(got[keep] / truth[keep] - 1.0).max())


def floor_err(got_pwr, truth_pwr, weak):
    """the magnitude error on the bins `weak`, relative to the largest magnitude of the frame (e_max's analogue on powers)"""
    g, t = np.sqrt(np.asarray(got_pwr, np.float64)), np.sqrt(np.asarray(truth_pwr, np.float64))
    return float(np.abs(g - t)[weak].max() / t.max())


# ---- bars ----------------------------------------------------------------------------------------------------------------
def bar(e_ref, e_white, factor=SPEC_FACTOR):
    return factor * max(float(e_ref), float(e_white))


def judge(name, e_got, e_ref, e_white, factor=SPEC_FACTOR):
    """-> (e_got <= bar, bar); the error reached, the fp32 oracle's and the bar applied go to tests.errlog"""
    from tests.errlog import record
    b = bar(e_ref, e_white, factor)
    record("dft_truth %s | fp32 ref %.3e white %.3e" % (name, e_ref, e_white), 1.0 + float(e_got), 1.0, b)
    return bool(e_got <= b), b


def spectrum_errors(x, truth):
    return e_rms(x, truth), e_max(x, truth)


def check_spectrum(name, got, ref32, truth, white):
    """THE bar of the spectrum comparisons: got (the transform under test) and ref32 (the oracle's prec=0 on the same input)
    against truth; white = (e_rms, e_max) of the oracle's prec=0 on the family's white-noise input at this length.
    -> list of failures (empty: inside the bar), each (metric, error, bar)."""
    failures = []
    for k, metric in enumerate(("e_rms", "e_max")):
        eg, er = spectrum_errors(got, truth)[k], spectrum_errors(ref32, truth)[k]
        ok, b = judge("%s %s" % (name, metric), eg, er, white[k])
        if not ok:
            failures.append((metric, eg, b))
    return failures


def passes_old_bar(got, want):
    """the parity tests' bar: 1e-5 of the spectrum's maximum"""
    return e_max(got, want) < OLD_BAR


# ---- inputs of a transform (exact complex64) --------------------------------------------------------------------------------
def white(n, seed, amp=1.0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * amp).astype(c64)


def carrier_noise(n, k, seed, down_db=60.0, amp=1.0):
    """an exact-bin carrier (bin k of n) plus white noise down_db below it"""
    t = np.arange(n)
    return (amp * np.exp(2j * np.pi * ((k * t) % n) / n) + white(n, seed, amp * 10 ** (-down_db / 20) / np.sqrt(2)).astype(c128)).astype(c64)


def dc(n, val=0.75 - 0.5j):
    return np.full(n, val, c64)


def alternating(n, val=0.75 - 0.5j):
    return (np.where(np.arange(n) & 1, -1.0, 1.0) * val).astype(c64)


def impulse(n, idx, val=1.0 + 0.5j):
    x = np.zeros(n, c64)
    x[idx] = val
    return x


def lines(n, bins, amps, phases):
    """a spectrum (or a sequence) that is zero except at `bins`"""
    x = np.zeros(n, c64)
    for b, a, p in zip(bins, amps, phases):
        x[b % n] = c64(a * np.exp(1j * p))
    return x


def digit_indices(radix=4, sub=4096):
    """index r + radix * q for every residue r and q in {0, 1, 15, 16, 255, 256, sub - 1}: the first, the last and a carry
    value of each radix-16 digit of the sub-transform's index, every residue of the split -> every table the passes read"""
    return [(r, q, r + radix * q) for q in (0, 1, 15, 16, 255, 256, sub - 1) for r in range(radix)]


# ---- int16 blocks for the acquisition front end ----------------------------------------------------------------------------
# Sample() of the IQ front end multiplies sample i by (-j)^i and decimates by four through two 31-tap half-band filters
# (oracle/kiwi_oracle.c, ko_sample_iq16_n); these build the block so that the DECIMATED sequence, the transform's input, is the
# named signal.
def _premix(z_re, z_im):
    """(z * j^i) as int16 pairs, exact: the front end's (-j)^i gives z back"""
    i = np.arange(z_re.size) & 3
    re = np.select([i == 0, i == 1, i == 2], [z_re, -z_im, -z_re], z_im)
    im = np.select([i == 0, i == 1, i == 2], [z_im, z_re, -z_im], -z_re)
    out = np.empty(2 * z_re.size, np.int16)
    out[0::2], out[1::2] = re, im
    return out


def iq16_noise(nsamples, seed, amp=3000.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.standard_normal(2 * nsamples) * amp), -32767, 32767).astype(np.int16)


def iq16_tone(nsamples, cycles_per_sample, seed=None, amp=12000.0, down_db=60.0):
    """a carrier of `cycles_per_sample` (at the input rate, after the front end's mix), plus noise down_db below it when seeded"""
    t = np.arange(nsamples)
    z = amp * np.exp(2j * np.pi * np.mod(cycles_per_sample * t, 1.0))
    if seed is not None:
        rng = np.random.default_rng(seed)
        z = z + (rng.standard_normal(nsamples) + 1j * rng.standard_normal(nsamples)) * amp * 10 ** (-down_db / 20) / np.sqrt(2)
    return _premix(np.rint(z.real).astype(np.int64), np.rint(z.imag).astype(np.int64))


def iq16_carrier(nsamples, fft_len, k, seed):
    """bin k of the fft_len-point transform of the decimated sequence, noise 60 dB down"""
    return iq16_tone(nsamples, k / (4.0 * fft_len), seed)


def iq16_dc(nsamples):
    return iq16_tone(nsamples, 0.0)


def iq16_alternating(nsamples):
    """1/8 cycle per input sample = the Nyquist frequency of the decimated sequence.  The int16 rounding of an 8-periodic
    sequence is 8-periodic, so the decimated sequence is exactly 2-periodic until the block ends."""
    return iq16_tone(nsamples, 0.125)


# input sample 4 t + 45 reaches decimated index t through the centre tap of both half-band filters and through no other tap
# (every other odd tap is zero): the decimated sequence is a single non-zero entry
IMPULSE_DELAY = 45


def iq16_impulse(nsamples, t, val=(20000, -12000)):
    """zero except one pair.  The pair that makes decimated entry t the only non-zero one, where the block holds it; for a t
    beyond that (the block's last entries are reached through outer taps only) the pair 4 t, whose response ENDS at t.
    -> (block, pure)"""
    i, pure = 4 * t + IMPULSE_DELAY, True
    if i >= nsamples:
        i, pure = 4 * t, False
        assert i < nsamples
    z_re, z_im = np.zeros(nsamples, np.int64), np.zeros(nsamples, np.int64)
    z_re[i], z_im[i] = val
    return _premix(z_re, z_im), pure


def acq_impulse_indices(nsamples, fft_len, radix):
    """[(t, pure)]: the decimated indices digit_indices() names, as far as a block of nsamples reaches.  A 10 ms block of
    163 680 samples ends at decimated index 40 919 of 65 536 and the front end pads the rest with zeros: no sample can put
    energy at q = 4095 there, and the block's last full group of residues stands in for it."""
    out = []
    for r, q, t in digit_indices(radix, fft_len // radix):
        if 4 * t >= nsamples:
            t = radix * ((nsamples // 4) // radix - 1) + r
        out.append((t, 4 * t + IMPULSE_DELAY < nsamples))
    return out


# ---- the correlators: truth of one (SV, Doppler) cell ----------------------------------------------------------------------
def cell_truth(data, code, dop, limit):
    """Correlate()'s cell in float64 on the exact complex64 spectra: conj(data[i]) * code[(i - dop) mod N], the backward
    transform, |y|^2 over [0, limit).  For dop < 0 the last |dop| products read the NEXT row of the code table (oracle/
    kiwi_oracle.c, correlate_cell), which these tests leave unwritten: zeros.
    -> dict(max_pwr, tot_pwr, idx, gap: relative distance of the top two powers, 1.0 for a single lag, peak: the largest
    power of the WHOLE backward transform)"""
    n = data.size
    c = np.asarray(code).astype(c128)[(np.arange(n) - dop) % n]
    if dop < 0:
        c[n + dop:] = 0
    pw = power(idft(np.conj(np.asarray(data).astype(c128)) * c))
    peak = float(pw.max())
    pw = pw[:limit]
    i = int(np.argmax(pw))
    if limit > 1:
        a, b = np.partition(pw, -2)[-2:]
        gap = float((b - a) / b) if b > 0 else 0.0
    else:
        gap = 1.0
    return dict(max_pwr=float(pw[i]), tot_pwr=float(np.sum(pw)), idx=i, gap=gap, peak=peak)


# A scalar power is compared where the truth exceeds this fraction of the largest power of its transform.  A transform's error
# is absolute -- e_rms of the output's rms at every lag -- so a lag a hundred times below the peak in power shows it ten times
# enlarged, and the yardstick there is ONE draw of the oracle's own error, not its size: on the first GPU run a single-lag window
# fell on a lag 40 times below the rms, where the kernel was 1.4e-7 of the rms off (the oracle's e_rms) and the oracle, by chance,
# 1.2e-8.  Windows that hold the peak are never left out.
POWER_FRAC = 1e-2


def power_errors(cells, truth, key):
    """|got / truth - 1| of cells[key] per cell, NaN where the truth is below POWER_FRAC of its transform's peak"""
    e = np.array([abs(float(cells[key][i]) / t[key] - 1.0) if t[key] > POWER_FRAC * t["peak"] else np.nan
                  for i, t in enumerate(truth)])
    return e


def cells_truth(data, code, limit, dop_lo=-2, dop_hi=2):
    return [cell_truth(data, code, d, limit) for d in range(dop_lo, dop_hi + 1)]


def scene_spectra(n, seed):
    """a noisy scene spectrum against a real code spectrum: the data is the code delayed and Doppler-shifted under noise"""
    rng = np.random.default_rng(seed)
    code = (rng.standard_normal(n) * 60.0).astype(np.float32).astype(c64)
    k = np.arange(n)
    delay, shift = int(rng.integers(0, 4000)), int(rng.integers(-2, 3))
    data = np.roll(code.astype(c128), shift) * np.exp(2j * np.pi * ((k * delay) % n) / n) * 0.05 \
        + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 40.0
    return data.astype(c64), code


def line_spectra(n, bins, seed):
    """a product spectrum of len(bins) lines: data holds the lines, the code spectrum is real and smooth, so every Doppler
    cell sees the same lines with other weights.  |y[n]|^2 is the lines' interference pattern."""
    rng = np.random.default_rng(seed)
    amps = 100.0 * (1.0 + rng.random(len(bins)))
    data = lines(n, bins, amps, rng.random(len(bins)) * 2 * np.pi)
    k = np.arange(n)
    code = (1.0 + 0.5 * np.cos(2 * np.pi * k * 3 / n) + 0.25 * np.sin(2 * np.pi * k * 7 / n)).astype(np.float32).astype(c64)
    return data, code


# Three lines out of digit_indices() whose interference pattern has ONE top: such a pattern returns to within (2 pi q / n)^2 of
# its maximum wherever q times every line distance is near a multiple of n, and the digit positions lie close to multiples of
# n / 16, so most triples tie.  These are the ones (of 150 drawn) whose top two powers stay furthest apart over the five Doppler
# cells and the windows 4092 and n; tests/test_dft_truth_cpu.py holds the count of cells that still tie.
THREE_LINES = {
    16384: [(64, 1020, 1025), (4, 61, 1022), (6, 1024, 1025), (65, 67, 1022), (0, 60, 1021), (66, 1020, 1021), (65, 1020, 1024),
            (63, 66, 1021), (0, 65, 1022), (67, 1020, 1025), (7, 64, 1027), (0, 65, 1027), (3, 64, 1025), (64, 67, 1024),
            (65, 1024, 16380), (7, 63, 1026), (7, 63, 1020), (63, 1024, 16380), (4, 64, 1021), (0, 1022, 1027)],
    65536: [(250, 4086, 4087), (4109, 4110, 65522), (28, 4087, 4096), (253, 269, 4087), (28, 4101, 65526), (23, 4111, 65526),
            (258, 4087, 4102), (9, 4086, 65523), (240, 4086, 4110), (263, 4080, 4108), (7, 254, 4099), (4083, 4105, 65524),
            (260, 264, 4100), (10, 4083, 65525), (242, 4094, 65526), (250, 269, 65532), (4108, 65525, 65529), (264, 271, 4091),
            (10, 240, 4096), (15, 4107, 65530)],
}


def two_lines(n, radix):
    """every digit position once as the first line; the second five or nine places on in that list (a neighbour, a far one)"""
    t = [i for _, _, i in digit_indices(radix, n // radix)]
    return [(t[i], t[(i + (5 if i & 1 else 9)) % len(t)]) for i in range(0, len(t), max(1, radix // 4))]


def corr_limits(n):
    """the three production windows -- the C/A code period, the E1B code period, the whole transform (the entry point takes
    at most 16 384 lags at either length) -- and two short ones, so that single lags are read"""
    return (4092, 16368, 16384, 1, 17)


@functools.lru_cache(maxsize=None)
def corr_inputs(n, radix):
    """[(name, kind, data, code)]: what family B sends through a correlator of length n"""
    out = [("scene%d" % s, "scene", *scene_spectra(n, 4000 + s)) for s in range(4)]
    out += [("2line-%d-%d" % b, "2line", *line_spectra(n, b, 4100 + sum(b) % 1000)) for b in two_lines(n, radix)]
    out += [("3line-%d-%d-%d" % b, "3line", *line_spectra(n, b, 4200 + sum(b) % 1000)) for b in THREE_LINES[n]]
    return out


def index_checked(kind, limit):
    """A two-line pattern is periodic, or flat at its top to (2 pi / n)^2: over a long window its peak index is no property of
    the transform.  Over 1 and 17 lags it is."""
    return kind != "2line" or limit <= 17


# ---- CFastFIR: overlap-save in complex128 ------------------------------------------------------------------------------------
def fir_truth(coef, x):
    """ProcessData (oracle/kiwi_oracle_snd.c) on whole 512-sample hops of x with exactly the float spectrum `coef`"""
    coef = np.asarray(coef).astype(c128)
    x = np.asarray(x).astype(c128)
    prev, out = np.zeros(512, c128), []
    for h in range(x.size // 512):
        cur = x[512 * h:512 * (h + 1)]
        out.append(idft(dft(np.concatenate([prev, cur])) * coef)[512:])
        prev = cur
    return np.concatenate(out)


def fir_inputs(n=2048):
    t = np.arange(n)
    out = [("noise", white(n, 77, 3000.0)),
           ("carrier", (2500.0 * np.exp(2j * np.pi * ((37 * t) % 1024) / 1024)).astype(c64))]
    for s in (0, 511, 512):
        out.append(("impulse%d" % s, impulse(n, 512 + s, 2000.0 - 1500.0j)))
    return out


def fir_allpass():
    """constant magnitude 2^-10: the backward transform of the forward one, scaled to the input"""
    return np.full(1024, 2.0 ** -10, c64)


# ---- waterfall frames (int16 [8192, 2]) --------------------------------------------------------------------------------------
def wf_noise(seed, dbfs=-30.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.standard_normal((8192, 2)) * 32767 * 10 ** (dbfs / 20) / np.sqrt(2)), -32767, 32767).astype(np.int16)


def wf_tones(tones):
    """[(bin, dBFS)] exact-bin tones, int16-rounded"""
    t = np.arange(8192)
    z = sum(32767 * 10 ** (db / 20) * np.exp(2j * np.pi * ((b * t) % 8192) / 8192) for b, db in tones)
    iq = np.empty((8192, 2), np.int16)
    iq[:, 0], iq[:, 1] = np.rint(z.real), np.rint(z.imag)
    return iq


def wf_pwr_truth(samps, fft_used, dc_bins, comp=None):
    """compute_frame()'s pwr[] (oracle/kiwi_oracle_wf.c): |X[i]|^2, the first dc_bins zero, X[i] * comp[i] where compensated"""
    X = dft(samps)[:fft_used]
    if comp is not None:
        X = X * np.asarray(comp[:fft_used], np.float64)
    p = power(X)
    p[:dc_bins] = 0
    return p
