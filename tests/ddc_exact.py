"""An exact-integer model of the two down-converters (waterfall: kg_ddc / ko_ddc_wf; audio: kg_rxddc / ko_ddc_rx_mode), shared by
tests/test_ddc_exact_cpu.py and tests/test_ddc_exact_gpu.py.

A CIC decimator of N stages is, in exact arithmetic, N cascaded running sums of length R sampled every R inputs; the pruned hardware
form differs from that only by the low bits it drops on the way, and the worst case of what those drops can do to an output follows from
the structure alone (Hogenauer): an error e[n] injected at a point reaches the output through the impulse response h of what FOLLOWS
that point, so |sum h e| <= max|e| * sum|h|.  This module computes the exact value as a rational (Python int numerator, one
denominator), the worst-case distance a faithful hardware form may have from it, and the rms distance a white-noise model of the
dropped bits predicts.  It models no register width, wrap or comb width: the only structural numbers it reads are HOW MANY bits are
dropped WHERE (tests/golden/cic_ref.json, the output of the reference's own generator), and those enter the bound only, never the value.

Python int / fractions.Fraction throughout; numpy int64 where the true value provably fits (stated at each use).  Nothing is imported
from oracle/ or from the product."""
import json
import math
import os
from fractions import Fraction

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M48 = (1 << 48) - 1
NCO_AMPL = 16383                     # 15-bit DDS output, symmetric
NCO_ADDR_BITS = 13
WF_W, RX_W = 24, 22                  # mixer OUT_WIDTH of the waterfall / the audio instance
WF_N = 5
RX_STD, RX_WIDE, RX_14 = 0, 1, 2
# mode -> (rx1 CIC, rx2 CIC, index into fir_iq.sv's tap tables in file order: RX_CFG == 3, RX_CFG == 14, default)
RX_MODES = {RX_STD: ("cic_rx1_12k", "cic_rx2_12k", 2), RX_WIDE: ("cic_rx1_20k", "cic_rx2_20k", 0), RX_14: ("cic_rx1_12k", "cic_rx2_12k", 1)}
RX_NAMES = {RX_STD: "std", RX_WIDE: "wide", RX_14: "rx14"}
FIR_COEFF_BITS = 18
# sensitivity mutations (tests/test_ddc_exact_cpu.py): each one is a plausible misreading of the Verilog, applied to the MODEL
MUTATIONS = ("addr_46_34", "phase_early", "q_negated", "iq_swapped", "preshift_off_by_one", "close_one_later",
             "fir_emits_first", "taps_other_mode", "r2_other_mode", "bytes_4_5_swapped")
# the nearest wrong table for each mode: std and wide differ by about 2 % per tap, which only a strong tone lifts over 4 bounds
OTHER_TAPS = {RX_STD: RX_WIDE, RX_WIDE: RX_STD, RX_14: RX_STD}
OTHER_R2 = {RX_STD: RX_WIDE, RX_WIDE: RX_STD, RX_14: RX_WIDE}
# rms assertion: measured rms <= K_RMS * predicted_rms.  1.5 x the largest ratio the oracle showed over every case of the CPU report
# (profiles/ddc_exact_model.txt, asserted by test_rms_factor_is_one_and_a_half_times_the_largest_measured_ratio).  A factor above 4
# would mean the noise model is wrong and has to be mended, not the factor widened: two such mends are in predicted_rms (one response
# from a drop to the final output; the means the final slices leave), after which the long-run ratio is 0.95 .. 1.02 and what is left
# is the scatter of 28 correlated values per audio channel.
K_RMS = 1.83                         # 1.5 x 1.218 (rx wide, channel 0)

_cic = json.load(open(os.path.join(GOLD, "cic_ref.json")))
_taps = json.load(open(os.path.join(GOLD, "ref_text_pins.json")))["fir_iq_sv"]["tap_sets"]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def stream(n, seed, tones, noise=40.0):
    """int16 ADC samples: tones (cycles/sample, amplitude) at random phases plus white noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n)
    x = rng.normal(0, noise, n)
    for f, a in tones:
        x = x + a * np.cos(2 * np.pi * f * t + rng.random() * 6)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def inc_for(f):
    """f cycles/sample as a 48-bit phase increment."""
    return int(round(f * 2 ** 48)) & M48


# ---- NCO and mixer ----------------------------------------------------------------------------------------------------------------
def nco_table():
    """(cos, sin) int16[8192]: round(16383 cos / sin(2 pi a / 8192)).  No entry is nearer than nco_tie_margin() to a rounding tie, so
    float64 trigonometry decides every rounding safely."""
    a = 2.0 * np.pi * np.arange(1 << NCO_ADDR_BITS) / (1 << NCO_ADDR_BITS)
    return np.rint(NCO_AMPL * np.cos(a)).astype(np.int16), np.rint(NCO_AMPL * np.sin(a)).astype(np.int16)


def nco_tie_margin():
    a = 2.0 * np.pi * np.arange(1 << NCO_ADDR_BITS) / (1 << NCO_ADDR_BITS)
    v = np.concatenate([NCO_AMPL * np.cos(a), NCO_AMPL * np.sin(a)])
    return float(np.abs(np.abs(v - np.floor(v)) - 0.5).min())


def mix(adc, phase0, inc, width, mut=()):
    """-> (I, Q) int64: floor(adc * dds * 32 / 2^(35 - width) + 1/2), dds = cos (I) and sin (Q) of phase bits 47:35, the phase being
    phase0 + n inc mod 2^48 for sample n (it advances after the sample is used).
    int64: |adc dds 32| <= 2^15 * 2^14 * 2^5 = 2^34.  uint64 phase arithmetic wraps modulo 2^64, a multiple of 2^48: exact."""
    adc = np.asarray(adc, np.int16).astype(np.int64)
    n = np.arange(adc.size, dtype=np.uint64) + np.uint64(1 if "phase_early" in mut else 0)
    ph = (np.uint64(phase0 & M48) + n * np.uint64(inc & M48)) & np.uint64(M48)
    lo = 34 if "addr_46_34" in mut else 48 - NCO_ADDR_BITS
    addr = ((ph >> np.uint64(lo)) & np.uint64((1 << NCO_ADDR_BITS) - 1)).astype(np.int64)
    c, s = nco_table()
    sh = 35 - width
    i = (adc * c[addr].astype(np.int64) * 32 + (1 << (sh - 1))) >> sh          # >> of int64 is floor
    q = (adc * s[addr].astype(np.int64) * 32 + (1 << (sh - 1))) >> sh
    if "q_negated" in mut:
        q = -q
    if "iq_swapped" in mut:
        i, q = q, i
    return i, q


# ---- exact running sums -----------------------------------------------------------------------------------------------------------
def boxcar_power(r, n):
    """Impulse response of n cascaded running sums of length r, as Python ints (object array), length n (r - 1) + 1."""
    h = np.array([1], object)
    for _ in range(n):
        cs = np.cumsum(np.concatenate([h, np.zeros(r - 1, object)]))
        h = cs - np.concatenate([np.zeros(r, object), cs])[:cs.size]
    return h


def _absmax(v):
    return max((abs(int(x)) for x in (v.max(), v.min())), default=0) if len(v) else 0


def decimated_sums(x, h, r):
    """y[k] = sum_j h[j] x[r k + r - 1 - j] with zero history, k < len(x) // r, as a list of Python ints.
    Evaluated as len(h) / r block products; in int64 where len(h) max|h| max|x| < 2^63 (no partial sum can leave the type), else in
    Python ints."""
    x = np.asarray(x)
    nb, k = -(-len(h) // r), len(x) // r
    if k == 0:
        return []
    fits = len(h) * _absmax(h) * _absmax(x) < 2 ** 63
    dt = np.int64 if fits else object
    hp = np.zeros(nb * r, dt)
    hp[:len(h)] = h
    hrev = hp[::-1]
    xp = np.zeros((nb - 1 + k) * r, dt)
    xp[(nb - 1) * r:] = x[:k * r]
    blk = xp.reshape(nb - 1 + k, r)
    y = sum(blk[b:b + k].dot(hrev[b * r:(b + 1) * r]) for b in range(nb))
    return [int(v) for v in y]


# ---- waterfall channel ------------------------------------------------------------------------------------------------------------
def wf_exact(adc, phase0, inc, log2r, mut=()):
    """-> (num_i, num_q, den): output k of a waterfall channel of decimation R = 2^log2r is num[k] / den exactly.
    R >= 2: five running sums of length R from zero history, taken at input R k + R - 1, over R^5 2^8 (the pre-shift normalises the
    gain to 2^65 and 73 bits are dropped on the way to 16: 2^8 = 2^(73 - 65)).  R = 1: floor(m / 2^8), den 1, and the hardware must
    EQUAL it."""
    mi, mq = mix(adc, phase0, inc, WF_W, mut)
    if log2r == 0:
        return [int(v) for v in mi >> 8], [int(v) for v in mq >> 8], 1
    r = 1 << log2r
    if "close_one_later" in mut:
        mi, mq = mi[1:], mq[1:]
    h = boxcar_power(r, WF_N)
    den = r ** WF_N * 2 ** 8
    if "preshift_off_by_one" in mut:
        den //= 2
    return decimated_sums(mi, h, r), decimated_sums(mq, h, r), den


# ---- audio chain ------------------------------------------------------------------------------------------------------------------
def signed_taps(mode):
    """The NT symmetric coefficients of a mode as signed Python ints, from the committed pin of fir_iq.sv's 18-bit tables."""
    half = [v - (1 << FIR_COEFF_BITS) if v >= 1 << (FIR_COEFF_BITS - 1) else v for v in _taps[RX_MODES[mode][2]]]
    return half + half[-2::-1]


def rx_decim(mode):
    c1, c2, _ = RX_MODES[mode]
    return _cic[c1]["R"] * _cic[c2]["R"] * 2


def rx_exact(adc, phase0, inc, mode, mut=()):
    """-> (num_i, num_q, den): record k of an audio channel carries floor-or-so of num[k] / den.
    rx1: three running sums at R1 over 2^(acc - 18); rx2: five at R2 over 4 (std, rx14) or 1 (wide); the symmetric FIR over 2^18,
    emitting on the second of every two inputs.  All linear, so one numerator over the product of the three denominators."""
    c1, c2, _ = RX_MODES[mode]
    e1 = _cic[c1]
    e2 = _cic[c2 if "r2_other_mode" not in mut else RX_MODES[OTHER_R2[mode]][1]]
    taps = signed_taps(mode if "taps_other_mode" not in mut else OTHER_TAPS[mode])
    den = 2 ** (e1["acc"] - e1["Bout"]) * 2 ** (e2["acc"] - e2["Bout"]) * 2 ** FIR_COEFF_BITS
    out = []
    for m in mix(adc, phase0, inc, RX_W, mut):
        s1 = decimated_sums(m, boxcar_power(e1["R"], e1["N"]), e1["R"])          # int64: 3 R1 * R1^2 * 2^21 < 2^63
        s2 = decimated_sums(np.array(s1, object), boxcar_power(e2["R"], e2["N"]), e2["R"])
        if "fir_emits_first" in mut:
            s2 = [0] + s2
        out.append(decimated_sums(np.array(s2, object), np.array(taps, object), 2))
    return out[0], out[1], den


def unpack_records(raw, mut=()):
    """6-byte records {u16 i, u16 q, u8 q3, u8 i3} -> (I, Q) lists of signed 24-bit Python ints."""
    b = np.asarray(raw, np.uint8).reshape(-1, 6).astype(np.int64)
    hi_i, hi_q = (4, 5) if "bytes_4_5_swapped" in mut else (5, 4)
    i = b[:, 0] | b[:, 1] << 8 | b[:, hi_i] << 16
    q = b[:, 2] | b[:, 3] << 8 | b[:, hi_q] << 16
    sx = lambda v: [int(x) - (1 << 24) if x >= 1 << 23 else int(x) for x in v]          # noqa: E731
    return sx(i), sx(q)


# ---- what the dropped bits can do -------------------------------------------------------------------------------------------------
def _drop_points(e, r, shift=0):
    """For a pruned CIC e (cic_ref.json entry) run at decimation r with its input pre-shifted by `shift` bits: one
    (e_max, step, h, at_input_rate) per point where low bits are dropped, e_max and step in units of the OUTPUT lsb, plus the kind of
    the final slice ("round", "floor" or None).
    trunc[] lists the bits dropped at the input of integrator 1..N, of comb 1..N and at the output.  Before the drop at point p the
    register's lsb weighs 2^(bits dropped earlier); B dropped bits leave an error of 0 .. 2^B - 1 of them -- 0 .. 2^B - 2^z when the
    low z bits are known to be zero because the input was shifted up (step is the 2^B of the uniform-noise model).  h is the exact
    impulse response from the point to the output: into integrator i (j = i - 1 integrators before it) it is
    boxcar_r^(N - j) (1 - z^-r)^j at the input rate, before comb k it is (1 - z^-1)^(combs that remain) at the output rate."""
    n, trunc = e["N"], e["trunc"]
    total = sum(trunc)
    pts, before = [], 0
    for p, bits in enumerate(trunc[:2 * n]):
        if bits:
            z = min(bits, max(0, shift - before))
            emax = (1 << bits) - (1 << z)
            if p < n:                                        # input of integrator p + 1
                box = boxcar_power(r, n - p)
                h = np.zeros(box.size + p * r, object)
                for k in range(p + 1):
                    h[k * r:k * r + box.size] += (-1) ** k * math.comb(p, k) * box
            else:                                            # input of comb p - n + 1
                left = 2 * n - p
                h = np.array([(-1) ** k * math.comb(left, k) for k in range(left + 1)], object)
            w = Fraction(1 << before, 1 << total)
            pts.append((emax * w, (1 << bits) * w, h, p < n))
        before += bits
    last = trunc[2 * n]
    return pts, ("round" if e["out"][3] >= 0 else "floor") if last else None


def _cic_bound(e, r, shift=0):
    pts, fin = _drop_points(e, r, shift)
    b = sum((emax * sum(abs(int(v)) for v in h) for emax, _, h, _ in pts), Fraction(0))
    return b + (Fraction(1, 2) if fin == "round" else 1 if fin == "floor" else 0)


def _cic_var(e, r, shift=0, tail=(1.0,)):
    """White-noise model: a drop of B bits is uniform noise of variance 2^(2B) / 12 lsb^2, independent from sample to sample; the
    means do not matter behind a comb (zero gain at DC).  `tail` is the impulse response of what follows this CIC, at its output rate
    and in final lsbs per lsb of this CIC's output: what a drop inside the CIC does to the final output goes through h AND tail as ONE
    response (sum h^2 * sum tail^2 would treat the noise as white again behind the CIC, which a low-pass behind a low-pass is far from).
    -> variance in final lsbs^2."""
    pts, fin = _drop_points(e, r, shift)
    tail = np.asarray(tail, np.float64)
    v = 0.0
    for emax, step, h, at_input_rate in pts:
        if not emax:
            continue
        h = h.astype(np.float64)
        if at_input_rate:                                    # tail acts on every r-th sample of the input rate
            c = np.zeros(h.size + (tail.size - 1) * r)
            for k, t in enumerate(tail):
                c[k * r:k * r + h.size] += t * h
        else:
            c = np.convolve(h, tail)
        v += float(step) ** 2 / 12 * float(np.sum(c * c))
    return v + (float(np.sum(tail * tail)) / 12 if fin else 0.0)


def wf_shift(log2r):
    """The variable pre-shift: what is left of the accumulator above the input and the growth of this R."""
    e = _cic["cic_wf1"]
    return e["acc"] - (e["Bin"] + e["N"] * log2r)


def worst_case_bound(kind, arg):
    """Largest |hardware output - exact value| a faithful pruned form can show, in output lsbs, as a Fraction.
    ("wf", log2r): the sum over the drop points, + 1/2 for the final round-half-up (0 for R = 1: equality).
    ("rx", mode): rx1's bound times rx2's gain sum|boxcar^5| / 2^(acc - Bout), + 1/2 where rx2 rounds, times sum|taps| / 2^18, + 1 for
    the FIR's floor."""
    if kind == "wf":
        return Fraction(0) if arg == 0 else _cic_bound(_cic["cic_wf1"], 1 << arg, wf_shift(arg))
    c1, c2, _ = RX_MODES[arg]
    e1, e2 = _cic[c1], _cic[c2]
    g2 = Fraction(sum(int(v) for v in boxcar_power(e2["R"], e2["N"])), 2 ** (e2["acc"] - e2["Bout"]))
    b2 = _cic_bound(e1, e1["R"]) * g2 + _cic_bound(e2, e2["R"])
    return b2 * Fraction(sum(abs(t) for t in signed_taps(arg)), 2 ** FIR_COEFF_BITS) + 1


def _final_mean(e):
    """Mean of (output - exact) that a CIC's final slice leaves when the dropped B bits are uniform: rounding half up 2^-(B + 1),
    plain truncation -(2^B - 1) / 2^(B + 1).  Unlike the means of the drops inside (zero gain at DC behind a comb) it stays."""
    bits = e["trunc"][2 * e["N"]]
    if not bits:
        return 0.0
    return 2.0 ** -(bits + 1) if e["out"][3] >= 0 else -((1 << bits) - 1) / 2.0 ** (bits + 1)


def predicted_rms(kind, arg):
    """The same sums with variances: sqrt(sum 2^(2B) / 12 * sum h^2 + mean^2), in output lsbs, h running from the drop to the FINAL
    output (for the audio chain through rx2 and the FIR as one response).  The mean: each final slice leaves one (_final_mean) and what
    follows passes it on with its gain at DC -- through rx2's R2^5 / 4 that is the largest single term of the audio chain; the FIR's
    floor is uniform on (-1, 0], variance 1 / 12 and mean -1/2."""
    if kind == "wf":
        e = _cic["cic_wf1"]
        return 0.0 if arg == 0 else math.sqrt(_cic_var(e, 1 << arg, wf_shift(arg)) + _final_mean(e) ** 2)
    c1, c2, _ = RX_MODES[arg]
    e1, e2 = _cic[c1], _cic[c2]
    fir = np.array(signed_taps(arg), np.float64) / 2.0 ** FIR_COEFF_BITS                 # at rx2's output rate
    up = np.zeros((fir.size - 1) * e2["R"] + 1)
    up[::e2["R"]] = fir
    after_rx1 = np.convolve(boxcar_power(e2["R"], e2["N"]).astype(np.float64), up) / 2.0 ** (e2["acc"] - e2["Bout"])
    mean = _final_mean(e1) * after_rx1.sum() + _final_mean(e2) * fir.sum() - 0.5
    return math.sqrt(_cic_var(e1, e1["R"], tail=after_rx1) + _cic_var(e2, e2["R"], tail=fir) + 1 / 12 + mean * mean)


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def distance(got, num, den, skip=0):
    """got (ints) against num / den: -> (max |got - num/den| as a Fraction over all outputs, rms as a float over outputs skip..)."""
    assert len(got) == len(num), (len(got), len(num))
    d = [int(g) * den - n for g, n in zip(got, num)]
    worst = Fraction(max((abs(v) for v in d), default=0), den)
    tail = d[skip:]
    rms = math.sqrt(sum(v * v for v in tail) / len(tail)) / den if tail else 0.0
    return worst, rms


def exceeds(got, num, den, bound):
    """How many times the largest |got - num/den| over the outputs both have exceeds `bound` (float); a different count alone
    counts as infinitely far."""
    if len(got) != len(num) and min(len(got), len(num)) == 0:
        return math.inf
    k = min(len(got), len(num))
    worst, _ = distance(got[:k], num[:k], den)
    return float(worst / bound)


# ---- the cases both test files use (the CPU file runs the oracle on them, the GPU file the kernels) --------------------------------
# Waterfall: one stream, eight channels.  A strong tone at 0.0123 cycles/sample and a weaker one 1.5 * 2^-16 above it, so that every
# decimation up to 8192 has both inside its output band (white noise alone decimates to an amplitude of ~300 at R = 8192, too little to
# tell a mutation from the bound of 33 there); each channel's NCO sits 2^-(log2r + 3) above the strong tone -- distinct increments,
# and a baseband frequency of an eighth of the output rate, so that a one-sample slip of the closing sample shows.
WF_LOG2R = (0, 1, 2, 3, 4, 8, 9, 13)
WF_SAMPLES = 8192 * 24
WF_TONE = 0.0123
WF_SKIP = 5                          # outputs before the start-up transient of the truncation bias has left the five combs


def wf_case_stream():
    return stream(WF_SAMPLES, 1301, ((WF_TONE, 12000.0), (WF_TONE + 1.5 * 2.0 ** -16, 3000.0)), noise=60.0)


def wf_case_inc(log2r):
    return inc_for(WF_TONE + 2.0 ** -(log2r + 3))


# Audio: per mode one stream of 48 records and two channels; the strong tone 1.2e-5 cycles/sample (an eighth of the record rate) above
# channel 0's NCO and 2.0e-5 below channel 1's, a weaker one 3.5e-5 above the strong one, an out-of-band tone and noise.  The strong tone is as large as the others leave room for
# (26000 of 32767: about 9e5 at the output): the std and wide tap tables are only then 4 bounds apart.
RX_RECORDS = 48
RX_SKIP = 34                         # records before the 65-tap FIR (33 records) and the CICs ahead of it have filled
RX_INCS = (WF_TONE - 1.2e-5, WF_TONE + 2.0e-5)


def rx_case_stream(mode):
    return stream(rx_decim(mode) * RX_RECORDS, 1400 + mode, ((WF_TONE, 26000.0), (WF_TONE + 3.5e-5, 1500.0), (0.2, 3000.0)), noise=40.0)


_memo = {}


def wf_case_exact(log2r):
    """(num_i, num_q, den) of the waterfall case's channel, computed once per process."""
    if ("wf", log2r) not in _memo:
        _memo["wf", log2r] = wf_exact(wf_case_stream(), 0, wf_case_inc(log2r), log2r)
    return _memo["wf", log2r]


def rx_case_exact(mode, ch):
    if ("rx", mode, ch) not in _memo:
        _memo["rx", mode, ch] = rx_exact(rx_case_stream(mode), 0, inc_for(RX_INCS[ch]), mode)
    return _memo["rx", mode, ch]


def check_case(kind, arg, got_i, got_q, exact):
    """The assertions both files make of one channel: every output within the worst case (R = 1: equal), the rms of the outputs behind
    the start-up within K_RMS of the prediction.  -> (max error in lsbs, rms, predicted rms) for the reports."""
    num_i, num_q, den = exact
    bound, pred = worst_case_bound(kind, arg), predicted_rms(kind, arg)
    skip = WF_SKIP if kind == "wf" else RX_SKIP
    assert len(got_i) == len(num_i) and len(got_q) == len(num_q), (kind, arg, len(got_i), len(num_i))
    wi, ri = distance(got_i, num_i, den, skip)
    wq, rq = distance(got_q, num_q, den, skip)
    worst, rms = max(wi, wq), math.sqrt((ri * ri + rq * rq) / 2)
    print("%s %s: max |out - exact| %.3f lsb (bound %.3f), rms %.4f (predicted %.4f, ratio %.3f)"
          % (kind, arg, float(worst), float(bound), rms, pred, rms / pred if pred else 0.0))
    assert worst <= bound, (kind, arg, float(worst), float(bound))
    assert rms <= K_RMS * pred, (kind, arg, rms, pred, K_RMS)
    return float(worst), rms, pred
