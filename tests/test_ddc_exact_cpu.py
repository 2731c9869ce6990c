"""The DDC oracle (oracle/kiwi_oracle_ddc.c) against the exact-integer model of tests/ddc_exact.py, and proof that the model can fail.

The oracle is a hand restatement of verilog/rx/{iq_mixer,cic_prune_var,rx}.v, cic_*.vh and fir_iq.sv, and the kernels were written
from the same reading, so bit-exact agreement of the two (tests/test_ddc_gpu.py) cannot see a misreading both share.  The model depends
on no register width: N running sums of length R, sampled every R inputs, as a rational.  A faithful pruned form stays within a
worst-case distance of it that follows from where how many bits are dropped; every output of the oracle must (hard assertion), the rms
of its distance must be what a white-noise model of the dropped bits predicts, and for R = 1 the two must be equal.

A bound that nothing can break proves nothing: ten misreadings of the Verilog are applied to the MODEL, one at a time, and the oracle
must then miss the bound by at least 4x.

`python -m tests.test_ddc_exact_cpu` prints the report kept in profiles/ddc_exact_model.txt."""
import math

import numpy as np
import pytest

from tests import ddc_exact as dx

MIN_EXCESS = 4.0
_got = {}


def oracle_wf(ko, log2r):
    if ("wf", log2r) not in _got:
        out, _ = ko.ddc_wf(dx.wf_case_stream(), dx.wf_case_inc(log2r), log2r)
        _got["wf", log2r] = (out[:, 0].tolist(), out[:, 1].tolist())
    return _got["wf", log2r]


def oracle_rx_raw(ko, mode, ch):
    if ("rx", mode, ch) not in _got:
        _got["rx", mode, ch] = ko.ddc_rx(dx.rx_case_stream(mode), dx.inc_for(dx.RX_INCS[ch]), mode=mode)[0]
    return _got["rx", mode, ch]


def test_nco_table_is_the_rounded_cosine_everywhere(oracle):
    """round(16383 cos / sin(2 pi a / 8192)) from float64, safe because no entry is near a tie -- equal to the oracle's table and to
    the one the kernels are given (kg_ddc_nco_table, a host function)."""
    import ctypes as C
    from flydog_sdr_gps_amd import load_library
    assert dx.nco_tie_margin() > 1e-4                       # 2.9e-4: float64's 1e-12 cannot flip a rounding
    c, s = dx.nco_table()
    oc, os_ = oracle.ddc_nco_table()
    assert np.array_equal(c, oc) and np.array_equal(s, os_)
    kc, ks = np.empty(8192, np.int16), np.empty(8192, np.int16)
    assert load_library().kg_ddc_nco_table(kc.ctypes.data_as(C.c_void_p), ks.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(c, kc) and np.array_equal(s, ks)


def test_model_denominators_follow_from_the_generator_output():
    """R^5 2^8 is 2^(bits dropped - pre-shift); the audio chain's 2^(acc - 18), 4 or 1, 2^18."""
    wf1 = dx._cic["cic_wf1"]
    assert sum(wf1["trunc"]) == 73 and dx.wf_shift(13) == 0
    for log2r in range(1, 14):
        assert (1 << log2r) ** 5 * 2 ** 8 == 2 ** (sum(wf1["trunc"]) - dx.wf_shift(log2r))
    for mode, (c1, c2, _) in dx.RX_MODES.items():
        e1, e2 = dx._cic[c1], dx._cic[c2]
        assert sum(e1["trunc"]) == e1["acc"] - 18 and 2 ** sum(e2["trunc"]) == (1 if mode == dx.RX_WIDE else 4)
        assert dx.rx_decim(mode) == e1["R"] * e2["R"] * 2
    assert [len(dx.signed_taps(m)) for m in (dx.RX_STD, dx.RX_WIDE, dx.RX_14)] == [65, 65, 17]


def test_bounds_are_derived_and_of_the_expected_size():
    """Sanity of the derivation itself: below R = 256 the bound is about one lsb, it doubles per octave once the 61 bits dropped behind
    the fourth integrator are all live (33 lsb at R = 8192), and the audio chain's is a few thousandths of its output amplitude."""
    b = {l: float(dx.worst_case_bound("wf", l)) for l in range(14)}
    assert b[0] == 0 and all(1.0 < b[l] < 1.25 for l in range(1, 6)) and 33.0 < b[13] < 33.2
    assert all(b[l] < b[l + 1] for l in range(1, 13)) and abs((b[13] - b[1]) / (b[12] - b[1]) - 2.0) < 0.07
    assert [round(float(dx.worst_case_bound("rx", m))) for m in (dx.RX_STD, dx.RX_WIDE, dx.RX_14)] == [2043, 933, 1098]


@pytest.mark.parametrize("log2r", dx.WF_LOG2R)
def test_oracle_waterfall_is_within_the_worst_case_of_the_exact_model(oracle, log2r):
    gi, gq = oracle_wf(oracle, log2r)
    exact = dx.wf_case_exact(log2r)
    dx.check_case("wf", log2r, gi, gq, exact)
    if log2r == 0:
        assert gi == exact[0] and gq == exact[1]
    assert max(abs(v) for v in gi[8:]) > 5000                # the strong tone came through


@pytest.mark.parametrize("mode", [dx.RX_STD, dx.RX_WIDE, dx.RX_14])
def test_oracle_audio_chain_is_within_the_worst_case_of_the_exact_model(oracle, mode):
    for ch in range(2):
        raw = oracle_rx_raw(oracle, mode, ch)
        assert raw.size == 6 * dx.RX_RECORDS
        gi, gq = dx.unpack_records(raw)
        dx.check_case("rx", mode, gi, gq, dx.rx_case_exact(mode, ch))
        assert max(abs(v) for v in gi[dx.RX_SKIP:]) > 300000


def test_mixer_rounding_carry_at_every_table_value_through_r1(oracle):
    """adc in {-32768, -1, 0, 1, 32767} against all 8192 cosines and sines through the R = 1 path: equal, including every product
    whose rounding bit carries."""
    adc = np.repeat(np.array([-32768, -1, 0, 1, 32767], np.int16), 8192)
    inc = 1 << 35                                            # one table entry per sample
    got, _ = oracle.ddc_wf(adc, inc, 0)
    ni, nq, den = dx.wf_exact(adc, 0, inc, 0)
    assert den == 1 and got[:, 0].tolist() == ni and got[:, 1].tolist() == nq
    mi, _ = dx.mix(adc, 0, inc, dx.WF_W)
    assert np.count_nonzero((adc.astype(np.int64) * dx.nco_table()[0][np.arange(adc.size) % 8192] * 32 >> 10) & 1) > 1000
    assert int(mi.max()) == -int(mi.min()) == 32768 * 16383 * 32 >> 11 < 1 << 23          # -32768 x -16383: still 24 bits


def measured_ratios(ko):
    """case -> rms / predicted rms of the oracle (I and Q pooled), the quantity K_RMS is set from."""
    out = {}
    for log2r in dx.WF_LOG2R[1:]:
        gi, gq = oracle_wf(ko, log2r)
        ni, nq, den = dx.wf_case_exact(log2r)
        r = [dx.distance(g, n, den, dx.WF_SKIP)[1] for g, n in ((gi, ni), (gq, nq))]
        out["wf log2r %d" % log2r] = math.sqrt((r[0] ** 2 + r[1] ** 2) / 2) / dx.predicted_rms("wf", log2r)
    for mode in dx.RX_MODES:
        for ch in range(2):
            gi, gq = dx.unpack_records(oracle_rx_raw(ko, mode, ch))
            ni, nq, den = dx.rx_case_exact(mode, ch)
            r = [dx.distance(g, n, den, dx.RX_SKIP)[1] for g, n in ((gi, ni), (gq, nq))]
            out["rx %s ch %d" % (dx.RX_NAMES[mode], ch)] = math.sqrt((r[0] ** 2 + r[1] ** 2) / 2) / dx.predicted_rms("rx", mode)
    return out


def test_rms_factor_is_one_and_a_half_times_the_largest_measured_ratio(oracle):
    worst = max(measured_ratios(oracle).values())
    assert abs(dx.K_RMS - 1.5 * worst) < 0.01 and dx.K_RMS <= 4.0, (dx.K_RMS, worst)


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
WF_MUTATIONS = [(m, l) for m in ("addr_46_34", "phase_early", "q_negated", "iq_swapped") for l in (3, 13)] + \
               [("preshift_off_by_one", l) for l in (1, 4, 9)] + [("close_one_later", l) for l in (1, 3)]
RX_MUTATIONS = [(m, mode) for m in ("fir_emits_first", "taps_other_mode", "r2_other_mode", "bytes_4_5_swapped")
                for mode in (dx.RX_STD, dx.RX_WIDE, dx.RX_14)] + \
               [(m, dx.RX_STD) for m in ("addr_46_34", "phase_early", "q_negated", "iq_swapped")]


def wf_excess(ko, mut, log2r):
    gi, gq = oracle_wf(ko, log2r)
    ni, nq, den = dx.wf_exact(dx.wf_case_stream(), 0, dx.wf_case_inc(log2r), log2r, mut=(mut,))
    bound = dx.worst_case_bound("wf", log2r)
    return max(dx.exceeds(gi, ni, den, bound), dx.exceeds(gq, nq, den, bound))


def rx_excess(ko, mut, mode):
    raw = oracle_rx_raw(ko, mode, 0)
    gi, gq = dx.unpack_records(raw, mut=(mut,))
    ni, nq, den = dx.rx_exact(dx.rx_case_stream(mode), 0, dx.inc_for(dx.RX_INCS[0]), mode, mut=(mut,))
    bound = dx.worst_case_bound("rx", mode)
    return max(dx.exceeds(gi, ni, den, bound), dx.exceeds(gq, nq, den, bound))


def test_every_mutation_is_exercised():
    assert {m for m, _ in WF_MUTATIONS + RX_MUTATIONS} == set(dx.MUTATIONS) and len(dx.MUTATIONS) == 10


@pytest.mark.parametrize("mut,log2r", WF_MUTATIONS)
def test_a_misread_waterfall_model_is_caught(oracle, mut, log2r):
    x = wf_excess(oracle, mut, log2r)
    print("wf log2r %d, model with %s: oracle is %.1f bounds away" % (log2r, mut, x))
    assert x >= MIN_EXCESS, (mut, log2r, x)


@pytest.mark.parametrize("mut,mode", RX_MUTATIONS)
def test_a_misread_audio_model_is_caught(oracle, mut, mode):
    x = rx_excess(oracle, mut, mode)
    print("rx %s, model with %s: oracle is %.1f bounds away" % (dx.RX_NAMES[mode], mut, x))
    assert x >= MIN_EXCESS, (mut, mode, x)


def report():
    from oracle import kiwi_oracle as ko
    ko.lib()
    lines = ["Exact-integer CIC model against the DDC oracle (tests/test_ddc_exact_cpu.py, tests/ddc_exact.py)",
             "max |oracle - exact| over every output of a case, in output lsbs, against the derived worst case; rms over the outputs behind",
             "the start-up (I and Q pooled) against the white-noise prediction", ""]
    fmt = "%-14s outputs %6d  max %8.3f  bound %9.3f  rms %7.4f  predicted %7.4f  ratio %.3f"
    ratios = measured_ratios(ko)
    for log2r in dx.WF_LOG2R:
        gi, gq = oracle_wf(ko, log2r)
        ni, nq, den = dx.wf_case_exact(log2r)
        worst = max(dx.distance(gi, ni, den)[0], dx.distance(gq, nq, den)[0])
        if log2r == 0:
            lines.append("%-14s outputs %6d  equal: %s" % ("wf log2r 0", len(gi), gi == ni and gq == nq))
            continue
        name = "wf log2r %d" % log2r
        pred = dx.predicted_rms("wf", log2r)
        lines.append(fmt % (name, len(gi), float(worst), float(dx.worst_case_bound("wf", log2r)), ratios[name] * pred, pred, ratios[name]))
        if log2r == 13:
            d = [float((g * den - n) / den) for g, n in zip(gi[:4], ni[:4])]
            steady = max(abs(g * den - n) / den for g, n in zip(gi[dx.WF_SKIP:] + gq[dx.WF_SKIP:], ni[dx.WF_SKIP:] + nq[dx.WF_SKIP:]))
            lines.append("%-14s first four I outputs off by %s (start-up of the truncation bias), steady-state max %.3f"
                         % ("", ", ".join("%.2f" % v for v in d), steady))
    for mode in dx.RX_MODES:
        for ch in range(2):
            gi, gq = dx.unpack_records(oracle_rx_raw(ko, mode, ch))
            ni, nq, den = dx.rx_case_exact(mode, ch)
            worst = max(dx.distance(gi, ni, den)[0], dx.distance(gq, nq, den)[0])
            name = "rx %s ch %d" % (dx.RX_NAMES[mode], ch)
            pred = dx.predicted_rms("rx", mode)
            lines.append(fmt % (name, len(gi), float(worst), float(dx.worst_case_bound("rx", mode)), ratios[name] * pred, pred, ratios[name])
                         + "  amplitude %d" % max(abs(v) for v in gi[dx.RX_SKIP:]))
    lines += ["", "largest rms ratio %.3f -> K_RMS = 1.5 x that = %.2f (tests/ddc_exact.py has %.2f)"
              % (max(ratios.values()), 1.5 * max(ratios.values()), dx.K_RMS), "",
              "sensitivity: the oracle against a model with one misreading, in multiples of the worst-case bound (at least %.0f asked)" % MIN_EXCESS]
    for mut, log2r in WF_MUTATIONS:
        lines.append("   wf log2r %-2d  %-20s %10.1f" % (log2r, mut, wf_excess(ko, mut, log2r)))
    for mut, mode in RX_MUTATIONS:
        lines.append("   rx %-4s      %-20s %10.1f" % (dx.RX_NAMES[mode], mut, rx_excess(ko, mut, mode)))
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
