"""The yardstick of tests/test_dft_truth_gpu.py held on the CPU, and proof that its bar can fail.

1. The oracle against the exact DFT (numpy.fft in complex128 on the same float inputs): the double transform (prec=1) is one
   float rounding per component away, the fp32 radix-4 transform (prec=0) sits where it was measured, within a factor of 2 --
   so the yardstick cannot degrade unseen.
2. Planted defects, through the oracle's FFT hook and the GPU tests' own bar function (tests.dft_truth.check_spectrum): each
   fails the new bar on at least one of the inputs the GPU tests use and passes the parity tests' 1e-5 of the maximum on all.
3. The peak-index condition of the correlator tests: how many cells it leaves out, and that the fp32 oracle finds the float64
   argmax on all the others."""
import numpy as np
import pytest

from tests import dft_truth as T

# fp32 radix-4 (prec=0) against the exact DFT on white noise: (rms relative, max relative to max), measured.  65536 is one more
# radix-4 pass than 16384's seven: sqrt(8 / 7) of that row.
PREC0 = {1024: (1.1e-7, 1.2e-7), 8192: (1.3e-7, 1.6e-7), 16384: (1.4e-7, 1.3e-7), 65536: (1.5e-7, 1.5e-7)}


def ulps(got, truth):
    """|got - truth| in units of the float spacing at truth, per component"""
    g = np.ascontiguousarray(got, np.complex64).view(np.float32).astype(np.float64)
    t = np.ascontiguousarray(truth, np.complex128).view(np.float64)
    return np.abs(g - t) / np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)


def transform_inputs(n, seed=0):
    """what the GPU families transform, as sequences of length n"""
    out = [("noise", T.white(n, 11 + seed)), ("carrier", T.carrier_noise(n, n // 8 + 3, 12 + seed)), ("dc", T.dc(n)),
           ("alternating", T.alternating(n))]
    out += [("impulse%d" % i, T.impulse(n, i)) for i in sorted({i for _, _, i in T.digit_indices(4, n // 4) if i < n})]
    return out


@pytest.mark.parametrize("n", sorted(PREC0))
def test_double_oracle_is_one_rounding_from_the_truth(oracle, n):
    for name, x in transform_inputs(n):
        for sign, truth in ((-1, T.dft(x)), (+1, T.idft(x))):
            u = ulps(oracle.fft(x, sign=sign, prec=1), truth)
            # the float64 radix-2 itself is 1e-16 of the spectrum's norm off: it can move a rounding only where a component is
            # that small against the largest
            big = np.abs(truth.view(np.float64)) > 1e-6 * np.abs(truth).max()
            assert u[big].max() <= 0.5 + 1e-6, (name, n, sign, u[big].max())


@pytest.mark.parametrize("n", sorted(PREC0))
def test_float_oracle_sits_where_it_was_measured(oracle, n):
    rms, mx = PREC0[n]
    for seed in range(3):
        x = T.white(n, 100 + seed)
        e = T.spectrum_errors(oracle.fft(x, prec=0), T.dft(x))
        assert rms / 2 <= e[0] <= rms * 2 and mx / 2 <= e[1] <= mx * 2, (n, seed, e)
        e = T.spectrum_errors(oracle.fft(x, sign=+1, prec=0), T.idft(x))
        assert rms / 2 <= e[0] <= rms * 2 and mx / 2 <= e[1] <= mx * 2, (n, seed, "backward", e)
    # impulses: 0.7-0.9e-7 rms, 1.3-2.2e-7 max (index 0 and n / 2 are exact)
    for i in (1, 5, n // 4 + 3, n - 1):
        x = T.impulse(n, i)
        e = T.spectrum_errors(oracle.fft(x, prec=0), T.dft(x))
        assert e[0] <= 2 * 0.9e-7 and e[1] <= 2 * 2.2e-7, (n, i, e)


# ---- planted defects -----------------------------------------------------------------------------------------------------------
def radix2_f32(x, sign, tw, poke=None):
    """fp32 radix-2 decimation in time with the twiddle table tw[k] ~ exp(-2 pi i k / n), k < n / 2; poke = (pass, entry): that
    one twiddle of that one pass turned by 1e-6 rad"""
    n = x.size
    lg = n.bit_length() - 1
    idx, rev = np.arange(n), np.zeros(n, np.int64)
    for b in range(lg):
        rev |= ((idx >> b) & 1) << (lg - 1 - b)
    a = np.asarray(x, np.complex64)[rev]
    for s in range(1, lg + 1):
        m, h = 1 << s, 1 << (s - 1)
        w = tw[np.arange(h) * (n // m)]
        if sign > 0:
            w = np.conj(w)
        if poke is not None and poke[0] == s:
            w = w.copy()
            w[poke[1]] = np.complex64(w[poke[1]].astype(np.complex128) * np.exp(1e-6j))
        a = a.reshape(n // m, m)
        u, v = a[:, :h], a[:, h:] * w
        a = np.concatenate([u + v, u - v], axis=1).reshape(-1)
    return a


def tw_exact(n):
    return np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(np.complex64)


def tw_recurrence(n, run=64):
    """w^k by repeated fp32 multiplication, restarted from an exact value every `run` entries (a table of coarse twiddles times
    a recurrence; run over the whole table the drift reaches 9e-5, and runs of 256 reach 1e-5 on an impulse: the old bar sees those)"""
    t = np.full(n // 2, np.complex64(np.exp(-2j * np.pi / n)), np.complex64).reshape(-1, run)
    t[:, 0] = np.exp(-2j * np.pi * np.arange(0, n // 2, run) / n).astype(np.complex64)
    return np.cumprod(t, axis=1, dtype=np.complex64).reshape(-1)


N_DEFECT = 16384
DEFECTS = {
    "control": lambda x, sign: radix2_f32(x, sign, tw_exact(x.size)),
    "float recurrence twiddles": lambda x, sign: radix2_f32(x, sign, tw_recurrence(x.size)),
    "one twiddle of the last pass off by 1e-6 rad": lambda x, sign: radix2_f32(x, sign, tw_exact(x.size), (14, 1)),
    "one twiddle of the second pass off by 1e-6 rad": lambda x, sign: radix2_f32(x, sign, tw_exact(x.size), (2, 1)),
    "output perturbed by 3e-6": lambda x, sign: (
        (T.dft(x) if sign < 0 else T.idft(x)) * (1 + 3e-6 * np.exp(2j * np.pi * np.random.default_rng(3).random(x.size)))).astype(np.complex64),
}


@pytest.fixture(scope="module")
def defect_inputs(oracle):
    ins = transform_inputs(N_DEFECT)
    rows = [(name, x, T.dft(x), oracle.fft(x, prec=0), oracle.fft(x, prec=1)) for name, x in ins]
    white = T.spectrum_errors(rows[0][3], rows[0][2])
    return rows, white


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_fails_the_new_bar_and_passes_the_old(oracle, defect_inputs, defect):
    rows, white = defect_inputs
    oracle.set_fft_hook(DEFECTS[defect])
    try:
        failed, old_ok = {}, True
        for name, x, truth, ref32, ref64 in rows:
            got = oracle.fft(x, prec=2)
            f = T.check_spectrum("planted %s: %s" % (defect, name), got, ref32, truth, white)
            if f:
                failed[name] = f
            old_ok = old_ok and T.passes_old_bar(got, ref64)
    finally:
        oracle.set_fft_hook(None)
    assert old_ok, "the 1e-5 bar sees this defect too"
    if defect == "control":
        assert not failed, failed               # the same transform without a defect is inside the bar on every input
    else:
        assert failed, "no input of the GPU tests shows this defect at the new bar"
    if defect.startswith("one twiddle"):
        assert any(k.startswith("impulse") for k in failed)     # one wrong twiddle is an impulse's whole output


# ---- where the GPU tests put their impulses ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsamples,fft_len,radix", [(65536, 16384, 4), (163680, 65536, 16)])
def test_impulse_blocks_land_where_they_say(oracle, nsamples, fft_len, radix):
    for t, pure in T.acq_impulse_indices(nsamples, fft_len, radix):
        iq, p = T.iq16_impulse(nsamples, t)
        _, td = oracle.sample_iq16(iq, prec=0, want_td=True, nsamples=nsamples, fft_len=fft_len)
        nz = np.flatnonzero(td)
        assert p == pure and nz[-1] == t and (nz.size == 1 if pure else nz.size > 1), (t, pure, nz)


# ---- peak indices -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,radix,limit", [(n, r, l) for n, r in ((16384, 4), (65536, 16)) for l in T.corr_limits(n)])
def test_index_condition_keeps_95_percent_and_the_float_oracle_is_exact_on_them(oracle, n, radix, limit):
    checked = left = 0
    for name, kind, data, code in T.corr_inputs(n, radix):
        if not T.index_checked(kind, limit):
            continue
        truth = T.cells_truth(data, code, limit)
        _, cells = oracle.correlate(code, data, limit=limit, dop_lo=-2, dop_hi=2, prec=0)
        for k, c in enumerate(truth):
            checked += 1
            if c["gap"] < T.TIE:
                left += 1
            else:
                assert int(cells["idx"][k]) == c["idx"], (name, k, c, cells[k])
    assert checked >= 100 and left <= 0.05 * checked, (checked, left)
