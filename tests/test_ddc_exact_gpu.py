"""The DDC kernels (kg_ddc, kg_rxddc, through the C ABI) against the exact-integer model of tests/ddc_exact.py -- no oracle in the loop.

tests/test_ddc_gpu.py holds the kernels bit-exact to oracle/kiwi_oracle_ddc.c, which was written from the same reading of the Verilog
as they were.  Here every output must lie within the worst-case distance a faithful pruned CIC can have from N exact running sums, the
rms distance must be what the dropped bits predict (K_RMS as fixed by tests/test_ddc_exact_cpu.py), and R = 1 must be equal.  The cases
are the ones the CPU file runs the oracle on; the model's values are computed once per process (ddc_exact.wf_case_exact / rx_case_exact).

Every output of every channel is compared, not a window: the model evaluates R <= 128 in int64 and the three larger decimations in
about a second of Python integers."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Ddc, RxDdc
from tests import ddc_exact as dx

pytestmark = pytest.mark.gpu


def check_wf_channels(rows):
    """rows: per channel of dx.WF_LOG2R an int16 [nout, 2] array."""
    for ch, log2r in enumerate(dx.WF_LOG2R):
        got = rows[ch]
        assert got.shape == (dx.WF_SAMPLES >> log2r, 2), (log2r, got.shape)
        exact = dx.wf_case_exact(log2r)
        gi, gq = got[:, 0].tolist(), got[:, 1].tolist()
        dx.check_case("wf", log2r, gi, gq, exact)
        if log2r == 0:
            assert gi == exact[0] and gq == exact[1]
        assert np.abs(got[8:].astype(int)).max() > 5000


def test_ddc_eight_channels_in_one_push(gpu_ctx):
    """One object, decimations 1, 2, 4, 8, 16, 256, 512, 8192 at distinct increments -- the bypass kernel, the two staged special
    cases, the small, the 64-bit and the 96-bit run passes -- on 8192 x 24 samples in ONE push."""
    adc = dx.wf_case_stream()
    d = Ddc(gpu_ctx, nchan=len(dx.WF_LOG2R), max_samples=adc.size)
    try:
        for ch, log2r in enumerate(dx.WF_LOG2R):
            d.set_wf(ch, dx.wf_case_inc(log2r), 1 << log2r)
        check_wf_channels(d.push(adc, list(range(len(dx.WF_LOG2R)))))
    finally:
        d.close()


def test_ddc_ragged_pushes_from_an_unaligned_pointer(gpu_ctx):
    """The same stream in pushes of 1, 63, 4097 samples and the rest, read from 3 samples into the allocation: state carried from push
    to push, the sample-by-sample walk of an unaligned block.  Same assertions, same expected values."""
    adc = dx.wf_case_stream()
    n, chans, shift = adc.size, list(range(len(dx.WF_LOG2R))), 3
    d = Ddc(gpu_ctx, nchan=len(chans), max_samples=n)
    stride = n + 2
    d_adc = gpu_ctx.alloc(2 * (n + 16))
    d_out = gpu_ctx.alloc(len(chans) * stride * 4)
    try:
        for ch, log2r in enumerate(dx.WF_LOG2R):
            d.set_wf(ch, dx.wf_case_inc(log2r), 1 << log2r)
        pad = np.zeros(n + 16, np.int16)
        pad[shift:shift + n] = adc
        gpu_ctx.upload(d_adc, pad)
        parts, pos = [[] for _ in chans], 0
        for step in (1, 63, 4097, n):
            step = min(step, n - pos)
            nouts = d.push_dev(d_adc + 2 * (shift + pos), step, chans, d_out, stride)
            host = np.zeros((len(chans), stride, 2), np.int16)
            gpu_ctx.download(d_out, host)
            for ch in chans:
                parts[ch].append(host[ch, :int(nouts[ch])].copy())
            pos += step
        assert pos == n
        check_wf_channels([np.concatenate(p) for p in parts])
    finally:
        gpu_ctx.free(d_out)
        gpu_ctx.free(d_adc)
        d.close()


@pytest.mark.parametrize("mode", [dx.RX_STD, dx.RX_WIDE, dx.RX_14])
def test_rxddc_two_channels_two_pushes(gpu_ctx, mode):
    """Each audio instance: two channels at different increments, 48 records' worth of samples in two unequal pushes; the 24-bit I
    and Q unpacked from the records within the bound, the record count equal."""
    adc = dx.rx_case_stream(mode)
    decim = dx.rx_decim(mode)
    d = RxDdc(gpu_ctx, nchan=2, max_samples=adc.size, mode=mode)
    try:
        assert d.decim == decim and adc.size == decim * dx.RX_RECORDS
        for ch in range(2):
            d.set_freq(ch, dx.inc_for(dx.RX_INCS[ch]))
        cut = decim * 17 + 1234
        a, b = d.push(adc[:cut], [0, 1]), d.push(adc[cut:], [0, 1])
        for ch in range(2):
            raw = np.concatenate([a[ch], b[ch]])
            assert raw.size == 6 * dx.RX_RECORDS, (mode, ch, raw.size)
            gi, gq = dx.unpack_records(raw)
            dx.check_case("rx", mode, gi, gq, dx.rx_case_exact(mode, ch))
            assert max(abs(v) for v in gi[dx.RX_SKIP:]) > 300000
    finally:
        d.close()
