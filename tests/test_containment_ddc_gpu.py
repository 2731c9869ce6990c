"""Containment of the device entry points of include/kiwigpu.h, part 3: the waterfall DDC (push, capture, step), the audio DDC, the
waterfall frames, and the entry points that only read caller memory (aperture averages, the acquisition front end).  The four
properties (W, R, P, E) and the layouts are those of tests/test_containment_gpu.py; the DDC and frame cases are held to the oracle /
the host-buffer call as well."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import Aperture, Ddc, RxDdc, Searcher, Waterfall, WfParams, ddc, wf
from flydog_sdr_gps_amd._lib import check, ptr
from tests.guarded import contain

pytestmark = pytest.mark.gpu

N = 4096 + 1234                       # one whole block of the R = 1 kernel's straight-line loop and a ragged end
LOG2R = [0, 0, 1, 4]                  # channel -> log2 R: two bypass channels, R = 2, R = 16
LIST = [2, 0, 3, 1]


def adc_stream(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n)
    x = rng.normal(0, 40.0, n) + 9000.0 * np.cos(2 * np.pi * 0.0123 * t + 1.0) + 700.0 * np.cos(2 * np.pi * 0.201 * t + 2.0)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def inc_for(f):
    return (-int(round(f * 2 ** 48))) & ((1 << 48) - 1)


INCS = [inc_for(0.017 + 0.019 * k) for k in range(4)]
ADC = adc_stream(2 * N, 77)


def new_ddc(ctx):
    d = Ddc(ctx, nchan=4, max_samples=N)
    for ch, lr in enumerate(LOG2R):
        d.set_wf(ch, INCS[ch], 1 << lr)
    return d


# (alignment of d_adc, alignment of d_out, stride pad, stride a multiple of): 2 / 4 bytes is the least the header allows (the ADC
# pointer shifted by one sample).  The R = 1 kernel stores whole blocks 16 bytes at a time when d_adc sits at 8 bytes and EVERY
# R = 1 row at 16: row 0 at 16 bytes and the padded stride rounded up to 4 pairs (5330 + 4 -> 5336 pairs = 16 * 1334 bytes) puts
# all four rows there, so N = one whole block (16-byte stores) and a ragged end of 1234 = 4 * 308 + 2 pairs (16-byte stores of the
# general form, then two single pairs), with two pairs of pad behind each row for a store that runs past the last pair to land in.
# The tight run of these cases keeps stride = the used size (5330 pairs: the R = 1 rows at 8 mod 16), the other form of the kernel.
ALIGNMENTS = [(2, 4, 1, 1), (8, 16, 4, 4), (16, 16, 4, 4), (2, 16, 4, 4), (16, 4, 1, 1)]
ALIGNED = ALIGNMENTS[1]


def out_rows(lay, nrows, max_used, a_out, pad, mult):
    """the pair rows of one call -> (Guarded, stride in pairs)"""
    g, st = lay.out(nrows, max_used, 4, a_out, pad=pad, mult=1 if lay.tight else mult)
    assert lay.tight or mult != 4 or all(g.row_ptr(i) % 16 == 0 for i in range(nrows))
    return g, st


@pytest.mark.parametrize("a_adc,a_out,pad,mult", ALIGNMENTS)
def test_ddc_wf_push(gpu_ctx, oracle, a_adc, a_out, pad, mult):
    def case(lay):
        d = new_ddc(gpu_ctx)
        try:
            res = []
            for piece in range(2):
                want = [int(d.outputs(ch, N)) for ch in LIST]
                g_adc, _ = lay.inp([ADC[piece * N:(piece + 1) * N]], a_adc)
                g_out, s_out = out_rows(lay, 4, max(want), a_out, pad, mult)
                nouts = d.push_dev(g_adc.ptr, N, LIST, g_out.ptr, s_out)
                gpu_ctx.sync()
                assert nouts.tolist() == want
                res.append((lay.take(g_out, [4 * int(k) for k in nouts]), nouts))
            return res
        finally:
            d.close()

    res = contain(gpu_ctx, case)
    for i, ch in enumerate(LIST):
        want, _ = oracle.ddc_wf(ADC, INCS[ch], LOG2R[ch])
        assert res[0][0][i][2] + res[1][0][i][2] == np.ascontiguousarray(want, np.int16).tobytes(), ch


@pytest.mark.parametrize("a_adc,a_out,pad,mult", ALIGNMENTS[:2])
@pytest.mark.parametrize("max_out", [1, 100])
def test_ddc_wf_capture(gpu_ctx, oracle, max_out, a_adc, a_out, pad, mult):
    """the one-shot sampler: min(max_out, n >> log2 R) pairs per row; the push behind it shows the state the capture left"""
    def case(lay):
        d = new_ddc(gpu_ctx)
        try:
            g_adc, _ = lay.inp([ADC[:N]], a_adc)
            g_out, s_out = out_rows(lay, 4, max_out, a_out, pad, mult)
            nouts = d.capture_dev(g_adc.ptr, N, LIST, g_out.ptr, s_out, max_out)
            gpu_ctx.sync()
            assert nouts.tolist() == [min(max_out, N >> LOG2R[ch]) for ch in LIST]
            cap = lay.take(g_out, [4 * int(k) for k in nouts])
            want = [int(d.outputs(ch, N)) for ch in LIST]
            g_adc2, _ = lay.inp([ADC[N:]], a_adc)
            g_out2, s_out2 = out_rows(lay, 4, max(want), a_out, pad, mult)
            nouts2 = d.push_dev(g_adc2.ptr, N, LIST, g_out2.ptr, s_out2)
            gpu_ctx.sync()
            return cap, nouts, lay.take(g_out2, [4 * int(k) for k in nouts2]), nouts2
        finally:
            d.close()

    cap, _, _, _ = contain(gpu_ctx, case)
    for i, ch in enumerate(LIST):                      # a fresh channel's first outputs: the reset falls on the block's first sample
        want, _ = oracle.ddc_wf(ADC[:N], INCS[ch], LOG2R[ch])
        assert cap[i][2] == np.ascontiguousarray(want[:max_out], np.int16).tobytes(), ch


# (list, out_off, max_out (0: the entry pushes), layout).  The first: least alignment, both R = 1 entries capture.  The second: the
# R = 1 entries PUSH, at offsets of whole 16 bytes into 16-byte rows, so the whole-block 16-byte stores and the ragged end run at an
# offset into the row too; its first three entries are a pushed, a captured and a pushed one at out_off = [0, 6, 2].
STEPS = [([2, 0, 3, 1], [0, 6, 2, 3], [0, 100, 0, 1], ALIGNMENTS[0]),
         ([0, 3, 2, 1], [0, 6, 2, 4], [0, 100, 0, 0], ALIGNED)]


@pytest.mark.parametrize("chans,offs,maxs,layout", STEPS, ids=["least", "aligned"])
def test_ddc_wf_step(gpu_ctx, chans, offs, maxs, layout):
    """pushed and captured entries in one call, each at an offset into its row: the pairs in front of out_off[i] are guard too"""
    a_adc, a_out, pad, mult = layout
    out_off, max_out, lst = np.array(offs, np.int64), np.array(maxs, np.int64), np.array(chans, np.int32)

    def case(lay):
        d = new_ddc(gpu_ctx)
        try:
            res = []
            for piece in range(2):
                want = [min(int(m), N >> LOG2R[ch]) if m else int(d.outputs(ch, N)) for ch, m in zip(chans, max_out)]
                g_adc, _ = lay.inp([ADC[piece * N:(piece + 1) * N]], a_adc)
                g_out, s_out = out_rows(lay, 4, max(w + int(o) for w, o in zip(want, out_off)), a_out, pad, mult)
                nouts = np.zeros(4, np.int64)
                check(gpu_ctx.lib.kg_ddc_wf_step_dev(d.h, ptr(g_adc.ptr), N, ptr(lst), 4, ptr(g_out.ptr), s_out, ptr(out_off), ptr(max_out),
                                                     ptr(nouts)), "kg_ddc_wf_step_dev")
                gpu_ctx.sync()
                assert nouts.tolist() == want
                res.append((lay.take(g_out, [(4 * int(o), 4 * int(o + k)) for o, k in zip(out_off, nouts)]), nouts))
            return res
        finally:
            d.close()

    res = contain(gpu_ctx, case)
    # the entries equal what the two single-mode calls give for the same channels (first block)
    rows = res[0][0]
    d = new_ddc(gpu_ctx)
    try:
        pushed = d.push(ADC[:N], [ch for ch, m in zip(chans, maxs) if not m])
    finally:
        d.close()
    for i, ch, m in zip(range(4), chans, maxs):
        if m:
            d = new_ddc(gpu_ctx)
            try:
                want = d.capture(ADC[:N], [ch], m)[0]
            finally:
                d.close()
        else:
            want = pushed[[c for c, mm in zip(chans, maxs) if not mm].index(ch)]
        assert rows[i][2] == want.tobytes(), (i, ch)


@pytest.mark.parametrize("a_adc", [2, 16])
@pytest.mark.parametrize("mode", [ddc.RX_STD, ddc.RX_WIDE])
def test_rxddc_push(gpu_ctx, mode, a_adc):
    """n = 3 decim + 5, then 5: the second call yields no record or one.  d_adc at 2 bytes, the least the header allows, and at 16:
    the kernel reads a run of the stream eight samples at a time where the run's start is 16-byte aligned"""
    lst = [2, 0, 1]
    decim = ddc.RX_DECIM if mode == ddc.RX_STD else ddc.RX_DECIM_WIDE
    ns = [3 * decim + 5, 5]
    adc = adc_stream(sum(ns), 78)
    incs = [ddc.rx_phase_inc(7.0e6 + 1.0e5 * ch) for ch in range(3)]

    def case(lay):
        d = RxDdc(gpu_ctx, nchan=3, max_samples=ns[0], mode=mode)
        try:
            for ch in range(3):
                d.set_freq(ch, incs[ch])
            res, pos = [], 0
            for n in ns:
                want = [int(d.outputs(ch, n)) for ch in lst]
                g_adc, _ = lay.inp([adc[pos:pos + n]], a_adc)
                g_out, s_out = lay.out(3, max(want), 6, 2)
                nouts = d.push_dev(g_adc.ptr, n, lst, g_out.ptr, s_out)
                gpu_ctx.sync()
                assert nouts.tolist() == want
                res.append((lay.take(g_out, [6 * int(k) for k in nouts]), nouts))
                pos += n
            return res
        finally:
            d.close()

    res = contain(gpu_ctx, case)
    assert np.frombuffer(res[0][1][2], np.int32).tolist() == [3, 3, 3]
    d = RxDdc(gpu_ctx, nchan=3, max_samples=sum(ns), mode=mode)         # the same stream in one piece through the host-buffer call
    try:
        for ch in range(3):
            d.set_freq(ch, incs[ch])
        whole = d.push(adc, lst)
    finally:
        d.close()
    for i in range(3):
        assert res[0][0][i][2] + res[1][0][i][2] == whole[i].tobytes(), i


# ------------------------------------------------------------------------------------------------------------- waterfall frames
GAP = 6                                # iq_t pairs of guard between two frames (frame offsets are even)


def new_wf(ctx, nb):
    w = Waterfall(ctx, nchan=2)
    w.set_tables()
    w.set_channel(0, WfParams.for_zoom(0, 0.0), interp=wf.WF_MAX, window_func=wf.WINF_NONE, cic_comp=False)
    w.set_channel(1, WfParams.for_zoom(3, 1.0e6))
    if nb:
        for ch in range(2):
            w.nb_setup(ch, [100.0 + 50 * ch, 50.0])
    return w


def frames_iq(seed):
    rng = np.random.default_rng(seed)
    t = np.arange(8192)
    out = []
    for f in range(3):
        x = 3000 * np.exp(2j * np.pi * (0.05 + 0.1 * f) * t) + 200 * (rng.standard_normal(8192) + 1j * rng.standard_normal(8192))
        x[100 + 50 * f::1500] *= 9.0                                   # pulses (for the blanker)
        out.append(np.stack([np.clip(x.real, -32768, 32767), np.clip(x.imag, -32768, 32767)], 1).astype(np.int16))
    return out


CHAN_OF = [1, 0, 1]


@pytest.mark.parametrize("which", ["frames", "frames_at", "frames_at_blanked", "nb_frames"])
def test_wf_frames(gpu_ctx, which):
    """3 frames over 2 channels.  kg_wf_frames_dev reads them back to back; the _at forms where frame_off says, with guard between
    and around the frames (a row of the guarded input = one frame).  Rows / spectra go out back to back: 1024 bytes (8192 complex
    floats) per frame."""
    iq = frames_iq(61)
    nb = which in ("frames_at_blanked", "nb_frames")

    def case(lay):
        w = new_wf(gpu_ctx, nb)
        try:
            if which == "frames_at_blanked":
                w.set_nb(1, True)
            if which == "frames":
                g_iq, _ = lay.inp([np.concatenate(iq)], 8)
                off = None
            else:
                g_iq, s_iq = lay.inp(iq, 8, pad=GAP, elem=4)
                off = [f * s_iq for f in range(3)]
            per = 8192 * 8 if which == "nb_frames" else 1024
            g_out, _ = lay.out(1, 3 * per, 1, 8 if which == "nb_frames" else 4)
            if which == "nb_frames":
                w.nb_frames(CHAN_OF, g_iq.ptr, g_out.ptr, off, off[2] + 8192)
            else:
                w.frames_dev(CHAN_OF, g_iq.ptr, g_out.ptr, off, None if off is None else off[2] + 8192)
            gpu_ctx.sync()
            return lay.take(g_out, 3 * per), (w.nb_state([0, 1]) if nb else None)
        finally:
            w.close()

    rows, _ = contain(gpu_ctx, case)
    if which in ("frames", "frames_at"):                               # what the host-buffer call gives for the same frames
        w = new_wf(gpu_ctx, False)
        try:
            assert rows[0][2] == w.frames(CHAN_OF, np.stack(iq)).tobytes()
        finally:
            w.close()


# ---------------------------------------------------------------------------------------------- entry points that only read (R)
def test_aper_update(gpu_ctx):
    lst = [2, 0, 1]
    rng = np.random.default_rng(71)
    rows = [[rng.integers(0, 256, 1024).astype(np.uint8) for _ in lst] for _ in range(2)]

    def case(lay):
        a = Aperture(gpu_ctx, nchan=4)
        try:
            for k, clear in enumerate((1, 0)):
                g_rows, s_rows = lay.inp(rows[k], 1)
                a.update_dev(lst, g_rows.ptr, s_rows, [(0, 0.2, clear, 0), (1, 4.0, clear, 1), (2, 0.5, clear, 0)])
                gpu_ctx.sync()
            return [a.get(ch) for ch in lst]
        finally:
            a.close()

    contain(gpu_ctx, case)


def test_acq_sample(gpu_ctx):
    """the front end's three device forms: packed bits (any byte address), one IQ block, two IQ blocks a stride apart (4 bytes)"""
    rng = np.random.default_rng(72)
    bits = [rng.integers(0, 256, 65536 // 8).astype(np.uint8)]
    iq = [rng.integers(-2000, 2000, 2 * 65536).astype(np.int16) for _ in range(2)]

    def case(lay):
        s = Searcher(gpu_ctx, max_sats=1, max_blocks=2)
        try:
            g_bits, _ = lay.inp(bits, 1)
            s.sample(g_bits.ptr, block=0)
            gpu_ctx.sync()
            td_bits = s.get_data_td(0)
            g_one, _ = lay.inp(iq[:1], 4, elem=4)
            s.sample_iq16(g_one.ptr, block=1)
            gpu_ctx.sync()
            td_one = s.get_data_td(1)
            g_two, s_two = lay.inp(iq, 4, elem=4)
            s.sample_iq16_batch(g_two.ptr, 2, first_block=0, stride_bytes=4 * s_two)
            gpu_ctx.sync()
            return td_bits, td_one, s.get_data_td(0), s.get_data_td(1)
        finally:
            s.close()

    _, td_one, td_b0, td_b1 = contain(gpu_ctx, case)
    assert td_one == td_b0 and td_b0 != td_b1
