"""Containment in the receiver bank's own buffers (kg_rxbank_buffers, kg_rxbank_spec_rows).  They are the library's allocations, so
there are no guard bands here, only the rows themselves: before every step each caller-visible buffer is overwritten with a byte
pattern, and after the step
  - every row's bytes beyond nrec / nfir / pkt_bytes still hold the pattern,
  - every row of a receiver that left, and every row a receiver's mode does not produce, is wholly untouched,
  - frames / packets / spectrum rows of slots beyond the step's counts are untouched;
the used parts are the same for the patterns 0x00 and 0xFF (no step reads what a buffer held before it) and equal, bit for bit, an
unpatterned run of the same bank.

wf_iq is left out: it is the samplers' ring, which an overlapped receiver legitimately keeps older samples in and reads back on later
steps (the frame is the ring's newest 8192 outputs); the used parts of everything computed from it are compared instead."""
import ctypes as C

import numpy as np
import pytest

from flydog_sdr_gps_amd import WfParams, post
from flydog_sdr_gps_amd._lib import check
from flydog_sdr_gps_amd.rxbank import ADC_CLOCK, UI_SRATE, RxBank, light_mix

pytestmark = pytest.mark.gpu

NRX, N, STEPS = 4, 1 << 22, 3
STEREO = {2}                           # receiver 2 is in IQ mode: IQ payload rows, no mono16 / ADPCM rows
LEFT_BEFORE = {3: 1}                   # receiver 3 leaves before step 1


def adc_blocks():
    rng = np.random.Generator(np.random.PCG64(90))
    t = np.arange(N * STEPS)
    x = rng.normal(0, 300.0, t.size) + 9000.0 * np.cos(2 * np.pi * 0.0123 * t) + 2500.0 * np.cos(2 * np.pi * 0.0301 * t + 1.0)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(STEPS, N)


def buffers(bank):
    """name -> (device pointer, rows, row bytes) of every caller-visible buffer but wf_iq"""
    b = bank.bufs
    fs, rs = int(b.fir_stride), int(b.rx_stride)
    out = {"wf_rows": (b.wf_rows, NRX, 1024), "wf_pkts": (b.wf_pkts, NRX, int(b.wf_pkt_stride)), "rx_raw": (b.rx_raw, NRX, 6 * rs),
           "rx_in": (b.rx_in, NRX, 8 * rs), "fir_out": (b.fir_out, NRX, 8 * fs), "s16": (b.s16, NRX, 2 * fs),
           "adpcm": (b.adpcm, NRX, fs // 2), "agc": (b.agc, NRX, 8 * fs), "iq_pay": (b.iq_pay, NRX, 4 * fs)}
    d, stride = C.c_void_p(), C.c_size_t()
    check(bank.lib.kg_rxbank_spec_rows(bank.h, C.byref(d), C.byref(stride)), "kg_rxbank_spec_rows")
    out["spec"] = (int(d.value), check(bank.lib.kg_rxbank_spec_max(bank.h), "kg_rxbank_spec_max"), int(stride.value))
    return out


def run_bank(adc, pattern):
    """-> per step: the used part of every buffer, the maps and the step info"""
    bank = RxBank(NRX, N)
    d_adc = bank.ctx.alloc(2 * N)
    try:
        mix = light_mix(NRX, n=N)
        bank.configure(mix)
        hz_per_start = UI_SRATE / (1024 << 14)
        bank.set_wf(1, WfParams.for_zoom(11, 3.0e6 / hz_per_start, adc_clock=ADC_CLOCK, ui_srate=UI_SRATE), True)   # overlapped: R = 1024
        bank.set_audio(2, mix[2][2], mode=post.MODE_IQ)
        bank.set_spec(0, 2)                                             # receiver 0 shows the audio spectrum
        bufs = buffers(bank)
        steps = []
        for step in range(STEPS):
            for rx, at in LEFT_BEFORE.items():
                if at == step:
                    bank.leave(rx)
            gone = {rx for rx, at in LEFT_BEFORE.items() if at <= step}
            bank.sync()
            bank.ctx.upload(d_adc, adc[step])
            if pattern is not None:
                for name, (dptr, rows, rb) in bufs.items():
                    bank.ctx.upload(dptr, np.full(rows * rb, pattern, np.uint8))
            info = bank.step(d_adc)
            bank.sync()
            rx_of, f_off, pkt_bytes = bank.frame_map()
            nrec, nfir, pos, seq = bank.audio_map()
            s_rx, s_inst, s_blk = bank.spec_map()
            assert not set(int(r) for r in rx_of) & gone and all(nrec[rx] == 0 and nfir[rx] == 0 for rx in gone)
            nf = len(rx_of)
            # the bytes a row may hold after this step
            used = {"wf_rows": [1024 if f < nf else 0 for f in range(NRX)],
                    "wf_pkts": [int(pkt_bytes[f]) if f < nf else 0 for f in range(NRX)],
                    "rx_raw": [6 * int(nrec[rx]) for rx in range(NRX)], "rx_in": [8 * int(nrec[rx]) for rx in range(NRX)],
                    "fir_out": [8 * int(nfir[rx]) for rx in range(NRX)],
                    "s16": [0 if rx in STEREO else 2 * int(nfir[rx]) for rx in range(NRX)],
                    "adpcm": [0 if rx in STEREO else int(nfir[rx]) // 2 for rx in range(NRX)],
                    "agc": [8 * int(nfir[rx]) if rx in STEREO else 0 for rx in range(NRX)],     # the others are SSB: no AGC row
                    "iq_pay": [4 * int(nfir[rx]) if rx in STEREO else 0 for rx in range(NRX)],
                    "spec": [1024 if r < len(s_rx) else 0 for r in range(bufs["spec"][1])]}
            parts = {}
            for name, (dptr, rows, rb) in bufs.items():
                got = np.empty((rows, rb), np.uint8)
                bank.ctx.download(dptr, got)
                parts[name] = [got[r, :used[name][r]].copy() for r in range(rows)]
                if pattern is not None:
                    for r in range(rows):
                        stray = np.flatnonzero(got[r, used[name][r]:] != pattern)
                        assert stray.size == 0, "step %d: %s row %d written at byte %d, %d bytes beyond its %d used" % (
                            step, name, r, used[name][r] + int(stray[0]), stray.size, used[name][r])
            steps.append((parts, (rx_of, f_off, pkt_bytes), (nrec, nfir, pos, seq), (s_rx, s_inst, s_blk),
                          (int(info.step), int(info.nframes), int(info.nmoves))))
        return steps
    finally:
        bank.sync()
        bank.ctx.free(d_adc)
        bank.close()


def test_bank_buffers():
    from tests.guarded import first_difference, freeze
    adc = adc_blocks()
    plain, zeros, ones = (freeze(run_bank(adc, p)) for p in (None, 0x00, 0xFF))
    # the configuration does what the cases need: frames, an overlapped frame, sound blocks of both kinds, a spectrum row
    nfir_total = sum(int(np.frombuffer(s[2][1][2], np.int32).sum()) for s in plain)
    assert nfir_total >= 512 * 2 * 3
    assert any(len(s[1][0][2]) // 4 >= 3 for s in plain) and any(len(s[3][0][2]) > 0 for s in plain)
    d = first_difference(zeros, ones)
    assert d is None, "a step's results depend on what the buffers held before it: " + d
    d = first_difference(zeros, plain)
    assert d is None, "the patterned run differs from the unpatterned one: " + d
