"""Times the standard noise blanker (NB_STD): kg_nb_process_dev (the audio call site, rx/rx_sound.cpp:593-598) for 14 / 128 / 1024
channels x 512 / 4096 samples, and kg_wf_frames_dev (one frame per channel) with 0 % and 100 % of the frames blanked (the waterfall's
pre-pass, rx/rx_waterfall.cpp:1087-1099) for 14 and 128 channels.
usage: python tools/time_nb.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, NoiseBlanker, Waterfall, WfParams, synth, wf   # noqa: E402

ctx = Context(0)
print("device %s" % ctx.name)
reps = 20
for nchan in (14, 128, 1024):
    for n in (512, 4096):
        rng = np.random.default_rng(1)
        x = rng.normal(0, 300, (nchan, n, 2)).astype(np.float32)
        x[:, ::97] *= 40.0                                 # pulses
        d = ctx.alloc(x.nbytes)
        ctx.upload(d, x)
        nb = NoiseBlanker(ctx, nchan=nchan, max_in=n)
        for ch in range(nchan):
            nb.setup(ch, 12000.0, [100.0, 50.0])
        chans = np.arange(nchan, dtype=np.int32)
        cnt = np.full(nchan, n, np.int32)
        for _ in range(3):
            nb.process_dev(chans, d, n, cnt, d, n)
        ctx.sync()
        ctx.timer_start()
        for _ in range(reps):
            nb.process_dev(chans, d, n, cnt, d, n)
        us = ctx.timer_stop() / reps * 1e3
        print("kg_nb_process_dev  nchan %5d x %5d samples: %9.1f us per call" % (nchan, n, us))
        nb.close()
        ctx.free(d)

tabs = wf.window_functions(), wf.cic_comp_table()
for nchan in (14, 128):
    w = Waterfall(ctx, nchan=nchan)
    w.set_tables(*tabs)
    for ch in range(nchan):
        w.set_channel(ch, WfParams.for_zoom(ch % 8, 1.0e6 * (ch % 8)))
        w.nb_setup(ch, [100.0, 50.0])
    iq = np.stack([synth.wf_iq_frame(seed=ch) for ch in range(nchan)])
    d_iq, d_out = ctx.alloc(iq.nbytes), ctx.alloc(nchan * 1024)
    ctx.upload(d_iq, iq)
    chan_of = np.arange(nchan, dtype=np.int32)
    for frac in (0, 100):
        for ch in range(nchan):
            w.set_nb(ch, frac == 100)
        for _ in range(3):
            w.frames_dev(chan_of, d_iq, d_out)
        ctx.sync()
        ctx.timer_start()
        for _ in range(reps):
            w.frames_dev(chan_of, d_iq, d_out)
        us = ctx.timer_stop() / reps * 1e3
        print("kg_wf_frames_dev   nchan %5d, %3d %% blanked: %9.1f us per call (one frame per channel)" % (nchan, frac, us))
    ctx.free(d_iq)
    ctx.free(d_out)
    w.close()
ctx.close()

# a `receivers` bank step (128 receivers) with the blanker on every receiver (audio and waterfall) against off, ABAB in one process
import time  # noqa: E402
from flydog_sdr_gps_amd import nb as nb_mod, synth as synth_mod  # noqa: E402
from flydog_sdr_gps_amd.rxbank import MIXES, RxBank  # noqa: E402

N = 1 << 22
bank = RxBank(128, N)
mix = MIXES["survey"](128, 0, N)
bank.configure(mix)
a = synth_mod.adc_stream(N, 0x5EED0001)
d_adc = bank.ctx.alloc(a.nbytes)
bank.ctx.upload(d_adc, a)


def steps(k):
    for _ in range(3):
        bank.step(d_adc)
    bank.sync()
    t0 = time.perf_counter()
    for _ in range(k):
        bank.step(d_adc)
    bank.sync()
    return (time.perf_counter() - t0) / k * 1e3


res = {"off": [], "on": []}
for rep in range(2):
    for state in ("off", "on"):
        for rx in range(128):
            if state == "on":
                bank.set_nb(rx, nb_mod.NB_STD, [100.0, 50.0], (1, 1))
            else:
                bank.set_nb(rx, nb_mod.NB_OFF)
        res[state].append(steps(20))
        print("receivers bank step, 128 receivers, blanker %-3s: %7.3f ms per step" % (state, res[state][-1]))
print("on / off: %.3f" % (min(res["on"]) / min(res["off"])))
bank.ctx.free(d_adc)
bank.close()
