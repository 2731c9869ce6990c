"""Times the audio spectrum rows (specAF_FFT, rx/rx_sound.cpp:175-220):
  * kg_fir_process_spec_dev (rows only) against kg_fir_process_each_dev, and against the two-call form kg_fir_process_taps_dev (d_post)
    + kg_snd_spec_rows_dev, for 14 and 128 channels at one and four blocks a call;
  * a `receivers` bank step (128 receivers) with the rows on for every receiver against off, ABAB in one process.
Every figure is the median of REPS timed batches of BATCH calls between device events, each batch behind a drained stream; the
spread is the batches' (max - min) / median.  At these sizes a call is bound by the host enqueueing its launches, not by the device.
usage: python tools/time_spec.py"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, snd, synth   # noqa: E402
from flydog_sdr_gps_amd._lib import check, ptr       # noqa: E402

ctx = Context(0)
print("device %s" % ctx.name)
REPS, BATCH = 9, 400


def timed(fn):
    for _ in range(5):
        fn()
    ctx.sync()
    t = []
    for _ in range(REPS):
        ctx.timer_start()
        for _ in range(BATCH):
            fn()
        t.append(ctx.timer_stop() / BATCH * 1e3)
    t = np.array(t)
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


for nchan in (14, 128):
    for nblk in (1, 4):
        n = 512 * nblk
        rng = np.random.default_rng(1)
        x = (rng.normal(0, 3000, (nchan, n)) + 1j * rng.normal(0, 3000, (nchan, n))).astype(np.complex64)
        d_in, d_out = ctx.alloc(x.nbytes), ctx.alloc(nchan * n * 8)
        d_rows, d_post = ctx.alloc(nchan * nblk * 1024), ctx.alloc(nchan * nblk * 1024 * 8)
        ctx.upload(d_in, x)
        F = snd.FastFir(ctx, nchan=nchan, max_in=n)
        for ch in range(nchan):
            F.setup(ch, 300.0, 2700.0, 0.0, 12000.0)
        chans = np.arange(nchan, dtype=np.int32)
        each = np.full(nchan, n, np.int32)
        inst = np.zeros(nchan, np.int32)
        inst_rows = np.zeros(nchan * nblk, np.int32)
        nout = np.zeros(nchan, np.int32)

        def plain():
            check(F.lib.kg_fir_process_each_dev(F.h, ptr(chans), nchan, ptr(d_in), n, ptr(each), ptr(d_out), n, ptr(nout)), "each")

        def fused():
            F.process_spec_dev(chans, d_in, n, each, d_out, n, d_rows, nblk * 1024, inst)

        def two_calls():
            check(F.lib.kg_fir_process_taps_dev(F.h, ptr(chans), nchan, ptr(d_in), n, n, ptr(d_out), n, ptr(nout), None, ptr(d_post),
                                                nblk * 1024), "taps")
            snd.spec_rows_dev(ctx, d_post, 1024, inst_rows, d_rows, 1024)

        res = {k: timed(f) for k, f in (("plain", plain), ("fused", fused), ("two calls", two_calls), ("plain again", plain))}
        print("nchan %4d x %d block(s): " % (nchan, nblk) +
              "; ".join("%s %7.1f us (spread %4.1f %%)" % (k, v[0], 100 * v[1]) for k, v in res.items()) +
              "; fused - plain %+6.1f us, fused / two calls %.3f" % (res["fused"][0] - res["plain"][0], res["fused"][0] / res["two calls"][0]))
        F.close()
        for d in (d_in, d_out, d_rows, d_post):
            ctx.free(d)
ctx.close()

from flydog_sdr_gps_amd.rxbank import MIXES, RxBank  # noqa: E402

N = 1 << 22
bank = RxBank(128, N)
bank.configure(MIXES["survey"](128, 0, N))
a = synth.adc_stream(N, 0x5EED0001)
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
for rep in range(3):
    for state in ("off", "on"):
        for rx in range(128):
            bank.set_spec(rx, 2 if state == "on" else 0)
        res[state].append(steps(40))
        print("receivers bank step, 128 receivers, rows %-3s: %7.3f ms per step" % (state, res[state][-1]))
for k, v in res.items():
    print("rows %-3s: median %.3f ms, spread %.1f %%" % (k, np.median(v), 100 * (max(v) - min(v)) / np.median(v)))
print("on - off: %+.3f ms (%.2f %%)" % (np.median(res["on"]) - np.median(res["off"]), 100 * (np.median(res["on"]) / np.median(res["off"]) - 1)))
bank.ctx.free(d_adc)
bank.close()
