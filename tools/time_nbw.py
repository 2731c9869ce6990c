"""Times kg_post_process_dev with the Wild noise blanker (NB_WILD, rx/Teensy/NB_Wild.cpp) on every channel of a batch of SSB receiver
channels, 512 samples per channel and launch (c2s_sound()'s ns_out): the stage off, on at the defaults (thresh 0.95, 10 taps, 7
samples) and at the array limits (40 taps, 41 samples), each on clicky input (the scan reaches its cap of 20 hits, every one a serial
repair) and on quiet input (thresh 20: no hit, the block pays the autocorrelation, Levinson-Durbin, the two filters and the scan).
The off rows bracket the others, so their spread is the run-to-run spread on this machine ("The Wild noise blanker").
usage: python tools/time_nbw.py [nchan ...]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, Post, post   # noqa: E402

# name -> (vector or None, clicky input)
CASES = [("stage off", None, True), ("0.95/10/7 clicky", (0.95, 10, 7), True), ("20/10/7 quiet", (20.0, 10, 7), False),
         ("0.95/40/41 clicky", (0.95, 40, 41), True), ("20/40/41 quiet", (20.0, 40, 41), False), ("stage off (again)", None, False)]

ctx = Context(0)
n = 512
for nchan in [int(a) for a in sys.argv[1:]] or [14, 128, 1024]:
    rng = np.random.default_rng(1)
    t = np.arange(n)
    tone = 3000 * np.exp(2j * np.pi * rng.uniform(0.01, 0.2, (nchan, 1)) * t)
    inputs = {False: (tone + rng.normal(0, 30, (nchan, n)) + 1j * rng.normal(0, 30, (nchan, n))).astype(np.complex64),
              True: (tone + rng.normal(0, 900, (nchan, n)) + 1j * rng.normal(0, 900, (nchan, n))).astype(np.complex64)}
    chans = np.arange(nchan, dtype=np.int32)
    d_x = {k: ctx.alloc(v.nbytes) for k, v in inputs.items()}
    for k, v in inputs.items():
        ctx.upload(d_x[k], v)
    d_s = ctx.alloc(nchan * n * 2); d_d = ctx.alloc(nchan * n * 4); d_a = ctx.alloc(nchan * n * 8)
    for name, vec, clicky in CASES:
        P = Post(ctx, nchan=nchan)
        for ch in range(nchan):
            P.set_agc(ch, True, ch & 1, -100, 50, 6, 1000, 12000.0)
            P.set_smeter(ch, 12000.0)
            P.set_mode(ch, post.MODE_SSB)
            if vec is not None:
                P.nbw_init(ch, vec)
                P.set_nbw(ch, 1)
        for _ in range(6):
            P.process_dev(chans, d_x[clicky], n, n, d_s, d_d, d_a, n)
        ctx.sync()
        best, total, rounds, reps = 1e30, 0.0, 5, 10
        for _ in range(rounds):
            ctx.timer_start()
            for _ in range(reps):
                P.process_dev(chans, d_x[clicky], n, n, d_s, d_d, d_a, n)
            us = ctx.timer_stop() / reps * 1e3
            best = min(best, us); total += us
        rt = n / 12000.0 / (total / rounds * 1e-6)
        print("nchan %5d %-20s %8.1f us per 512-sample pass (best of %d rounds %8.1f), %7.0f x real time at 12 kHz"
              % (nchan, name, total / rounds, rounds, best, rt))
        P.close()
    for d in list(d_x.values()) + [d_s, d_d, d_a]:
        ctx.free(d)
