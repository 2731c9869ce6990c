"""Times kg_post_process_dev with the noise-reduction stage (rx/rx_sound.cpp:933-949) for a batch of SSB receiver channels, 512
samples per channel and launch (c2s_sound()'s ns_out): NR_WDSP at 64 and 128 taps, auto-notch, denoiser and both; NR_ORIG, both;
and the NR-off modes (SSB, AM, NBFM) beside them, which launch what they launched before the stage existed.
usage: python tools/time_nr.py [nchan ...]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, Post, post   # noqa: E402

# name -> (mode, algo, taps, enables (denoise, auto-notch))
CASES = [("SSB, NR off", post.MODE_SSB, post.NR_OFF, 0, (0, 0)), ("AM, NR off", post.MODE_AM, post.NR_OFF, 0, (0, 0)),
         ("NBFM, NR off", post.MODE_NBFM, post.NR_OFF, 0, (0, 0)),
         ("WDSP 64 auto-notch", post.MODE_SSB, post.NR_WDSP, 64, (0, 1)), ("WDSP 64 denoise", post.MODE_SSB, post.NR_WDSP, 64, (1, 0)),
         ("WDSP 64 both", post.MODE_SSB, post.NR_WDSP, 64, (1, 1)), ("WDSP 128 auto-notch", post.MODE_SSB, post.NR_WDSP, 128, (0, 1)),
         ("WDSP 128 denoise", post.MODE_SSB, post.NR_WDSP, 128, (1, 0)), ("WDSP 128 both", post.MODE_SSB, post.NR_WDSP, 128, (1, 1)),
         ("ORIG both", post.MODE_SSB, post.NR_ORIG, 0, (1, 1))]

ctx = Context(0)
n = 512
for nchan in [int(a) for a in sys.argv[1:]] or [14, 128, 1024]:
    rng = np.random.default_rng(1)
    t = np.arange(n)
    x = (3000 * np.exp(2j * np.pi * rng.uniform(0.01, 0.2, (nchan, 1)) * t)
         + rng.normal(0, 30, (nchan, n)) + 1j * rng.normal(0, 30, (nchan, n))).astype(np.complex64)
    chans = np.arange(nchan, dtype=np.int32)
    d_x = ctx.alloc(x.nbytes); ctx.upload(d_x, x)
    d_s = ctx.alloc(nchan * n * 2); d_d = ctx.alloc(nchan * n * 4); d_a = ctx.alloc(nchan * n * 8)
    for name, mode, algo, taps, en in CASES:
        P = Post(ctx, nchan=nchan)
        for ch in range(nchan):
            P.set_agc(ch, True, ch & 1, -100, 50, 6, 1000, 12000.0)
            P.set_smeter(ch, 12000.0)
            P.set_mode(ch, mode)
            P.set_am_passband(ch, -4900, 4900, 12000.0); P.squelch_setup(ch, 12000.0); P.squelch_set(ch, 0, 0)
            P.set_nr_algo(ch, algo)
            for ty in (0, 1):
                if algo == post.NR_WDSP:
                    for k, v in enumerate((taps, 16, 1e-4, 0.1)):
                        P.set_nr_param(ch, ty, k, v)
                elif algo == post.NR_ORIG:
                    P.set_nr_param(ch, ty, post.NR_DELAY, 0)
                if en[ty]:
                    P.set_nr_enable(ch, ty, 1)
        for _ in range(3):
            P.process_dev(chans, d_x, n, n, d_s, d_d, d_a, n)
        ctx.sync()
        ctx.timer_start()
        reps = 10
        for _ in range(reps):
            P.process_dev(chans, d_x, n, n, d_s, d_d, d_a, n)
        us = ctx.timer_stop() / reps * 1e3
        rt = n / 12000.0 / (us * 1e-6)
        print("nchan %5d %-20s %8.1f us per 512-sample pass, %7.0f x real time at 12 kHz" % (nchan, name, us, rt))
        P.close()
    for d in (d_x, d_s, d_d, d_a):
        ctx.free(d)
