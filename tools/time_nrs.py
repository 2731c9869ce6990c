"""Times kg_post_process_dev with the spectral noise reduction (NR_SPECTRAL, rx/Teensy/NR_spectral.cpp) on every channel of a batch
of SSB receiver channels, 512 samples per channel and launch (c2s_sound()'s ns_out), past its start-up phase; and in the same run
NR_WDSP at 64 taps with one type enabled and NR off, the two rows it is held against ("Spectral noise reduction").
usage: python tools/time_nrs.py [nchan ...]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, Post, post   # noqa: E402

CASES = ["SSB, NR off", "WDSP 64 denoise", "spectral", "SSB, NR off (again)"]

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
    for name in CASES:
        P = Post(ctx, nchan=nchan)
        for ch in range(nchan):
            P.set_agc(ch, True, ch & 1, -100, 50, 6, 1000, 12000.0)
            P.set_smeter(ch, 12000.0)
            P.set_mode(ch, post.MODE_SSB)
            if name.startswith("WDSP"):
                P.set_nr_algo(ch, post.NR_WDSP)
                for k, v in enumerate((64, 16, 1e-4, 0.1)):
                    P.set_nr_param(ch, post.NR_DENOISE, k, v)
                P.set_nr_enable(ch, post.NR_DENOISE, 1)
            elif name == "spectral":
                P.nrs_passband(ch, 300.0, 2700.0)
                P.nrs_select(ch)
                for k, v in enumerate((1.0, 0.95, 1000.0)):
                    P.set_nr_param(ch, post.NR_DENOISE, k, v)
        for _ in range(12):                                 # 24 frames: past the 20 frames of the start-up phase
            P.process_dev(chans, d_x, n, n, d_s, d_d, d_a, n)
        ctx.sync()
        if name == "spectral":
            assert (P.nrs_state(chans[:4])["ints"][:, 0] == 3).all()
        best, total, rounds, reps = 1e30, 0.0, 5, 10
        for _ in range(rounds):
            ctx.timer_start()
            for _ in range(reps):
                P.process_dev(chans, d_x, n, n, d_s, d_d, d_a, n)
            us = ctx.timer_stop() / reps * 1e3
            best = min(best, us); total += us
        rt = n / 12000.0 / (total / rounds * 1e-6)
        print("nchan %5d %-20s %8.1f us per 512-sample pass (best of %d rounds %8.1f), %7.0f x real time at 12 kHz"
              % (nchan, name, total / rounds, rounds, best, rt))
        P.close()
    for d in (d_x, d_s, d_d, d_a):
        ctx.free(d)
