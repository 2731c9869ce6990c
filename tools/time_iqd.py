"""Times the IQ display extension (extensions/IQ_display/iq_display.cpp; kg_iqd_process_dev): one call over 14 channels at one and four
blocks of 512 samples a channel, in points and in density mode (points 1024, auto gain), with the PLL off, on the 8th power and in the
two-PLL MSK mode.  Every figure is the median of REPS timed batches of BATCH calls between device events, each batch behind a drained
stream; the spread is the batches' (max - min) / median.  Recorded, not gated, beside the 42.7 ms of signal a 512-sample block
represents at 12 kHz.  The figures hold the binding's array conversions and the host's schedule walk besides the kernel.
usage: python tools/time_iqd.py [out.txt]        (default profiles/iqd_time.txt)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flydog_sdr_gps_amd import Context, iqd   # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "iqd_time.txt")
ctx = Context(0)
lines = ["device %s, %d compute units; a block of 512 samples is 42.7 ms of signal at 12 kHz" % (ctx.name, ctx.num_cus)]
REPS, BATCH, NCHAN = 7, 40, 14


def timed(fn):
    for _ in range(3):
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


for nblk in (1, 4):
    rng = np.random.default_rng(1)
    n = nblk * 512
    t = np.arange(n) / 12000.0
    x = np.stack([8000.0 * np.exp(2j * np.pi * (5.0 + ch) * t) + rng.normal(0, 100, n) + 1j * rng.normal(0, 100, n) for ch in range(NCHAN)]).astype(np.complex64)
    cap = NCHAN * (n + iqd.RING) * 4
    d_iq, d_rows, d_st = ctx.alloc(x.nbytes), ctx.alloc(cap), ctx.alloc(24 * NCHAN * nblk)
    ctx.upload(d_iq, x)
    chans, nb, inst = np.arange(NCHAN, dtype=np.int32), np.full(NCHAN, nblk, np.int32), np.zeros(NCHAN, np.int32)
    q = iqd.IqDisplay(ctx, nchan=NCHAN)

    def call():
        q.process_dev(chans, nb, inst, 512, d_iq, n, d_rows, cap, d_st, NCHAN * nblk, NCHAN * nblk)

    for draw, dname in ((iqd.POINTS, "points"), (iqd.DENSITY, "density")):
        res = {}
        for pname, mode, arg in (("PLL off", 0, 0), ("exponent 8", 1, 8), ("MSK", 2, 200)):
            for ch in range(NCHAN):
                q.init(ch)
                q.set_run(ch, 1, 12000.0)
                q.set_draw(ch, draw)
                q.set_pll_mode(ch, mode, arg)
            res[pname] = timed(call)
        lines.append("%d channels x %d block(s), %-7s: " % (NCHAN, nblk, dname) +
                     "; ".join("%s %7.1f us (spread %4.1f %%)" % (k, v[0], 100 * v[1]) for k, v in res.items()))
    q.close()
    for d in (d_iq, d_rows, d_st):
        ctx.free(d)
ctx.close()
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
