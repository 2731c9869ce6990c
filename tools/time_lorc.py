"""Times the Loran-C extension (extensions/Loran_C/loran_c.cpp; kg_lorc_process): one call over 14 connections x 1 block of 512 samples,
both Loran channels of every connection under CMA, EMA and IIR (GRI 3990: 478.8 samples, so every block holds a bucket 0), once with a
row from every channel in the block (i_srate 0) and once with none (i_srate 10^9).  kg_lorc_process takes HOST arrays: a figure holds
two temporaries, the copies in and out, the kernel, the wait, the binding's array conversions and the host's schedule walk (made twice:
once ahead of the first copy so that a refused call enqueues nothing, once for the table).  The host's share is timed alone with
kg_lorc_plan, which makes that walk once and nothing else.  Every figure is the median of REPS timed batches of BATCH calls by the
host's clock; the spread is the batches' (max - min) / median.  Recorded, not gated, beside the 42.7 ms of signal a 512-sample block
represents at 12 kHz.
usage: python tools/time_lorc.py [out.txt]        (default profiles/lorc_time.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flydog_sdr_gps_amd import Context, lorc   # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lorc_time.txt")
ctx = Context(0)
lines = ["device %s, %d compute units; a block of 512 samples is 42.7 ms of signal at 12 kHz" % (ctx.name, ctx.num_cus)]
REPS, BATCH, NCONN = 7, 40, 14


def timed(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(BATCH):
            fn()
        t.append((time.perf_counter() - t0) / BATCH * 1e6)
    t = np.array(t)
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


rng = np.random.default_rng(1)
x = (900.0 * (rng.standard_normal((NCONN, 1, 512)) + 1j * rng.standard_normal((NCONN, 1, 512)))).astype(np.complex64)
conns, nblk = np.arange(NCONN, dtype=np.int32), np.ones(NCONN, np.int32)
rows = np.zeros(NCONN * 2 * 2 * 1200, np.uint8)
q = lorc.LoranC(ctx, nconn=NCONN)
for with_rows, i_srate in ((True, 0), (False, 10 ** 9)):
    for name, algo, param in (("CMA", lorc.CMA, 2), ("EMA", lorc.EMA, 8), ("IIR", lorc.IIR, 0.0005)):
        for c in range(NCONN):
            q.init(c, 12000.0, i_srate)
            for ch in range(2):
                q.set_gri(c, ch, 3990)
                q.set_avg_algo(c, ch, algo)
                q.set_avg_param(c, ch, param)
            q.start(c)
        q.process(conns, x, rows=rows, max_rows=64)                            # the restart's clear is behind it
        n = q.process(conns, x, rows=rows, max_rows=64)[1].size
        assert (n >= 2 * NCONN) == with_rows and (n == 0) != with_rows, n
        call = timed(lambda: q.process(conns, x, rows=rows, max_rows=64))
        plan = timed(lambda: q.plan(conns, nblk, 512))
        lines.append("%d connections x 1 block, %s, %-12s: call %7.1f us (spread %4.1f %%); the schedule walk alone %6.1f us (spread %4.1f %%), twice a call: "
                     "%4.1f %% of it" % (NCONN, name, "%d rows" % n if with_rows else "no row", call[0], 100 * call[1], plan[0], 100 * plan[1],
                                         100 * 2 * plan[0] / call[0]))
q.close()
ctx.close()
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
