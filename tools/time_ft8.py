"""Times stage 1 of the FT8 / FT4 extension (extensions/FT8/; kg_ft8_push, kg_ft8_load_wf) of the stand-alone object: a push of 14
connections x 8 callbacks of 512 samples in the middle of an FT8 slot (2 or 3 blocks a connection: 4 or 6 transforms of 3840 points),
the same for FT4 (7 or 8 blocks: 14 or 16 transforms of 1152), and the slot end by kg_ft8_load_wf on a full FT8 waterfall: the golden's
e2e scene as the device's own monitor leaves it (140 candidates wanted, as many as pass kept) against the same waterfall with min_score
300 (nothing passes: sync scores and compaction alone); the difference is the heap's lane and the likelihoods.  kg_ft8_push takes HOST
arrays: its figures hold the temporaries, the copies in and out, the kernels and the waits.  Every figure is the median of REPS timed
batches by the host's clock; the spread is the batches' (max - min) / median.  Recorded, not gated, beside the 15 s of signal a slot
represents.  Then a receiver bank's step (14 receivers, 4 Mi ADC samples): never told about the extension -- which enqueues exactly what
the bank enqueued before the extension existed --, with ONE receiver started and with ALL started (FT4), 40 steps enqueued with no wait,
then drained; and, with all 14 started and every step waited for (16 Mi ADC samples a step), the step in which all 14 slots end against
the median step.  With KIWIGPU_PARENT_LIBRARY=<the parent commit's libkiwigpu.so> the never-told step is timed against the parent IN
ALTERNATION on this box: 7 rounds of one fresh process each, the median and the spread of both; without it the file says that no
parent was timed.
usage: python tools/time_ft8.py [out.txt]        (default profiles/ft8_time.txt)
       python tools/time_ft8.py --never-told     (one figure: microseconds a step; the alternation's child)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import subprocess                               # noqa: E402
from flydog_sdr_gps_amd import Context, Ft8, synth     # noqa: E402
from flydog_sdr_gps_amd.rxbank import MIXES, RxBank    # noqa: E402
from tests import ft8_common as F               # noqa: E402

N_ADC = 1 << 22


def bank_of(n, started, protocol=1):
    mix = MIXES["light"](14, 0, n)
    bank = RxBank(14, n)
    bank.configure(mix)
    for rx in range(14):
        bank.set_audio(rx, mix[rx][2], -4900.0, 4900.0)
    for rx in range(started):
        bank.ft8_init(rx, protocol)
        bank.ft8_start(rx)
    if started:
        bank.ft8_set_now(7500.8125)
    adc = synth.adc_stream(n, 0x5EED0008)
    d_adc = bank.ctx.alloc(adc.nbytes)
    bank.ctx.upload(d_adc, adc)
    return bank, d_adc


def bank_batch(started, reps):
    """-> microseconds a step of each of `reps` batches of 40 steps enqueued with no wait, then drained"""
    bank, d_adc = bank_of(N_ADC, started)
    for _ in range(12):
        bank.step(d_adc)
    bank.sync()
    out = []
    for _ in range(reps + 2):
        for rx in range(started):                         # a slot start each batch: no receiver reaches a slot end inside one
            bank.ft8_init(rx, 1)
        t0 = time.perf_counter()
        for _ in range(40):
            bank.step(d_adc)
        bank.sync()
        out.append((time.perf_counter() - t0) / 40 * 1e6)
    bank.ctx.free(d_adc)
    bank.close()
    return out[2:]


if len(sys.argv) > 1 and sys.argv[1] == "--never-told":
    if os.environ.get("KIWIGPU_LIBRARY"):                 # the parent's library has no kg_ft8_*: this Python binds the rest of it
        from flydog_sdr_gps_amd import _lib
        _lib.FT8_SYMBOLS.clear()
    print("%.3f" % float(np.median(bank_batch(0, 3))))
    sys.exit(0)

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ft8_time.txt")
ctx = Context(0)
lines = ["device %s, %d compute units; an FT8 slot is 15 s of signal at 12000 Hz, an FT4 slot 7.5 s" % (ctx.name, ctx.num_cus)]
REPS, NCONN, NB = 7, 14, 8


def timed(fn, batch):
    for _ in range(2):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(batch):
            fn()
        t.append((time.perf_counter() - t0) / batch * 1e6)
    t = np.array(t)
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


conns = list(range(NCONN))
for p in (F.FT8, F.FT4):
    x, t = F.STREAMS["e2e_" + F.pname(p)][1]()
    x, t = x[2:], t[2:]                                                   # from the sync on
    q = Ft8(ctx, nconn=NCONN)
    for c in conns:
        q.init(c, p)
    at = [0]

    def push():
        if at[0] + NB > 100:                                              # stay inside the slot: begin it again
            for c in conns:
                q.init(c, p)
            at[0] = 0
        q.push(conns, np.broadcast_to(x[at[0]:at[0] + NB], (NCONN, NB, F.NS)), np.broadcast_to(t[at[0]:at[0] + NB], (NCONN, NB)))
        at[0] += NB

    us, sp = timed(push, 10)
    lines.append("%s: 14 connections x 8 callbacks (%.1f blocks a connection, no slot end): call %8.1f us (spread %4.1f %%)" %
                 (F.pname(p).upper(), NB * F.NS / float(F.SIZES[p]["block"]), us, 100 * sp))
    q.close()

x, t = F.STREAMS["e2e_ft8"][1]()
q = Ft8(ctx, nconn=1)
q.init(0, F.FT8)
for b in range(0, x.shape[0], 40):
    q.push([0], x[None, b:b + 40], t[None, b:b + 40])
mag = q.state(0, previous=True)[2]
n = int(q.load_wf(0, F.FT8, mag)["ncand"])
a, sa = timed(lambda: q.load_wf(0, F.FT8, mag), 10)
b, sb = timed(lambda: q.load_wf(0, F.FT8, mag, 140, 300), 10)
p140, kw140, n140, ms140 = F.LOADS["load_a_ft8"]
mag140 = F.waterfall(p140, **kw140)
k140 = int(q.load_wf(0, p140, mag140, n140, ms140)["ncand"])
d, sd = timed(lambda: q.load_wf(0, p140, mag140, n140, ms140), 10)
e, se = timed(lambda: q.load_wf(0, p140, mag140, n140, 300), 10)
const = np.full_like(mag, 100)
c, sc = timed(lambda: q.load_wf(0, F.FT8, const, 140, 0), 5)
lines.append("slot end by kg_ft8_load_wf (177 KB of waterfall in, three launches, the 100 KB record out): %d candidates %8.1f us (spread %4.1f %%), none %8.1f us "
             "(spread %4.1f %%): the heap's lane and the likelihoods %+.1f us; a constant waterfall at min_score 0 (all 56880 hypotheses through the one lane) %8.1f us (spread %4.1f %%)"
             % (n, a, 100 * sa, b, 100 * sb, a - b, c, 100 * sc))
lines.append("slot end on the golden's load_a_ft8 (50 blocks, 769 hypotheses pass): %d candidates kept %8.1f us (spread %4.1f %%), none (min_score 300) %8.1f us (spread %4.1f %%): "
             "the heap's lane and 140 likelihoods %+.1f us" % (k140, d, 100 * sd, e, 100 * se, d - e))
q.close()
ctx.close()


def med(v):
    v = np.array(v)
    return float(np.median(v)), float((v.max() - v.min()) / np.median(v))


never, one_rx, all_rx = med(bank_batch(0, REPS)), med(bank_batch(1, REPS)), med(bank_batch(14, REPS))
lines.append("bank of 14 receivers, 4 Mi ADC samples a step (0.8 sound blocks): wall %7.1f us a step never told (spread %4.1f %%), %7.1f us with one receiver started "
             "(spread %4.1f %%): %+6.1f us, %7.1f us with all 14 started (spread %4.1f %%): %+6.1f us" % (
                 never[0], 100 * never[1], one_rx[0], 100 * one_rx[1], one_rx[0] - never[0], all_rx[0], 100 * all_rx[1], all_rx[0] - never[0]))
bank, d_adc = bank_of(1 << 24, 14)
steps, end_step = [], None
for k in range(60):
    bank.ft8_set_now(7500.8125 + 0.14 * k)
    t0 = time.perf_counter()
    bank.step(d_adc)
    bank.sync()
    steps.append((time.perf_counter() - t0) * 1e6)
    if len(bank.ft8_out()[1]) == 14:
        end_step = k
bank.ctx.free(d_adc)
bank.close()
lines.append("bank of 14 receivers all started (FT4), 16 Mi ADC samples a step (3.1 sound blocks), every step waited for: median step %8.1f us; the step in which all 14 slots end "
             "(step %s): %8.1f us" % (float(np.median(steps)), end_step, steps[end_step] if end_step is not None else float("nan")))
parent = os.environ.get("KIWIGPU_PARENT_LIBRARY")
if parent:
    mine, theirs = [], []
    for _ in range(7):
        for lib, dst in ((None, mine), (parent, theirs)):
            env = dict(os.environ)
            env.pop("KIWIGPU_PARENT_LIBRARY")
            if lib:
                env["KIWIGPU_LIBRARY"] = lib
            dst.append(float(subprocess.run([sys.executable, os.path.abspath(__file__), "--never-told"], env=env, capture_output=True, text=True, check=True).stdout.split()[-1]))
    a, b = med(mine), med(theirs)
    lines.append("the never-told step against the parent commit's library, in alternation on this box, 7 rounds of a fresh process each (each figure the median of 3 batches "
                 "of 40 steps): this commit %7.1f us (spread %4.1f %%), the parent %7.1f us (spread %4.1f %%): %+.1f us" % (a[0], 100 * a[1], b[0], 100 * b[1], a[0] - b[0]))
else:
    lines.append("the parent commit was NOT timed in alternation on this box (no KIWIGPU_PARENT_LIBRARY): the never-told figure above stands alone")
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
