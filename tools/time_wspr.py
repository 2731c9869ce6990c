"""Times stage 1 of the WSPR extension (extensions/wspr/; kg_wspr_push, kg_wspr_load): a whole cycle of 14 connections -- 88 callbacks of
512 samples each at 375 Hz, pushed 8 callbacks at a time (11 pushes, the last of which holds group 85 and enqueues the cycle end) --
then the pushes apart: one of 8 callbacks x 14 connections (7 groups a connection: 28 transforms and 7 rows), one of 2 callbacks, and the
cycle end by kg_wspr_load on the golden's planes: 12 candidates (12 workgroups, 1440 hypotheses of 162 symbols each) against a plane
without a peak (the copies in and the peak list alone); the difference is the search.  kg_wspr_push takes HOST arrays: its figures
hold four temporaries, the copies in and out, the kernels and the waits.  Every figure is the median of REPS timed batches by the
host's clock; the spread is the batches' (max - min) / median.  Recorded, not gated, beside the 120 s of signal a cycle represents.
Then a receiver bank's step (14 receivers, 4 Mi ADC samples): never told about the extension -- which enqueues exactly what the bank
enqueued before the extension existed --, with ONE receiver capturing and with ALL capturing (int_decimate 1, the densest schedule: a
group about every step and receiver), 40 steps enqueued with no wait, then drained.
usage: python tools/time_wspr.py [out.txt]        (default profiles/wspr_time.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flydog_sdr_gps_amd import Context, Wspr, synth     # noqa: E402
from flydog_sdr_gps_amd.rxbank import MIXES, RxBank     # noqa: E402
from tests import wspr_common as W               # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wspr_time.txt")
ctx = Context(0)
lines = ["device %s, %d compute units; a cycle is 45000 samples at 375 Hz: 120 s of signal" % (ctx.name, ctx.num_cus)]
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


pool = W.pool()
conns = list(range(NCONN))
# connection c walks the noise segment from sample 500 c on
x = np.stack([pool[W.AT["noise"] + 500 * c:][:W.CYCLE].reshape(-1, 512) for c in range(NCONN)])
clk = [W.clock(512 * b, 375, 0.0) for b in range(x.shape[1])]
mi, se = np.array([[m for m, s in clk]] * NCONN), np.array([[s for m, s in clk]] * NCONN)
q = Wspr(ctx, nconn=NCONN)


def cycle():
    ends = 0
    for c in conns:
        q.init(c, 375.0)
        q.set_capture(c, 1)
    for b in range(0, x.shape[1], NB):
        rows, m, ev, cy, counts = q.push(conns, x[:, b:b + NB], mi[:, b:b + NB], se[:, b:b + NB])
        ends += int(counts[:, 1].sum())
    return ends


assert cycle() == NCONN
whole = timed(cycle, 1)
lines.append("%d connections, a whole cycle in 11 pushes of %d callbacks of 512: %9.1f us (spread %4.1f %%): %6.1f us a connection and cycle" % (
    NCONN, NB, whole[0], 100 * whole[1], whole[0] / NCONN))


def burst(cs, nb):
    """capture off and on (the next callback starts a cycle), then nb callbacks in one push: nb - 1 groups a connection"""
    for c in cs:
        q.set_capture(c, 0)
        q.set_capture(c, 1)
    q.push(cs, x[:len(cs), :nb], 1, 7)


mid = timed(lambda: burst(conns, NB), 10)
lines.append("%d connections x %d callbacks (7 groups a connection, no cycle end): call %8.1f us (spread %4.1f %%)" % (NCONN, NB, mid[0], 100 * mid[1]))
one = timed(lambda: burst(conns, 2), 40)
lines.append("%d connections x 2 callbacks (1 group a connection):                 call %8.1f us (spread %4.1f %%)" % (NCONN, one[0], 100 * one[1]))
single = timed(lambda: burst([0], NB), 10)
lines.append(" 1 connection  x %d callbacks:                                        call %8.1f us (spread %4.1f %%)" % (NB, single[0], 100 * single[1]))
many, flat = W.planes(**W.LOADS["many"][0]), W.planes(**W.LOADS["flat"][0])
assert q.load(0, 0, *many)["npk"] == 12 and q.load(0, 0, *flat)["npk"] == 0
t12, t0 = timed(lambda: q.load(0, 0, *many), 10), timed(lambda: q.load(0, 0, *flat), 10)
lines.append("cycle end by kg_wspr_load (0.7 MB of planes in, one launch, the record out): 12 candidates %8.1f us (spread %4.1f %%), no peak %8.1f us "
             "(spread %4.1f %%): the search of 12 candidates %+7.1f us" % (t12[0], 100 * t12[1], t0[0], 100 * t0[1], t12[0] - t0[0]))
lines.append("the search: 12 workgroups of 256 lanes, 17280 hypotheses x 162 symbols x (1 ifd byte + 4 roots) read from LDS = 14 M LDS reads; ifd itself is "
             "evaluated 7290 times a candidate into LDS, not once a hypothesis and symbol; bound by one workgroup's latency (6 hypotheses a lane in turn), "
             "not by the card: 12 of %d compute units are busy" % ctx.num_cus)
q.close()

# a bank's step: 14 receivers of the "light" mix in USB, wall time per step over 40 steps enqueued with no wait, then drained
N = 1 << 22


def bank_wall(capturing):
    mix = MIXES["light"](NCONN, 0, N)
    bank = RxBank(NCONN, N)
    bank.configure(mix)
    for rx in range(NCONN):
        bank.set_audio(rx, mix[rx][2], -4900.0, 4900.0)
    for rx in range(capturing):
        bank.wspr_init(rx, 375.0)
        bank.wspr_set_capture(rx, 1)
    if capturing:
        bank.wspr_set_now(1, 7)
    adc = synth.adc_stream(N, 0x5EED0004)
    d_adc = bank.ctx.alloc(adc.nbytes)
    bank.ctx.upload(d_adc, adc)
    for _ in range(12):
        bank.step(d_adc)
    bank.sync()

    def run():
        for rx in range(capturing):                       # a cycle start each batch: the receivers never reach the wait at didx >= TPOINTS
            bank.wspr_set_capture(rx, 0)
            bank.wspr_set_capture(rx, 1)
        for _ in range(40):
            bank.step(d_adc)
        bank.sync()

    t = timed(run, 1)
    bank.ctx.free(d_adc)
    bank.close()
    return t[0] / 40, t[1]


never, one_rx, all_rx = bank_wall(0), bank_wall(1), bank_wall(NCONN)
lines.append("bank of %d receivers, 4 Mi ADC samples a step (0.8 sound blocks): wall %7.1f us a step never told (spread %4.1f %%), %7.1f us with one receiver capturing "
             "(spread %4.1f %%): %+6.1f us, %7.1f us with all %d capturing (spread %4.1f %%): %+6.1f us" % (
                 NCONN, never[0], 100 * never[1], one_rx[0], 100 * one_rx[1], one_rx[0] - never[0], all_rx[0], NCONN, 100 * all_rx[1], all_rx[0] - never[0]))
ctx.close()
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
