"""Times the FAX extension (extensions/FAX/FaxDecoder.cpp; kg_fax_push): one push over 14 connections x 64 blocks of 512 samples of the
120 lpm test signal of tests/fax_common.py (5.5 lines a connection and push; every line demodulated, detected and decoded, the phasing
lines searched), and a receiver bank's step with one FAX receiver against the same bank never told about the extension -- which
enqueues exactly what the bank enqueued before the extension existed.  kg_fax_push takes HOST arrays: its figure holds four
temporaries, the copies in and out, the kernel and two waits.  Every figure is the median of REPS timed batches by the host's clock;
the spread is the batches' (max - min) / median.  Recorded, not gated, beside the 2.73 s of signal that 64 blocks represent at 12 kHz.
usage: python tools/time_fax.py [out.txt]        (default profiles/fax_time.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flydog_sdr_gps_amd import Context, FaxDecoder, synth   # noqa: E402
from flydog_sdr_gps_amd.rxbank import MIXES, RxBank          # noqa: E402
from tests import fax_common as fc                           # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fax_time.txt")
ctx = Context(0)
lines = ["device %s, %d compute units; 64 blocks of 512 samples are 2.73 s of signal at 12 kHz" % (ctx.name, ctx.num_cus)]
REPS, NCONN, NB = 7, 14, 64


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


pool = fc.pool()
q = FaxDecoder(ctx, nconn=NCONN)
for c in range(NCONN):
    q.start(c, lpm=120)
# connection c walks the signal from block 20 c on: start tone, phasing lines and image lines are all under way in one push
x = np.stack([pool[fc.AT["a120"] + 512 * 20 * c:][:512 * NB].reshape(NB, 512) for c in range(NCONN)])
rates = [12000.0] * NCONN
recs, rows = q.push(list(range(NCONN)), x, rates)
nl, nr = sum(r.size for r in recs), sum(r.shape[0] for r in rows)
call = timed(lambda: q.push(list(range(NCONN)), x, rates), 10)
lines.append("%d connections x %d blocks, 120 lpm, %d lines and %d rows in the first push: call %8.1f us (spread %4.1f %%)" % (NCONN, NB, nl, nr, call[0], 100 * call[1]))
one = timed(lambda: q.push([0], x[:1], rates[:1]), 10)
lines.append(" 1 connection  x %d blocks: call %8.1f us (spread %4.1f %%)" % (NB, one[0], 100 * one[1]))
blk = timed(lambda: q.push(list(range(NCONN)), x[:, :1], rates), 40)
lines.append("%d connections x  1 block : call %8.1f us (spread %4.1f %%)" % (NCONN, blk[0], 100 * blk[1]))
q.close()

# a bank's step: 14 receivers of the "light" mix in USB, wall time per step over 40 steps enqueued with no wait, then drained
N = 1 << 22


def bank_wall(with_fax):
    mix = MIXES["light"](NCONN, 0, N)
    bank = RxBank(NCONN, N)
    bank.configure(mix)
    for rx in range(NCONN):
        bank.set_audio(rx, mix[rx][2], -4900.0, 4900.0)
    if with_fax:
        bank.fax_start(0, lpm=120, srate=float(bank.fs))
    adc = synth.adc_stream(N, 0x5EED0004)
    d_adc = bank.ctx.alloc(adc.nbytes)
    bank.ctx.upload(d_adc, adc)
    for _ in range(12):
        bank.step(d_adc)
    bank.sync()

    def run():
        for _ in range(40):
            bank.step(d_adc)
        bank.sync()

    t = timed(run, 1)
    bank.ctx.free(d_adc)
    bank.close()
    return t[0] / 40, t[1]


without, with_ = bank_wall(False), bank_wall(True)
lines.append("bank of %d receivers, 4 Mi ADC samples a step (0.8 sound blocks): wall %7.1f us a step never told (spread %4.1f %%), %7.1f us with one FAX receiver "
             "at 120 lpm (spread %4.1f %%): %+6.1f us" % (NCONN, without[0], 100 * without[1], with_[0], 100 * with_[1], with_[0] - without[0]))
ctx.close()
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
