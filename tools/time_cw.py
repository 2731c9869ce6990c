"""Times the CW decoder extension (extensions/CW_decoder/uhsdr_cw_decoder.cpp; kg_cw_push): one push over 14 connections x 64 blocks of
512 samples of the 30 wpm test signal of tests/cw_common.py (372 Goertzel blocks a connection and push, every one walked by the decoder's
single lane), one connection x 64 blocks, 14 connections x 1 block, and a receiver bank's step with one CW receiver against the same
bank never told about the extension -- which enqueues exactly what the bank enqueued before the extension existed.  kg_cw_push takes
HOST arrays: its figure holds three temporaries, the copies in and out, the kernel and two waits.  Every figure is the median of REPS
timed batches by the host's clock; the spread is the batches' (max - min) / median.  Recorded, not gated, beside the 2.73 s of signal
that 64 blocks represent at 12 kHz.
usage: python tools/time_cw.py [out.txt]        (default profiles/cw_time.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flydog_sdr_gps_amd import Context, CwDecoder, cw, synth  # noqa: E402
from flydog_sdr_gps_amd.rxbank import MIXES, RxBank           # noqa: E402
from tests import cw_common as cc                             # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cw_time.txt")
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


pool = cc.pool()
q = CwDecoder(ctx, nconn=NCONN)
for c in range(NCONN):
    q.start(c, 40)
    q.set_pboff(c, cc.PBOFF)
    q.set_threshold(c, 20000)
# connection c walks the clean signal from block 15 c on: training, characters and word spaces are all under way in one push
x = np.stack([pool[cc.AT["clean"] + 512 * 15 * c:][:512 * NB].reshape(NB, 512) for c in range(NCONN)])
now = [100] * NCONN
evs = q.push(list(range(NCONN)), x, now)
ne, nc = sum(e.size for e in evs), sum(int((e["kind"] == cw.CHARS).sum()) for e in evs)
call = timed(lambda: q.push(list(range(NCONN)), x, now), 10)
lines.append("%d connections x %d blocks, 30 wpm, %d events (%d cw_chars) in the first push: call %8.1f us (spread %4.1f %%)" % (NCONN, NB, ne, nc, call[0], 100 * call[1]))
one = timed(lambda: q.push([0], x[:1], now[:1]), 10)
lines.append(" 1 connection  x %d blocks: call %8.1f us (spread %4.1f %%)" % (NB, one[0], 100 * one[1]))
blk = timed(lambda: q.push(list(range(NCONN)), x[:, :1], now), 40)
lines.append("%d connections x  1 block : call %8.1f us (spread %4.1f %%)" % (NCONN, blk[0], 100 * blk[1]))
q.close()

# a bank's step: 14 receivers of the "light" mix in USB, wall time per step over 40 steps enqueued with no wait, then drained
N = 1 << 22


def bank_wall(with_cw):
    mix = MIXES["light"](NCONN, 0, N)
    bank = RxBank(NCONN, N)
    bank.configure(mix)
    for rx in range(NCONN):
        bank.set_audio(rx, mix[rx][2], -4900.0, 4900.0)
    if with_cw:
        bank.cw_start(0, 40, 12000.0, float(bank.fs))
        bank.cw_set_pboff(0, cc.PBOFF)
        bank.cw_set_threshold(0, 4000)
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
lines.append("bank of %d receivers, 4 Mi ADC samples a step (0.8 sound blocks): wall %7.1f us a step never told (spread %4.1f %%), %7.1f us with one CW receiver "
             "(spread %4.1f %%): %+6.1f us" % (NCONN, without[0], 100 * without[1], with_[0], 100 * with_[1], with_[0] - without[0]))
ctx.close()
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
