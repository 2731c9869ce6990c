"""Times stage 2 of the WSPR extension (kg_wspr_decode; include/kiwigpu_wspr_dec.h) on the scene `timeup_a` of tests/wspr_dec_common.py --
a candidate that passes minsync1, passes the gate on some jiggles and never decodes: every jiggle and every Fano run is paid for -- as 1
candidate, as 12 candidates of one connection and as 14 connections x 12.  Each call is loaded afresh (ignore cleared) outside the timed
region.  kg_wspr_decode takes HOST arrays: its figures hold two temporaries, the table of connections, the chain of 17 launches, the
records' copy out and the wait.  The split between the sync kernels and the Fano kernel is taken as the difference between a pass at
maxcycles M and the same pass at maxcycles 1 (81 cycles a set: the Fano kernel all but empty).  Then the worst Fano case: a pass at
(10000, 1) with 12 time-up candidates, 129 jiggles each.  And, because the cycle-end kernel of stage 1 now also stores the held
candidates, the cycle end by kg_wspr_load as tools/time_wspr.py times it, to set against profiles/wspr_time.txt.  Then a receiver
bank's step by that tool's method -- never told, one receiver capturing, the same with decode on -- and the one step that holds a cycle
end, with and without pass 0 behind it.
Every figure is the median of REPS timed calls by the host's clock; the spread is (max - min) / median.  Recorded, not gated.
usage: python tools/time_wspr_decode.py [out.txt]        (default profiles/wspr_decode_time.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flydog_sdr_gps_amd import Context, Wspr     # noqa: E402
from tests import wspr_common as W1              # noqa: E402
from tests import wspr_dec_common as W           # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wspr_decode_time.txt")
ctx = Context(0)
lines = ["device %s, %d compute units; a candidate is 162 symbols x 4 tones x 256 samples a hypothesis" % (ctx.name, ctx.num_cus)]
REPS, NCONN = 7, 14
g = W.load()
x, cands, _ = W.scene_inputs("timeup_a")
cand = tuple(cands.tolist()[0])
q = Wspr(ctx, nconn=NCONN)
q.set_metric_table(g["mettab"])
for c in range(NCONN):
    q.init(c, 375.0)


def timed(conns, ncand, maxcycles, iifac):
    t, res = [], None
    for r in range(REPS + 2):
        for c in conns:
            q.load_iq(c, 0, x, [cand] * ncand)
        t0 = time.perf_counter()
        res = q.decode(conns, maxcycles, iifac)
        if r >= 2:
            t.append((time.perf_counter() - t0) * 1e6)
    t = np.array(t)
    assert (res[0][:, :ncand]["result"] == W.TIME_UP).all() or maxcycles == 1
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t)), res


for conns, ncand, what in (([0], 1, " 1 candidate"), ([0], 12, "12 candidates of one connection"), (list(range(NCONN)), 12, "14 connections x 12 candidates")):
    full, empty = timed(conns, ncand, 200, 2), timed(conns, ncand, 1, 2)
    gates = int(full[2][0][:, :ncand]["gates"].sum())
    lines.append("pass 0 (200, 2), %-32s call %9.1f us (spread %4.1f %%); at maxcycles 1 %9.1f us (spread %4.1f %%): the Fano kernel %+9.1f us for %d gated jiggles of "
                 "%d run" % (what + ":", full[0], 100 * full[1], empty[0], 100 * empty[1], full[0] - empty[0], gates, 65 * ncand * len(conns)))
worst, base = timed([0], 12, 10000, 1), timed([0], 12, 1, 1)
lines.append("pass (10000, 1), 12 time-up candidates, 129 jiggles each: call %9.1f us (spread %4.1f %%); at maxcycles 1 %9.1f us (spread %4.1f %%): the Fano kernel %+9.1f us "
             "for %d runs of 810000 cycles" % (worst[0], 100 * worst[1], base[0], 100 * base[1], worst[0] - base[0], int(worst[2][0][:, :12]["gates"].sum())))
lines.append("the sync side of a pass is 6 x (corr + pick) + corr + soft: 162 workgroups a candidate and launch; a lane runs one tone's recurrence once and "
             "adds into 5 lags (lag calls, jiggles) or 1 (frequency calls); the Fano kernel is one lane a gated jiggle, 32 lanes a workgroup, bound by "
             "the longest lane: a reading of the code, not a measurement")
many = W1.planes(**W1.LOADS["many"][0])
assert q.load(0, 0, *many)["npk"] == 12


def batched(fn, batch, reps=REPS):
    """tools/time_wspr.py's method: the median of `reps` timed batches by the host's clock, spread (max - min) / median"""
    for _ in range(2):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(batch):
            fn()
        t.append((time.perf_counter() - t0) / batch * 1e6)
    t = np.array(t)
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


t12 = batched(lambda: q.load(0, 0, *many), 10)
lines.append("stage 1's cycle end by kg_wspr_load, 12 candidates, with the held list stored too: %8.1f us (spread %4.1f %%), batches of 10 as tools/time_wspr.py "
             "takes it; profiles/wspr_time.txt has 388.2 us (spread 1.4 %%) for the parent" % (t12[0], 100 * t12[1]))
q.close()

# a receiver bank's step, by the method of tools/time_wspr.py (14 receivers of the "light" mix in USB, 4 Mi ADC samples a step, 40 steps
# enqueued with no wait, then drained): never told; one receiver capturing with decode on (no cycle end in the 40 steps)
from flydog_sdr_gps_amd import synth                    # noqa: E402
from flydog_sdr_gps_amd.rxbank import MIXES, RxBank     # noqa: E402
N = 1 << 22


def make_bank(n, capturing, decode):
    mix = MIXES["light"](NCONN, 0, N)
    bank = RxBank(NCONN, n)
    bank.configure(MIXES["light"](NCONN, 0, n))
    for rx in range(NCONN):
        bank.set_audio(rx, mix[rx][2], -4900.0, 4900.0)
    if decode:
        bank.wspr_set_metric_table(g["mettab"])
    for rx in range(capturing):
        bank.wspr_init(rx, 375.0)
        bank.wspr_set_capture(rx, 1)
        if decode:
            bank.wspr_set_decode(rx, 1)
    if capturing:
        bank.wspr_set_now(1, 7)
    adc = synth.adc_stream(n, 0x5EED0004)
    d_adc = bank.ctx.alloc(adc.nbytes)
    bank.ctx.upload(d_adc, adc)
    return bank, d_adc


def bank_wall(capturing, decode):
    bank, d_adc = make_bank(N, capturing, decode)
    for _ in range(12):
        bank.step(d_adc)
    bank.sync()

    def run():
        for rx in range(capturing):                       # a cycle start each batch: the receiver never reaches a cycle end
            bank.wspr_set_capture(rx, 0)
            bank.wspr_set_capture(rx, 1)
        for _ in range(40):
            bank.step(d_adc)
        bank.sync()

    t = batched(run, 1)
    bank.ctx.free(d_adc)
    bank.close()
    return t[0] / 40, t[1]


never, cap, dec = bank_wall(0, False), bank_wall(1, False), bank_wall(1, True)
lines.append("bank of %d receivers, 4 Mi ADC samples a step: wall %7.1f us a step never told (spread %4.1f %%; profiles/wspr_time.txt: 520.8 us, 1.4 %%), %7.1f us with one "
             "receiver capturing (spread %4.1f %%; there 548.9 us, 1.7 %%), %7.1f us with its decode on and no cycle end (spread %4.1f %%): %+6.1f us on the capturing step "
             "-- such a step launches nothing new" % (NCONN, never[0], 100 * never[1], cap[0], 100 * cap[1], dec[0], 100 * dec[1], dec[0] - cap[0]))


def cycle_end_step(decode):
    """steps of 32 Mi samples (6.4 sound blocks): the step that holds the receiver's cycle end, enqueued and drained alone, decode off / on"""
    bank, d_adc = make_bank(8 * N, 1, decode)
    t = []
    for rep in range(REPS + 1):
        bank.wspr_set_capture(0, 0)
        bank.wspr_set_capture(0, 1)
        for k in range(24):
            bank.sync()
            t0 = time.perf_counter()
            bank.step(d_adc)
            bank.sync()
            dt = (time.perf_counter() - t0) * 1e6
            if len(bank.wspr_out()[3]):                     # the cycle record is due: this was the step
                if rep:
                    t.append(dt)
                break
        else:
            raise SystemExit("no cycle end in 24 steps")
    bank.ctx.free(d_adc)
    bank.close()
    t = np.array(t)
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


e_off, e_on = cycle_end_step(False), cycle_end_step(True)
lines.append("the step that holds a cycle end (32 Mi samples a step, one receiver capturing, drained alone): %8.1f us with decode off (spread %4.1f %%), %8.1f us with pass 0 "
             "behind it (spread %4.1f %%): %+8.1f us, the chain of 17 launches for up to 12 candidates on the tail stream" % (
                 e_off[0], 100 * e_off[1], e_on[0], 100 * e_on[1], e_on[0] - e_off[0]))
ctx.close()
text = "\n".join(lines) + "\n"
print(text, end="")
with open(out_path, "w") as f:
    f.write(text)
