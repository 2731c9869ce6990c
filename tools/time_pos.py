"""Times kg_pos_solve_dev per call at 1 epoch and at 32 epochs of 12 rows (twelve satellites in view of a fixed receiver, Kalman on, the
three solvers: plot_e1b on), the rows on the device.  Per shape: a warm-up round, then 5 rounds of `calls` calls; the device time per
call from events around a round, the host's enqueue time per call from a clock around the same calls before the synchronise; median,
minimum and maximum over the rounds.  These are times of whole calls as a stream of them runs (the EKF converged, every epoch a
12-satellite SPP solve and an EKF update per solver); the kernel's own time was not measured (no trace is taken).  The line names the
GPU, the library (sha256 of libkiwigpu.so) and the kernel's sources.  DESIGN.md 6.13 holds the measured figures next to
kg_eph_sv_dev's (profiles/eph_time.txt).
usage: python tools/time_pos.py"""
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, _lib, eph, pos   # noqa: E402

ctx = Context(0)
rng = np.random.Generator(np.random.PCG64(15))
AZEL = [(10, 60), (80, 30), (150, 45), (220, 20), (300, 70), (350, 15), (45, 80), (120, 10), (200, 55), (260, 35), (330, 12), (30, 25)]
SATS = [0, 3, 7, 12, 33, 36, 40, 45, 50, 20, 25, 30]


def sha16(*paths):
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def timed(call, calls):
    dev_us, host_us = [], []
    for rnd in range(6):                            # the first round is the warm-up
        ctx.sync()
        ctx.timer_start()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        t1 = time.perf_counter()
        ms = ctx.timer_stop()
        if rnd:
            dev_us.append(1000.0 * ms / calls)
            host_us.append(1e6 * (t1 - t0) / calls)
    return {"calls_per_round": calls,
            "device_us_per_call": {"median": round(float(np.median(dev_us)), 2), "min": round(min(dev_us), 2), "max": round(max(dev_us), 2)},
            "host_enqueue_us_per_call": {"median": round(float(np.median(host_us)), 2), "min": round(min(host_us), 2), "max": round(max(host_us), 2)}}


def epochs(n):
    """n epochs of the same instant seen through fresh noise: the receiver's clock stands, the tick count runs (see below), osc_corr is 0"""
    sn, sv = np.zeros((n, 12), eph.snap_dtype), np.zeros((n, 12), eph.sv_dtype)
    for e in range(n):
        rows = pos.scene_rows((16.3, 48.2, 200.0), 100000.0, AZEL, range_error=rng.normal(0, 2.0, 12))
        sv[e]["x"], sv[e]["y"], sv[e]["z"], sv[e]["ct"], sv[e]["week"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], 2200
        sn[e]["sat"], sn[e]["power"] = SATS, 1e6
    return sn, sv


CSRC = os.path.join(os.path.dirname(_lib.library_path()), "csrc")
out = {"gpu": ctx.name, "cus": ctx.num_cus, "abi": _lib.ABI_VERSION, "library_sha16": sha16(_lib.library_path()),
       "kg_pos_sources_sha16": sha16(os.path.join(CSRC, "kg_pos.h"), os.path.join(CSRC, "kg_pos.hip")), "nrow": 12}
p = pos.PositionSolver(ctx)
p.set_mode(1, 1)
for name, n, calls in (("solve_1", 1, 1000), ("solve_32", 32, 100)):
    sn, sv = epochs(n)
    tk = 1000 + np.arange(6 * calls * n, dtype=np.uint64) * np.uint64(pos.F_OSC)      # a tick count that runs on from call to call: dt is 1 s
    d_sn, d_sv, d_tk, d_out = ctx.alloc(sn.nbytes), ctx.alloc(sv.nbytes), ctx.alloc(tk.nbytes), ctx.alloc(n * pos.epoch_dtype.itemsize)
    ctx.upload(d_sn, sn)
    ctx.upload(d_sv, sv)
    ctx.upload(d_tk, tk)
    at = [0]

    def call():
        p.solve_dev(d_sn, d_sv, 12, n, d_tk + 8 * n * at[0], None, d_out)
        at[0] += 1

    out[name] = timed(call, calls)
    assert at[0] == 6 * calls
    got = np.zeros(n, pos.epoch_dtype)
    ctx.download(d_out, got)
    want = pos.CALLED | pos.POS_VALID | pos.SPP_VALID | pos.EKF_VALID
    assert (got["fix"]["flags"] == want).all() and (got["fix"]["ekf_running"] == 4).all(), "every epoch was an SPP solve and an EKF update in all three solvers"
    out[name]["epochs_per_call"] = n
    out[name]["device_us_per_epoch"] = round(out[name]["device_us_per_call"]["median"] / n, 2)
    for d in (d_sn, d_sv, d_tk, d_out):
        ctx.free(d)
    p.reset()
p.close()
print(json.dumps(out))
