"""Times kg_eph_push_frames_dev and kg_eph_sv_dev per call on 12 channels (8 C/A, 4 E1B): a push of 12 x 1 frame and of 12 x 50
frames (complete ephemerides over and over: every frame is applied), kg_eph_sv_dev at 12 and at 12 x 1000 snapshots of the Valid
satellites that leaves.  Per shape: a warm-up round, then 5 rounds of `calls` calls; the device time per call from events around a
round, the host's enqueue time per call from a clock around the same calls before the synchronise; median, minimum and maximum over
the rounds.  These are times of whole calls as a stream of them runs; the kernels' own times were not measured (no trace is taken).
The line names the GPU, the library (sha256 of libkiwigpu.so) and the kernels' sources.  DESIGN.md 6.12 holds the measured figures
next to the tracker's (profiles/nav_time.txt).
usage: python tools/time_eph.py"""
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, _lib, eph, nav   # noqa: E402

ctx = Context(0)
rng = np.random.Generator(np.random.PCG64(14))
KINDS = [eph.NAVSTAR] * 8 + [eph.E1B] * 4


def ri(lo, hi):
    return int(rng.integers(lo, hi))


def ca_frames(n):
    """n applied subframes 1, 2, 3, 1, ... of one plausible ephemeris"""
    f = {1: dict(week=200, IODC=9, t_oc=9000, a_f0=ri(-2 ** 20, 2 ** 20)),
         2: dict(IODE2=9, M_0=ri(-2 ** 31, 2 ** 31), e=ri(0, int(0.02 * 2 ** 33)), sqrtA=int(5153.6 * 2 ** 19), t_oe=9000, dn=10000),
         3: dict(IODE3=9, OMEGA_0=ri(-2 ** 31, 2 ** 31), i_0=int(0.3 * 2 ** 31), omega=ri(-2 ** 31, 2 ** 31), OMEGA_dot=-22000)}
    out = np.zeros(n, nav.frame_dtype)
    for k in range(n):
        sub = k % 3 + 1
        w = eph.subframe_words(sub, f[sub], tow=24000 + k)
        bits = np.array([(x >> (23 - j)) & 1 for x in w for j in range(24)], np.uint8).reshape(10, 24)
        out[k]["data"][:38] = np.packbits(np.concatenate([bits, np.zeros((10, 6), np.uint8)], axis=1).reshape(-1))      # the decode skips the parity bits
        out[k]["bit"], out[k]["consumed"], out[k]["id"] = 300 * k, 300, sub
    return out


def e1b_frames(n):
    f = {5: dict(week=1300, tow=144000), 1: dict(iodc=7, toes=2400, M0=ri(-2 ** 31, 2 ** 31), e=ri(0, 2 ** 23), sqrtA=int(5440.6 * 2 ** 19)),
         2: dict(iodc=7, OMG0=ri(-2 ** 31, 2 ** 31), i0=int(0.31 * 2 ** 31), omg=ri(-2 ** 31, 2 ** 31)), 3: dict(iodc=7, OMGd=-16000, deln=9000),
         4: dict(iodc=7, toc=2400, f0=ri(-2 ** 20, 2 ** 20))}
    out = np.zeros(n, nav.frame_dtype)
    for k in range(n):
        wt = (5, 1, 2, 3, 4)[k % 5]
        w = eph.inav_word(wt, f[wt])
        page = np.concatenate(([0, 0], w[:112], np.zeros(6, np.uint8), [1, 0], w[112:], np.zeros(102, np.uint8))).astype(np.uint8)
        out[k]["data"][:30] = np.packbits(page)
        out[k]["bit"], out[k]["consumed"], out[k]["id"] = 500 * k, 500, wt
    return out


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


CSRC = os.path.join(os.path.dirname(_lib.library_path()), "csrc")
out = {"gpu": ctx.name, "cus": ctx.num_cus, "abi": _lib.ABI_VERSION, "library_sha16": sha16(_lib.library_path()),
       "kg_eph_sources_sha16": sha16(os.path.join(CSRC, "kg_eph.h"), os.path.join(CSRC, "kg_eph.hip")), "nchan": 12}
e = eph.Ephemerides(ctx, 12)
for ch, kind in enumerate(KINDS):
    e.set_sat(ch, ch, kind)
for name, nframes, calls in (("push_12x1", 1, 2000), ("push_12x50", 50, 500)):
    host = np.stack([ca_frames(nframes) if k != eph.E1B else e1b_frames(nframes) for k in KINDS])
    d_fr, d_cnt, d_no = ctx.alloc(host.nbytes), ctx.alloc(48), ctx.alloc(12 * nframes * 32)
    ctx.upload(d_fr, host)
    ctx.upload(d_cnt, np.full(12, nframes, np.int32))
    out[name] = timed(lambda: e.push_frames_dev(d_fr, nframes, d_cnt, nframes, d_no, nframes), calls)
    notes = np.zeros((12, nframes), eph.note_dtype)
    ctx.download(d_no, notes)
    assert notes["applied"].all(), "every frame of the push was applied"
    out[name]["frames_per_call"] = 12 * nframes
    for p in (d_fr, d_cnt, d_no):
        ctx.free(p)
assert all(e.get(sat)["valid"] for sat in range(12))
for name, per_sat, calls in (("sv_12", 1, 2000), ("sv_12000", 1000, 500)):
    snaps = np.zeros(12 * per_sat, eph.snap_dtype)
    snaps["sat"] = np.arange(12 * per_sat) % 12
    snaps["bits"] = snaps["bits_tow"] = rng.integers(0, 300, snaps.size)
    snaps["chips"], snaps["cg_phase"], snaps["power"] = rng.integers(0, 1023, snaps.size), rng.integers(0, 64, snaps.size), 1e6
    d_in, d_out = ctx.alloc(snaps.nbytes), ctx.alloc(snaps.size * 48)
    ctx.upload(d_in, snaps)
    out[name] = timed(lambda: e.sv_dev(d_in, snaps.size, d_out), calls)
    got = np.zeros(snaps.size, eph.sv_dtype)
    ctx.download(d_out, got)
    assert (got["flags"] == 0).all() and np.isfinite(got["x"]).all(), "every snapshot was computed"
    out[name]["snapshots_per_call"] = int(snaps.size)
    ctx.free(d_in)
    ctx.free(d_out)
e.close()
print(json.dumps(out))
