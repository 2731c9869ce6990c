"""Times kg_nav_push_bits_dev per call on 12 channels, at three sizes: `live` (one frame of new bits each: 8 C/A channels x 300 bits, 4
E1B channels x 500 symbols), `e1b_60s` (12 E1B channels x 15 000 symbols) and `ca_60s` (12 C/A channels x 3 000 bits).  The streams
are encoded frames back to back (flydog_sdr_gps_amd/nav.py), so every page is decoded and every subframe checked: the most a push of
that size has to do.  The same buffer is pushed again and again (it holds whole frames, so the stream continues).  Per size: a warm-up
round, then 5 rounds of `calls` pushes; the device time per call from events around a round, the host's enqueue time per call from a
clock around the same calls before the synchronise; median, minimum and maximum over the rounds.  The line names the GPU, the library
(sha256 of libkiwigpu.so) and the kernels' sources.  DESIGN.md 6.11 holds the measured figures next to tools/time_trk.py's.
usage: python tools/time_nav.py"""
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, _lib, nav   # noqa: E402

ctx = Context(0)
rng = np.random.Generator(np.random.PCG64(12))


def ca_stream(nframes):
    out, d = [], (0, 0)
    for k in range(nframes):
        w = [int(v) for v in rng.integers(0, 1 << 24, 10)]
        w[0] = (0x8B << 16) | (w[0] & 0xFFFF)
        f = nav.l1_subframe(w, *d)
        while f[-2] or f[-1]:
            w[9] = int(rng.integers(0, 1 << 24))
            f = nav.l1_subframe(w, *d)
        out.append(f)
    return np.concatenate(out)


def e1b_stream(npages):
    pages = []
    for k in range(npages):
        w = rng.integers(0, 2, 128).astype(np.uint8)
        w[:6] = [0, 0, 0, 0, (k >> 1) & 1, k & 1]
        pages.append(nav.e1b_page(w, reserved=rng.integers(0, 2, 64).astype(np.uint8)))
    return np.concatenate(pages)


def sha16(*paths):
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


CSRC = os.path.join(os.path.dirname(_lib.library_path()), "csrc")
out = {"gpu": ctx.name, "cus": ctx.num_cus, "abi": _lib.ABI_VERSION, "library_sha16": sha16(_lib.library_path()),
       "kg_nav_sources_sha16": sha16(os.path.join(CSRC, "kg_nav.h"), os.path.join(CSRC, "kg_nav.hip")), "nchan": 12}
SHAPES = (("live", [nav.L1] * 8 + [nav.E1B] * 4, 1, 2000), ("e1b_60s", [nav.E1B] * 12, 30, 200), ("ca_60s", [nav.L1] * 12, 10, 200))
for name, modes, nframes, calls in SHAPES:
    rows = [ca_stream(nframes) if m == nav.L1 else e1b_stream(nframes) for m in modes]
    nbits = [r.size for r in rows]
    stride = max(nbits)
    host = np.zeros((12, stride), np.uint8)
    for ch, r in enumerate(rows):
        host[ch, :r.size] = r
    cap = nav.cap_for(modes, nbits)
    d_bits, d_fr, d_cnt = ctx.alloc(host.nbytes), ctx.alloc(12 * cap * 64), ctx.alloc(48)
    ctx.upload(d_bits, host)
    ns = nav.NavSync(ctx, 12, modes)
    dev_us, host_us = [], []
    for rnd in range(6):                            # the first round is the warm-up
        ctx.sync()
        ctx.timer_start()
        t0 = time.perf_counter()
        for _ in range(calls):
            ns.push_dev(d_bits, stride, nbits, d_fr, cap, cap, d_cnt)
        t1 = time.perf_counter()
        ms = ctx.timer_stop()
        if rnd:
            dev_us.append(1000.0 * ms / calls)
            host_us.append(1e6 * (t1 - t0) / calls)
    counts = np.zeros(12, np.int32)
    ctx.download(d_cnt, counts)
    assert counts.tolist() == [nframes] * 12, counts     # every frame of the push was found and judged
    out[name] = {"bits_per_channel": nbits, "records_per_call": int(counts.sum()), "calls_per_round": calls,
                 "device_us_per_call": {"median": round(float(np.median(dev_us)), 2), "min": round(min(dev_us), 2), "max": round(max(dev_us), 2)},
                 "host_enqueue_us_per_call": {"median": round(float(np.median(host_us)), 2), "min": round(min(host_us), 2),
                                              "max": round(max(host_us), 2)}}
    ns.close()
    for p in (d_bits, d_fr, d_cnt):
        ctx.free(p)
print(json.dumps(out))
