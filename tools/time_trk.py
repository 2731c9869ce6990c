"""Times kg_trk_process_bits_dev: 12 tracking channels (8 C/A, 4 E1B, distinct rates) over 1 s of 1-bit stream (16.368 M clocks) in ONE
call, and in 100 calls of 10 ms.  The stream is noise, so every channel services every epoch with the loops closed on noise: the cost
does not depend on lock.  The line it prints names the GPU, the library (sha256 of libkiwigpu.so) and the kernel's sources.  The requirement is the stream's own: faster than real time (DESIGN.md 6.10 holds the measured figure).
usage: python tools/time_trk.py [nchan]"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flydog_sdr_gps_amd import Context, trk   # noqa: E402

FS = 16368000
nchan = int(sys.argv[1]) if len(sys.argv) > 1 else 12
ctx = Context(0)
rng = np.random.Generator(np.random.PCG64(3))
bits = rng.integers(0, 256, FS // 8, dtype=np.uint8)
d_bits = ctx.alloc(bits.nbytes)
ctx.upload(d_bits, bits)
cap = trk.cap_for(FS)
d_ep = ctx.alloc(nchan * cap * trk.epoch_dtype.itemsize)
d_cnt = ctx.alloc(4 * nchan)


def tracker():
    t = trk.Tracker(ctx, nchan)
    for ch in range(nchan):
        e1b = ch % 3 == 2
        t.set_sat(ch, trk.E1B_MODE | ch if e1b else ((ch % 9 + 1) << 4) + 10)
        if e1b:
            t.set_e1b_code(ch, rng.integers(0, 2, 4092, dtype=np.uint8))
        t.set_rate_cg(ch, (1 << 28) + 700 * (ch - 6))
        t.set_rate_lo(ch, (1 << 30) + 200000 * (ch - 6))
        lo, cg = trk.gains(e1b)
        t.set_gain_lo(ch, *lo)
        t.set_gain_cg(ch, *cg)
    t.sampler_reset()
    return t


def sha16(*paths):
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


from flydog_sdr_gps_amd import _lib   # noqa: E402
CSRC = os.path.join(os.path.dirname(_lib.library_path()), "csrc")
out = {"gpu": ctx.name, "cus": ctx.num_cus, "abi": _lib.ABI_VERSION, "library_sha16": sha16(_lib.library_path()),
       "kg_trk_sources_sha16": sha16(os.path.join(CSRC, "kg_trk.h"), os.path.join(CSRC, "kg_trk.hip")), "nchan": nchan, "clocks": FS}
for name, pieces in (("one_call", 1), ("calls_of_10ms", 100)):
    best = 1e30
    for rnd in range(4):                        # the first round is the warm-up
        t = tracker()
        n = FS // pieces
        t.process_dev(d_bits, 8, d_ep, cap, cap, d_cnt)      # uploads the state; 8 clocks keep the next call byte-aligned
        ctx.sync()
        ctx.timer_start()
        for k in range(pieces):
            t.process_dev(d_bits + 1 + k * n // 8, n - (8 if k == pieces - 1 else 0), d_ep, cap, cap, d_cnt)
        ms = ctx.timer_stop()
        counts = np.zeros(nchan, np.int32)
        ctx.download(d_cnt, counts)
        t.close()
        if rnd:
            best = min(best, ms)
    out[name + "_ms"] = round(best, 3)
    out[name + "_x_real_time"] = round(1000.0 / best, 1)
    out[name + "_last_counts"] = counts.tolist()
print(json.dumps(out))
