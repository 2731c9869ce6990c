"""Times the FFT extension (extensions/FFT/FFT.cpp; kg_fftext_process_dev): one call over 14 and 128 channels at one and four blocks a
channel, as wf (every block overwrites bin 0) and as integ (itime 3 s: 70 bins, the sums move between registers and memory whenever the
bin changes), beside kg_snd_spec_rows_dev on as many rows -- the library's other spectrum-to-bytes kernel, which keeps no sums.
Every figure is the median of REPS timed batches of BATCH calls between device events, each batch behind a drained stream; the spread
is the batches' (max - min) / median.  Recorded, not gated: at these sizes a call is expected to be bound by the host enqueueing its
launch and its table, not by the device (profiles/spec_time.txt found that for the row kernel).
usage: python tools/time_fftext.py [out.txt]        (default profiles/fftext_time.txt)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flydog_sdr_gps_amd import Context, fftext, snd   # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fftext_time.txt")
ctx = Context(0)
lines = ["device %s, %d compute units" % (ctx.name, ctx.num_cus)]
REPS, BATCH = 9, 400


def timed(fn):
    for _ in range(5):
        fn()
    ctx.sync()
    t = []
    for _ in range(REPS):
        ctx.timer_start()
        for _ in range(BATCH):
            fn()
        t.append(ctx.timer_stop() / BATCH * 1e3)
    t = np.array(t)
    return float(np.median(t)), float((t.max() - t.min()) / np.median(t))


for nchan in (14, 128):
    for nblk in (1, 4):
        rng = np.random.default_rng(1)
        spec = (rng.normal(0, 3e4, (nchan, nblk * 1024)) + 1j * rng.normal(0, 3e4, (nchan, nblk * 1024))).astype(np.complex64)
        d_spec, d_rows = ctx.alloc(spec.nbytes), ctx.alloc(nchan * nblk * 1024)
        ctx.upload(d_spec, spec)
        chans, nb, inst = np.arange(nchan, dtype=np.int32), np.full(nchan, nblk, np.int32), np.zeros(nchan, np.int32)
        inst_rows = np.zeros(nchan * nblk, np.int32)
        fx = fftext.FftExt(ctx, nchan=nchan, sample_rate=12000.0)

        def ext():
            fx.process_dev(chans, nb, inst, d_spec, nblk * 1024, d_rows, 1024, nchan * nblk)

        def rows():
            snd.spec_rows_dev(ctx, d_spec, 1024, inst_rows, d_rows, 1024)

        res = {}
        for name, run in (("wf", fftext.WF), ("integ", fftext.INTEG)):
            for ch in range(nchan):
                fx.set_itime(ch, 3.0)
                fx.set_run(ch, run)
            res[name] = timed(ext)
        res["spec rows"] = timed(rows)
        for ch in range(nchan):
            fx.set_run(ch, fftext.WF)
        res["wf again"] = timed(ext)
        lines.append("nchan %4d x %d block(s), %4d rows: " % (nchan, nblk, nchan * nblk) +
                     "; ".join("%s %7.1f us (spread %4.1f %%)" % (k, v[0], 100 * v[1]) for k, v in res.items()) +
                     "; integ / spec rows %.3f" % (res["integ"][0] / res["spec rows"][0]))
        fx.close()
        for d in (d_spec, d_rows):
            ctx.free(d)
ctx.close()
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
