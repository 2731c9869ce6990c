"""The FFT extension over the C ABI (kg_fftext): the one consumer of receive_FFT(POST_FILTERED).

Reference                                                       here
  fft_msgs  `SET run=`    extensions/FFT/FFT.cpp:206-244          -> FftExt.set_run
            `SET itime=`  :246-252                                -> FftExt.set_itime
            `SET clear`   :254-258                                -> FftExt.clear
  fft_data  :69-191                                               -> FftExt.process / process_dev; the limiter (:174-186): FftExt.due

The spectra are what kg_fir_process_taps_dev / kg_fir_process_spec_dev leave in d_post.  The message of :188 is bytes([bin]) + row.
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, ptr  # noqa: F401

OFF, WF, SPEC, INTEG = -1, 0, 1, 2              # KG_FFTEXT_*: FUNC_OFF .. FUNC_INTEG (FFT.cpp:66)
PASSBAND, CHAN_NULL = 0, 1                      # KG_SPEC_*
ROW, MAX_BINS, UPDATE_MS = 1024, 200, 100

info_dtype = np.dtype([("run", "<i4"), ("instance", "<i4"), ("fft_scale", "<f4"), ("spectrum_scale", "<f4"), ("bins", "<i4"), ("reset", "<i4"),
                       ("last_ms", "<u4"), ("reserved", "<i4"), ("fi", "<f8"), ("fft_sec", "<f8"), ("time", "<f8")])
assert info_dtype.itemsize == 56


class FftExt:
    """nchan channels of fft_t (FFT.cpp:40-59) on the GPU (kg_fftext): 200 x 1024 sums each"""

    def __init__(self, ctx=None, nchan=1, sample_rate=None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nchan = int(nchan)
        h = C.c_void_p()
        check(self.lib.kg_fftext_create(self.ctx.h, int(nchan), C.byref(h)), "kg_fftext_create")
        self.h = h
        if sample_rate is not None:
            self.set_rate(sample_rate)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None) and not getattr(self, "_borrowed", False):       # a receiver bank's object is the bank's
                self.lib.kg_fftext_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_rate(self, sample_rate):
        check(self.lib.kg_fftext_set_rate(self.h, float(sample_rate)), "kg_fftext_set_rate")

    def set_run(self, ch, run, is_sam=False, is_qam=False):
        """`SET run=`; is_sam / is_qam: snd->isSAM and snd->mode == MODE_QAM at the command"""
        check(self.lib.kg_fftext_set_run(self.h, int(ch), int(run), int(bool(is_sam)), int(bool(is_qam))), "kg_fftext_set_run")

    def set_itime(self, ch, itime):
        check(self.lib.kg_fftext_set_itime(self.h, int(ch), float(itime)), "kg_fftext_set_itime")

    def clear(self, ch):
        check(self.lib.kg_fftext_clear(self.h, int(ch)), "kg_fftext_clear")

    def restart(self, ch):
        check(self.lib.kg_fftext_restart(self.h, int(ch)), "kg_fftext_restart")

    def due(self, ch, now_ms):
        return bool(check(self.lib.kg_fftext_due(self.h, int(ch), int(now_ms) & 0xffffffff), "kg_fftext_due"))

    def _call(self, fn, name, chans, nblk, inst, spec, spec_stride, rows, row_stride, max_rows):
        chans, nblk, inst = (np.ascontiguousarray(a, np.int32) for a in (chans, nblk, inst))
        assert chans.size == nblk.size == inst.size
        m = np.zeros((4, max(int(max_rows), 1)), np.int32)
        n = check(fn(self.h, ptr(chans), int(chans.size), ptr(nblk), ptr(inst), ptr(spec), int(spec_stride), ptr(rows), int(row_stride), int(max_rows),
                     ptr(m[0]), ptr(m[1]), ptr(m[2]), ptr(m[3])), name)
        return m[:, :n].T.copy()

    def process_dev(self, chans, nblk, inst, d_spec, spec_stride, d_rows, row_stride, max_rows):
        """enqueue only -> int32 [rows, 4]: channel, list entry, block within the entry, bin of every row written"""
        return self._call(self.lib.kg_fftext_process_dev, "kg_fftext_process_dev", chans, nblk, inst, int(d_spec), spec_stride, int(d_rows), row_stride,
                          max_rows)

    def process(self, chans, spec, inst):
        """host arrays: spec complex64 [entries, nblk, 1024] -> (uint8 [rows, 1024], int32 [rows, 4]); synchronises"""
        spec = np.ascontiguousarray(spec, np.complex64)
        assert spec.ndim == 3 and spec.shape[2] == ROW
        nent, nb = spec.shape[:2]
        rows = np.zeros((max(nent * nb, 1), ROW), np.uint8)
        m = self._call(self.lib.kg_fftext_process, "kg_fftext_process", chans, [nb] * nent, inst, spec.view(np.float32), max(nb, 1) * ROW, rows, ROW,
                       rows.shape[0])
        return rows[:m.shape[0]].copy(), m

    def state(self, ch, sums=False):
        """-> (info record, ncma int32 [200], sums float32 [200, 1024] or None); with sums it synchronises"""
        info = np.zeros(1, info_dtype)
        ncma = np.zeros(MAX_BINS, np.int32)
        pwr = np.zeros((MAX_BINS, ROW), np.float32) if sums else None
        check(self.lib.kg_fftext_state(self.h, int(ch), ptr(info), ptr(pwr), ptr(ncma)), "kg_fftext_state")
        return info[0], ncma, pwr
