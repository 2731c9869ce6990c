"""The IQ display extension over the C ABI (kg_iqd): a consumer of receive_iq_samps(PRE_AGC), CFastFIR's output of every sound block.

Reference                                                              here
  iq_display_msgs `SET ext_server_init`  iq_display.cpp:258-262          -> IqDisplay.init
                  `SET run=`             :264-273                        -> IqDisplay.set_run
  process_msg     gain / points / pll_mode / pll_bandwidth / draw / display_mode / clear  :126-158
                                                                         -> IqDisplay.set_gain ... IqDisplay.clear
  iq_display_data / display_data  :71-112, :246-250                      -> IqDisplay.process / process_dev

The samples are what kg_fir_process_dev leaves in d_out.  A row is the payload of ext_send_msg_data (:82 / :93) under its cmd; a sent
status record is what the text message of :108 carries.
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, ptr  # noqa: F401

POINTS, DENSITY = 0, 1                          # KG_IQD_*: IQ_POINTS, IQ_DENSITY
RING, MAX_NS = 16384, 512
HYPOTF, FMODF = 0, 1                            # KG_IQD_MATH_*

status_dtype = np.dtype([("cmaI", "<f4"), ("cmaQ", "<f4"), ("df", "<f8"), ("phase", "<f4"), ("reserved", "<i4")])
row_dtype = np.dtype([("ch", "<i4"), ("ent", "<i4"), ("blk", "<i4"), ("samp", "<i4"), ("cmd", "<i4"), ("len", "<i4"), ("off", "<i8")])
info_dtype = np.dtype([("inited", "<i4"), ("run", "<i4"), ("points", "<i4"), ("nsamp", "<i4"), ("exponent", "<i4"), ("msk_mode", "<i4"),
                       ("msk_baud", "<i4"), ("draw", "<i4"), ("display_mode", "<i4"), ("maN", "<i4"), ("maNsend", "<i4"), ("ring", "<i4", (2,)),
                       ("reserved", "<i4"), ("gain", "<f4"), ("fs", "<f4"), ("pll_bandwidth", "<f4"), ("cmaI", "<f4"), ("cmaQ", "<f4"), ("ama", "<f4"),
                       ("pll", "<f4", (3, 7))])
assert status_dtype.itemsize == 24 and row_dtype.itemsize == 32 and info_dtype.itemsize == 164


class IqDisplay:
    """nchan iq_display objects (iq_display.cpp:29-242) on the GPU (kg_iqd): 416 KiB of rings each"""

    def __init__(self, ctx=None, nchan=1, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nchan = int(nchan)
        h = C.c_void_p()
        check(self.lib.kg_iqd_create(self.ctx.h, int(nchan), C.byref(h)), "kg_iqd_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None) and not getattr(self, "_borrowed", False):
                self.lib.kg_iqd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init(self, ch):
        check(self.lib.kg_iqd_init(self.h, int(ch)), "kg_iqd_init")

    def set_run(self, ch, run, rate=12000.0):
        check(self.lib.kg_iqd_set_run(self.h, int(ch), int(run), float(rate)), "kg_iqd_set_run")

    def set_gain(self, ch, gain):
        check(self.lib.kg_iqd_set_gain(self.h, int(ch), int(gain)), "kg_iqd_set_gain")

    def set_points(self, ch, points):
        check(self.lib.kg_iqd_set_points(self.h, int(ch), int(points)), "kg_iqd_set_points")

    def set_pll_mode(self, ch, pll_mode, arg):
        check(self.lib.kg_iqd_set_pll_mode(self.h, int(ch), int(pll_mode), int(arg)), "kg_iqd_set_pll_mode")

    def set_pll_bandwidth(self, ch, bandwidth):
        check(self.lib.kg_iqd_set_pll_bandwidth(self.h, int(ch), float(bandwidth)), "kg_iqd_set_pll_bandwidth")

    def set_draw(self, ch, draw):
        check(self.lib.kg_iqd_set_draw(self.h, int(ch), int(draw)), "kg_iqd_set_draw")

    def set_display_mode(self, ch, display_mode):
        check(self.lib.kg_iqd_set_display_mode(self.h, int(ch), int(display_mode)), "kg_iqd_set_display_mode")

    def clear(self, ch):
        check(self.lib.kg_iqd_clear(self.h, int(ch)), "kg_iqd_clear")

    def _call(self, fn, name, chans, nblk, inst, ns, iq, iq_stride, rows, rows_cap, status, status_cap, max_rows):
        chans, nblk, inst = (np.ascontiguousarray(a, np.int32) for a in (chans, nblk, inst))
        assert chans.size == nblk.size == inst.size
        m = np.zeros(max(int(max_rows), 1), row_dtype)
        sent = np.zeros(max(int(nblk.sum()), 1), np.int32)
        n = check(fn(self.h, ptr(chans), int(chans.size), ptr(nblk), ptr(inst), int(ns), ptr(iq), int(iq_stride), ptr(rows), int(rows_cap), ptr(status),
                     int(status_cap), ptr(m), int(max_rows), ptr(sent)), name)
        return m[:n].copy(), sent[:int(nblk.sum())].copy()

    def process_dev(self, chans, nblk, inst, ns, d_iq, iq_stride, d_rows, rows_cap, d_status, status_cap, max_rows):
        """enqueue only -> (row map [rows] of row_dtype, status map int32 [blocks of the call])"""
        return self._call(self.lib.kg_iqd_process_dev, "kg_iqd_process_dev", chans, nblk, inst, ns, int(d_iq), iq_stride, int(d_rows), rows_cap,
                          int(d_status), status_cap, max_rows)

    def process(self, chans, iq, inst):
        """host arrays: iq complex64 [entries, nblk, ns] -> (row bytes uint8, row map, status records [blocks], status map); synchronises"""
        iq = np.ascontiguousarray(iq, np.complex64)
        assert iq.ndim == 3 and 1 <= iq.shape[2] <= MAX_NS
        nent, nb, ns = iq.shape
        cap = (ns * nb + RING) * 4 * nent
        rows = np.zeros(cap, np.uint8)
        status = np.zeros(max(nent * nb, 1), status_dtype)
        m, sent = self._call(self.lib.kg_iqd_process, "kg_iqd_process", chans, [nb] * nent, inst, ns, iq.view(np.float32), max(nb, 1) * ns, rows, cap,
                             status, status.size, nent * nb * ns + 1)
        used = int(m["off"][-1] + m["len"][-1]) if m.size else 0
        return rows[:used].copy(), m, status[:nent * nb].copy(), sent

    def state(self, ch, arrays=False):
        """-> (info record, iq complex64 [2, 16384], plot uint8 [2, 16384, 2, 2], map uint8 [16384, 2]) (the arrays None without
        `arrays`); synchronises"""
        info = np.zeros(1, info_dtype)
        iq = np.zeros((2, RING), np.complex64) if arrays else None
        plot = np.zeros((2, RING, 2, 2), np.uint8) if arrays else None
        mp = np.zeros((RING, 2), np.uint8) if arrays else None
        check(self.lib.kg_iqd_state(self.h, int(ch), ptr(info), ptr(iq), ptr(plot), ptr(mp)), "kg_iqd_state")
        return info[0], iq, plot, mp


def math_dev(ctx, fn, d_a, d_b, n, d_out):
    """d_out[i] = hypotf / fmodf (HYPOTF / FMODF) of d_a[i], d_b[i] as kg_iqd's device code computes them; enqueue only"""
    check(ctx.lib.kg_iqd_math_dev(ctx.h, int(fn), C.c_void_p(int(d_a)), C.c_void_p(int(d_b)), int(n), C.c_void_p(int(d_out))), "kg_iqd_math_dev")
