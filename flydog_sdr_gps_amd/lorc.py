"""The Loran-C extension over the C ABI (kg_lorc): a consumer of receive_iq_samps(PRE_AGC), CFastFIR's output of every sound block.

Reference                                                              here
  loran_c_msgs `SET ext_server_init`  loran_c.cpp:218-228                -> LoranC.init, ms_per_bin
               `SET gri%d=` (init_gri :198-208) / `SET offset%d=` / `SET gain%d=` / `SET avg_algo%d=` / `SET avg_param%d=`  :230-280
                                                                         -> LoranC.set_gri ... LoranC.set_avg_param
               `SET start` / `SET stop`  :282-302                        -> LoranC.start / LoranC.stop
  loran_c_data  :65-196                                                  -> LoranC.process; its schedule alone: LoranC.plan

The samples are what kg_fir_process_dev leaves in d_out.  A row is the payload of ext_send_msg_data (:119-120) under its cmd: byte 0
the Loran channel, then a byte per bucket.
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, load_library, ptr  # noqa: F401

CMA, EMA, IIR = 0, 1, 2                         # KG_LORC_*: AVG_CMA, AVG_EMA, AVG_IIR
SCOPE_DATA, SCOPE_RESET = 0, 1
MAX_GRI, MAX_BUCKET, MAX_NS = 9999, 1199, 512

row_dtype = np.dtype([("conn", "<i4"), ("blk", "<i4"), ("samp", "<i4"), ("ch", "<i4"), ("cmd", "<i4"), ("len", "<i4"), ("off", "<i8")])
chan_dtype = np.dtype([("gri", "<u4"), ("samp", "<u4"), ("nbucket", "<u4"), ("dsp_samps", "<u4"), ("avg_samps", "<u4"), ("navgs", "<u4"),
                       ("samp_per_GRI", "<f8"), ("gain", "<f4"), ("max", "<f4"), ("offset", "<i4"), ("avg_algo", "<i4"), ("avg_param_f", "<f8"),
                       ("avg_param_i", "<i4"), ("restart", "<i4")])
info_dtype = np.dtype([("inited", "<i4"), ("started", "<i4"), ("i_srate", "<u4"), ("redraw_legend", "<i4"), ("srate", "<f8"), ("ch", chan_dtype, (2,))])
assert row_dtype.itemsize == 32 and chan_dtype.itemsize == 64 and info_dtype.itemsize == 152


def ms_per_bin(srate, i_srate):
    """the number of the `EXT ms_per_bin=` line (:223-225)"""
    return float(load_library().kg_lorc_ms_per_bin(float(srate), int(i_srate)))


class LoranC:
    """nconn loran_c_t objects (loran_c.cpp:29-54) on the GPU (kg_lorc): two Loran channels each"""

    def __init__(self, ctx=None, nconn=1, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nconn = int(nconn)
        h = C.c_void_p()
        check(self.lib.kg_lorc_create(self.ctx.h, int(nconn), C.byref(h)), "kg_lorc_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None) and not getattr(self, "_borrowed", False):
                self.lib.kg_lorc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init(self, conn, srate=12000.0, i_srate=12000):
        check(self.lib.kg_lorc_init(self.h, int(conn), float(srate), int(i_srate)), "kg_lorc_init")

    def set_gri(self, conn, ch, gri):
        check(self.lib.kg_lorc_set_gri(self.h, int(conn), int(ch), int(gri)), "kg_lorc_set_gri")

    def set_offset(self, conn, ch, offset):
        check(self.lib.kg_lorc_set_offset(self.h, int(conn), int(ch), int(offset)), "kg_lorc_set_offset")

    def set_gain(self, conn, ch, gain):
        check(self.lib.kg_lorc_set_gain(self.h, int(conn), int(ch), int(gain)), "kg_lorc_set_gain")

    def set_avg_algo(self, conn, ch, avg_algo):
        check(self.lib.kg_lorc_set_avg_algo(self.h, int(conn), int(ch), int(avg_algo)), "kg_lorc_set_avg_algo")

    def set_avg_param(self, conn, ch, avg_param):
        check(self.lib.kg_lorc_set_avg_param(self.h, int(conn), int(ch), float(avg_param)), "kg_lorc_set_avg_param")

    def start(self, conn):
        check(self.lib.kg_lorc_start(self.h, int(conn)), "kg_lorc_start")

    def stop(self, conn):
        check(self.lib.kg_lorc_stop(self.h, int(conn)), "kg_lorc_stop")

    def process(self, conns, iq, rows=None, max_rows=None, nblk=None):
        """host arrays: iq complex64 [entries, blocks, ns] -> (row bytes uint8, row map of row_dtype); synchronises.  rows: the caller's
        byte array (default: one large enough, zeroed); max_rows: the map's size; nblk: blocks per entry (default: all)"""
        if getattr(self, "_borrowed", False):
            raise RuntimeError("a receiver bank's LoranC is fed by the bank's steps")
        iq = np.ascontiguousarray(iq, np.complex64)
        assert iq.ndim == 3 and iq.shape[2] >= 1
        nent, nb, ns = iq.shape
        conns = np.ascontiguousarray(conns, np.int32)
        nblk = np.full(nent, nb, np.int32) if nblk is None else np.ascontiguousarray(nblk, np.int32)
        assert conns.size == nent == nblk.size
        if max_rows is None:
            max_rows = 2 * nent * (nb * ns + 1)
        if rows is None:
            rows = np.zeros(min(max_rows, 2 * nent * (nb * ns // 64 + 2)) * 1200, np.uint8)
        m = np.zeros(max(int(max_rows), 1), row_dtype)
        n = C.c_int32(0)
        check(self.lib.kg_lorc_process(self.h, ptr(conns), int(nent), ptr(nblk), int(ns), ptr(iq.view(np.float32)), int(max(nb, 1) * ns), ptr(rows), int(rows.size),
                                       ptr(m), int(max_rows), C.byref(n)), "kg_lorc_process")
        return rows, m[:n.value].copy()

    def plan(self, conns, nblk, ns):
        """the schedule of process() on so many blocks of ns samples, walked on copies -> (runs, rows, row bytes); changes nothing"""
        conns, nblk = np.ascontiguousarray(conns, np.int32), np.ascontiguousarray(nblk, np.int32)
        assert conns.size == nblk.size
        runs, rows, nbytes = C.c_int32(0), C.c_int32(0), C.c_size_t(0)
        check(self.lib.kg_lorc_plan(self.h, ptr(conns), int(conns.size), ptr(nblk), int(ns), C.byref(runs), C.byref(rows), C.byref(nbytes)), "kg_lorc_plan")
        return runs.value, rows.value, nbytes.value

    def state(self, conn):
        """-> (info record of info_dtype, avg float32 [2, 1199]); synchronises"""
        info = np.zeros(1, info_dtype)
        avg = np.zeros((2, MAX_BUCKET), np.float32)
        check(self.lib.kg_lorc_state(self.h, int(conn), ptr(info), ptr(avg)), "kg_lorc_state")
        return info[0], avg
