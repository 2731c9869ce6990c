"""The FAX extension over the C ABI (kg_fax): HF weather fax from the 16-bit mono audio a sound block ends as (receive_real_samps).

Reference                                                              here
  fax_msgs `SET fax_start lpm= phasing= autostop= debug=`  fax.cpp:128-156, FaxDecoder::Configure FaxDecoder.cpp:467-515
                                                                         -> FaxDecoder.start (every parameter of Configure)
           `SET fax_shift=`  fax.cpp:159-165                             -> FaxDecoder.set_shift
           `SET fax_stop`    fax.cpp:167-171                             -> FaxDecoder.stop
  fax_task -> ProcessSamples  fax.cpp:85-88, FaxDecoder.cpp:410-447      -> FaxDecoder.push (host arrays); on device memory: RxBank.fax_*

The schedule depends on the samples, so the decoder lives on the device and a push returns what the device counted: per listed
connection the completed lines (rec_dtype) and the rows -- FAX_MSG_DRAW (254), then imagewidth bytes, the payload of
ext_send_msg_data (FaxDecoder.cpp:404).
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, load_library, ptr  # noqa: F401

IMAGE, START, STOP = 0, 1, 2                    # KG_FAX_*: FaxDecoder.h:102
SPS_CHANGED, AUTOSTOPPED_0, AUTOSTOPPED_1, PHASED, ROW_SENT, PHASING_REJECTED, MEDIAN = 1, 2, 4, 8, 16, 32, 64
MAX_SPL, BLK, MSG_DRAW = 24576, 512, 254
NARROW, MIDDLE, WIDE = 0, 1, 2                  # firfilter::Bandwidth, FaxDecoder.h:42

rec_dtype = np.dtype([(n, "<i4") for n in ("blk", "off", "type", "typecount", "imageline", "phasingLinesLeft", "skip", "phasing_pos", "flags", "phasingSkipData",
                                           "ten_pct", "ninety_pct")])
info_dtype = np.dtype([(n, "<f8") for n in ("nom", "frac", "frac_prev", "ratio", "fi", "lineIncrFrac", "lineIncrAcc", "lineBlend", "carrier", "deviation")]
                      + [(n, "<i4") for n in ("lpm", "imagewidth", "bandwidth", "include_headers", "use_phasing", "autostop", "autostopped", "debug",
                                              "skip_header_detection", "spl", "skip", "samp_idx", "lasttype", "typecount", "imageline", "phasingLinesLeft",
                                              "phasingSkipData", "have_phasing", "fir_current", "started")]
                      + [("Iprev", "<f4"), ("Qprev", "<f4"), ("fir", "<f4", (2, 17)), ("phasingPos", "<i4", (40,)), ("shift", "<f4"), ("pad", "<i4")])
assert rec_dtype.itemsize == 48 and info_dtype.itemsize == 472


class FaxDecoder:
    """nconn FaxDecoder objects (FaxDecoder.cpp:51) on the GPU (kg_fax)"""

    def __init__(self, ctx=None, nconn=1, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nconn = int(nconn)
        h = C.c_void_p()
        check(self.lib.kg_fax_create(self.ctx.h, int(nconn), C.byref(h)), "kg_fax_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None) and not getattr(self, "_borrowed", False):
                self.lib.kg_fax_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def start(self, conn, lpm=120, imagewidth=1024, carrier=1900, deviation=400, bandwidth=MIDDLE, include_headers=True, phasing=True, autostop=True, debug=0,
              nom_rate=12000.0, srate=None):
        """the defaults are what fax.cpp:131-145 passes"""
        check(self.lib.kg_fax_start(self.h, int(conn), int(lpm), int(imagewidth), int(carrier), int(deviation), int(bandwidth), int(bool(include_headers)),
                                    int(bool(phasing)), int(bool(autostop)), int(debug), float(nom_rate), float(nom_rate if srate is None else srate)), "kg_fax_start")

    def set_shift(self, conn, shift):
        check(self.lib.kg_fax_set_shift(self.h, int(conn), float(shift)), "kg_fax_set_shift")

    def stop(self, conn):
        check(self.lib.kg_fax_stop(self.h, int(conn)), "kg_fax_stop")

    def max_lines(self, conns, nblk):
        """-> (the least max_lines of such a push, the widest imagewidth among its started connections)"""
        conns, nblk = np.ascontiguousarray(conns, np.int32), np.ascontiguousarray(nblk, np.int32)
        assert conns.size == nblk.size
        ml, mw = C.c_int32(0), C.c_int32(0)
        check(self.lib.kg_fax_max_lines(self.h, ptr(conns), int(conns.size), ptr(nblk), C.byref(ml), C.byref(mw)), "kg_fax_max_lines")
        return ml.value, mw.value

    def _shape(self, conns, s16, srate, nblk):
        s16 = np.ascontiguousarray(s16, np.int16)
        assert s16.ndim == 3 and s16.shape[2] == BLK
        nent, nb, _ = s16.shape
        conns = np.ascontiguousarray(conns, np.int32)
        srate = np.ascontiguousarray(srate, np.float64)
        nblk = np.full(nent, nb, np.int32) if nblk is None else np.ascontiguousarray(nblk, np.int32)
        assert conns.size == nent == nblk.size == srate.size
        ml, mw = self.max_lines(conns, nblk)
        return conns, s16, srate, nblk, nent, nb, max(ml, 1), (mw + 1 + 15) & ~15

    @staticmethod
    def _split(nent, counts, recs, rows):
        counts = counts.reshape(nent, 4)
        assert not counts[:, 2].any(), "a capacity was exceeded"
        return [recs[i, :counts[i, 1]].copy() for i in range(nent)], [rows[i, :counts[i, 0]].copy() for i in range(nent)]

    def push(self, conns, s16, srate, nblk=None):
        """host arrays: s16 int16 [entries, blocks, 512], srate float64 [entries] -> (per entry the records of rec_dtype, per entry the
        rows uint8 [rows, row_stride]: byte 0 is 254, then imagewidth bytes); synchronises"""
        if getattr(self, "_borrowed", False):
            raise RuntimeError("a receiver bank's FaxDecoder is fed by the bank's steps")
        conns, s16, srate, nblk, nent, nb, ml, rs = self._shape(conns, s16, srate, nblk)
        rows = np.zeros((nent, ml, rs), np.uint8)
        recs = np.zeros((nent, ml), rec_dtype)
        counts = np.zeros(4 * nent, np.int32)
        check(self.lib.kg_fax_push(self.h, ptr(conns), int(nent), ptr(nblk), ptr(s16), int(max(nb, 1) * BLK), ptr(srate), ptr(rows), int(rs), ptr(recs), int(ml),
                                   ptr(counts)), "kg_fax_push")
        return self._split(nent, counts, recs, rows)

    def state(self, conn):
        """-> (info record of info_dtype, m_samples int16, m_demod_data, the previous image line, m_outImage uint8; MAX_SPL entries each);
        synchronises"""
        info = np.zeros(1, info_dtype)
        samples = np.zeros(MAX_SPL, np.int16)
        demod, prev, out = (np.zeros(MAX_SPL, np.uint8) for _ in range(3))
        check(self.lib.kg_fax_state(self.h, int(conn), ptr(info), ptr(samples), ptr(demod), ptr(prev), ptr(out)), "kg_fax_state")
        return info[0], samples, demod, prev, out
