"""The FT8 / FT4 extension over the C ABI (kg_ft8; include/kiwigpu_ft8.h), stage 1: a consumer of the real-samples tap.

Reference (extensions/FT8/ft8_lib)                                     here
  decode_ft8_init / _protocol  decode_ft8.c:561-617                      -> Ft8.init
  ft8_conf.SNR_adj  :303                                                 -> Ft8.set_snr_adj
  decode_ft8_samples  :503-559, monitor_process  common/monitor.c:141-203,
  ftx_find_candidates  ft8/decode.c:192-254, the likelihoods  :256-328   -> Ft8.push; its schedule alone: Ft8.plan
  a waterfall handed in                                                  -> Ft8.load_wf

The samples are int16, as real_samples_s2 holds them.  Time is an input: every callback carries the seconds clock_gettime would have
given.  A slot record ends at log174; bp_decode, the CRC and the message are stage 2's.
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, load_library, ptr  # noqa: F401

FT8, FT4 = 0, 1                                  # KG_FT8_PROTO_*
EV_SLOT_START, EV_DECODE = 0, 1
MAX_CAND, MIN_SCORE, LDPC_N, MAX_NS, MAX_NFFT, MAX_WF = 140, 10, 174, 2048, 3840, 178932

ev_dtype = np.dtype([("conn", "<i4"), ("cb", "<i4"), ("kind", "<i4"), ("a", "<i4"), ("b", "<i4"), ("pad", "<i4"), ("t", "<i8")])
cand_dtype = np.dtype([("score", "<i2"), ("time_offset", "<i2"), ("freq_offset", "<i2"), ("time_sub", "u1"), ("freq_sub", "u1"),
                       ("freq_hz", "<f4"), ("time_sec", "<f4"), ("snr", "<f4")])
slot_dtype = np.dtype([("conn", "<i4"), ("due", "<i4"), ("ncand", "<i4"), ("num_blocks", "<i4"), ("protocol", "<i4"), ("slot", "<i4"), ("max_mag", "<f4"),
                       ("pad", "<i4"), ("cand", cand_dtype, (MAX_CAND,)), ("log174", "<f4", (MAX_CAND, LDPC_N))])
info_dtype = np.dtype([(n, "<i4") for n in ("inited", "protocol", "tsync", "in_pos", "frame_pos", "num_blocks", "parity", "last_blocks", "block_size", "nfft",
                                            "num_bins", "min_bin", "max_blocks", "num_samples", "slot_blocks", "block_stride")]
                      + [("slot", "<u4"), ("decode_time", "<u4"), ("slot_start", "<i8"), ("max_mag", "<f4"), ("last_max_mag", "<f4")])
assert (ev_dtype.itemsize, cand_dtype.itemsize, slot_dtype.itemsize, info_dtype.itemsize) == (32, 20, 32 + 20 * 140 + 4 * 140 * 174, 88)


class Ft8:
    """nconn decode_ft8_t with their monitors (decode_ft8.c:45-69, common/monitor.h) on the GPU (kg_ft8)"""

    def __init__(self, ctx=None, nconn=1, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nconn = int(nconn)
        h = C.c_void_p()
        check(self.lib.kg_ft8_create(self.ctx.h, int(nconn), C.byref(h)), "kg_ft8_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None) and not getattr(self, "_borrowed", False):
                self.lib.kg_ft8_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_snr_adj(self, snr_adj):
        check(self.lib.kg_ft8_set_snr_adj(self.h, float(snr_adj)), "kg_ft8_set_snr_adj")

    def init(self, conn, protocol=FT8, snd_rate=12000.0):
        check(self.lib.kg_ft8_init(self.h, int(conn), int(protocol), float(snd_rate)), "kg_ft8_init")

    def push(self, conns, samples, times, ncb=None, max_events=None, max_slots=None):
        """host arrays: samples int16 [entries, callbacks, ns], times float64 [entries, callbacks] -> (events of ev_dtype, the ended
        slots of slot_dtype in list order); synchronises"""
        if getattr(self, "_borrowed", False):
            raise RuntimeError("a receiver bank's Ft8 is fed by the bank's steps")
        samples = np.ascontiguousarray(samples, np.int16)
        assert samples.ndim == 3 and samples.shape[2] >= 1
        nent, nb, ns = samples.shape
        conns = np.ascontiguousarray(conns, np.int32)
        ncb = np.full(nent, nb, np.int32) if ncb is None else np.ascontiguousarray(ncb, np.int32)
        times = np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.float64), (nent, nb)))
        assert conns.size == nent == ncb.size
        max_events = nent * (2 + 2 * nb) if max_events is None else int(max_events)
        max_slots = nent if max_slots is None else int(max_slots)
        ev = np.zeros(max(max_events, 1), ev_dtype)
        slots = np.zeros(max(max_slots, 1), slot_dtype)
        ne, nsl = C.c_int32(0), C.c_int32(0)
        check(self.lib.kg_ft8_push(self.h, ptr(conns), int(nent), ptr(ncb), int(ns), ptr(samples), int(max(nb, 1) * ns), ptr(times), int(max(nb, 1)), ptr(ev),
                                   int(max_events), C.byref(ne), ptr(slots), int(max_slots), C.byref(nsl)), "kg_ft8_push")
        return ev[:ne.value].copy(), slots[:nsl.value].copy()

    def plan(self, conns, ncb, ns, times):
        """the schedule of push() walked on copies -> (blocks, events, slot ends); changes nothing"""
        conns = np.ascontiguousarray(conns, np.int32)
        ncb = np.ascontiguousarray(ncb, np.int32)
        nb = int(ncb.max()) if ncb.size else 0
        times = np.ascontiguousarray(np.broadcast_to(np.asarray(times, np.float64), (conns.size, max(nb, 1))))
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        check(self.lib.kg_ft8_plan(self.h, ptr(conns), int(conns.size), ptr(ncb), int(ns), ptr(times), int(max(nb, 1)), C.byref(a), C.byref(b), C.byref(c)), "kg_ft8_plan")
        return a.value, b.value, c.value

    def state(self, conn, previous=False):
        """-> (info of info_dtype, last_frame float32 [nfft], waterfall bytes [blocks, 2, 2, num_bins] of the slot under way, or of the
        slot that ended last)"""
        info = np.zeros(1, info_dtype)
        lf = np.zeros(MAX_NFFT, np.float32)
        mag = np.zeros(MAX_WF, np.uint8)
        check(self.lib.kg_ft8_state(self.h, int(conn), ptr(info), ptr(lf), ptr(mag), int(bool(previous))), "kg_ft8_state")
        i = info[0]
        nb = int(i["last_blocks"] if previous else i["num_blocks"])
        nbins = int(i["num_bins"])
        return i, lf[:int(i["nfft"])].copy(), mag[:nb * 4 * nbins].reshape(nb, 2, 2, nbins).copy() if nbins else mag[:0]

    def load_wf(self, conn, protocol, mag, num_candidates=MAX_CAND, min_score=MIN_SCORE):
        """mag uint8 [num_blocks, 2, 2, num_bins] -> the slot record of slot_dtype"""
        mag = np.ascontiguousarray(mag, np.uint8)
        assert mag.ndim == 4 and mag.shape[1:3] == (2, 2) and mag.shape[3] == (145 if protocol == FT4 else 481)
        slot = np.zeros(1, slot_dtype)
        check(self.lib.kg_ft8_load_wf(self.h, int(conn), int(protocol), int(mag.shape[0]), ptr(mag), int(num_candidates), int(min_score), ptr(slot)), "kg_ft8_load_wf")
        return slot[0]
