"""The WSPR extension over the C ABI (kg_wspr), stage 1: a consumer of receive_iq_samps, CFastFIR's output of every sound block.

Reference                                                              here
  wspr_msgs `SET ext_server_init`  wspr_main.cpp:834-838                 -> Wspr.init
            `SET capture=%d`  :880-900 (wspr_close / wspr_reset :790-824) -> Wspr.set_capture
  wspr_type / more_candidates  wspr.h:254-257                            -> Wspr.set_type / Wspr.set_more_candidates
  wspr_data  :595-788, WSPR_FFT  :117-240, pass 0 of wspr_decode  wspr.cpp:555-714
                                                                         -> Wspr.push; its schedule alone: Wspr.plan
  wspr_status  :96-114, wspr_send_peaks  :285-301                        -> Wspr.messages
Stage 2 (include/kiwigpu_wspr_dec.h):
  mettab of wspr_init  wspr.cpp:431-441                                  -> Wspr.set_metric_table (the table is the caller's)
  one pass of wspr_decode's candidate loop  wspr.cpp:733-883, fano.cpp   -> Wspr.decode; the reference's progression of passes: Wspr.decode_passes
  i_data / q_data and a candidate list handed in                         -> Wspr.load_iq;  fano alone: Wspr.fano

The samples are what kg_fir_process_dev leaves in d_out.  A row is the payload of ext_send_msg_data (:238): byte 0 the sync flag of
group 0, then a byte per bin.  Time is an input: every block carries the minute and second of its callback.
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, load_library, ptr  # noqa: F401

IDLE, SYNC, RUNNING, DECODING = 1, 2, 3, 4      # KG_WSPR_*: wspr_main.cpp:49-53
EV_STATUS, EV_PEAKS, EV_DECODES = 0, 1, 2
NBINS, NFFT, NT, TPOINTS, MAX_NPK, ROW_STRIDE = 411, 512, 348, 45000, 12, 416

row_dtype = np.dtype([("conn", "<i4"), ("blk", "<i4"), ("samp", "<i4"), ("group", "<i4"), ("half", "<i4"), ("tsync", "<i4"), ("off", "<i8")])
ev_dtype = np.dtype([("conn", "<i4"), ("blk", "<i4"), ("samp", "<i4"), ("kind", "<i4"), ("a", "<i4"), ("b", "<i4")])
pk_dtype = np.dtype([("bin0", "<i4"), ("freq0", "<f4"), ("snr0", "<f4"), ("pad", "<i4")])
cand_dtype = np.dtype([("freq0", "<f4"), ("shift0", "<i4"), ("drift0", "<f4"), ("sync0", "<f4"), ("freq_idx", "<i4"), ("bin0", "<i4")])
cycle_dtype = np.dtype([("due", "<i4"), ("half", "<i4"), ("npk", "<i4"), ("pad", "<i4"), ("pk", pk_dtype, (MAX_NPK,)), ("cand", cand_dtype, (MAX_NPK,))])
info_dtype = np.dtype([(n, "<i4") for n in ("inited", "capture", "reset", "tsync", "ping_pong", "fft_ping_pong", "decode_ping_pong", "decim", "didx", "group",
                                            "status", "status_resume", "last_sec", "abort_decode", "wspr_type", "more_candidates", "int_decimate", "cycles")]
                      + [("snd_rate", "<f8")])
SKIPPED, MINSYNC1, NO_CHANGE, TIME_UP, DECODED, QUICK_MISS = 0, 1, 2, 3, 4, 5          # KG_WSPR_*: kg_wspr_dec.result
PASSES = ((200, 2), (1000, 1), (5000, 1), (10000, 1))                                 # maxcycles, iifac of the reference's passes (wspr.cpp:505-508, :536-553)
dec_dtype = np.dtype([("result", "<i4"), ("ignore", "<i4"), ("f1", "<f4"), ("shift1", "<i4"), ("drift1", "<f4"), ("sync1", "<f4"),
                      ("tr_f", "<f4", (6,)), ("tr_shift", "<i4", (6,)), ("tr_sync", "<f4", (6,)),
                      ("idt", "<i4"), ("ii", "<i4"), ("jig_shift", "<i4"), ("gates", "<i4"), ("rms", "<f4"),
                      ("metric", "<u4"), ("cycles", "<u4"), ("maxnp", "<u4"), ("decdata", "u1", (11,)), ("symbols", "u1", (162,)), ("pad", "u1", (3,))])
assert dec_dtype.itemsize == 304
assert (row_dtype.itemsize, ev_dtype.itemsize, pk_dtype.itemsize, cand_dtype.itemsize, cycle_dtype.itemsize, info_dtype.itemsize) == (32, 24, 16, 24, 496, 80)


def messages(evs, cycles, conns=None, now=(0, 0)):
    """the text of the events of a push, as the reference sends it: `EXT WSPR_STATUS=%d WSPR_TIME_MSEC=%d=%d` (:106; the clock is the
    caller's: now = (sec, msec)) and `EXT WSPR_PEAKS=` with "%d:%s:" per peak, the bin and the "%d" of roundf(snr0) (:296-299,
    wspr.cpp:621).  cycles: what push() returned, a record per LIST ENTRY, with conns the list that was pushed (default: the identity);
    or a dict {connection: record}"""
    if not isinstance(cycles, dict):
        conns = range(len(cycles)) if conns is None else conns
        cycles = {int(c): cycles[i] for i, c in enumerate(conns)}
    out = []
    for e in evs:
        if e["kind"] == EV_STATUS:
            out.append((int(e["conn"]), "EXT WSPR_STATUS=%d WSPR_TIME_MSEC=%d=%d" % (e["a"], now[0], now[1])))
        elif e["kind"] == EV_PEAKS:
            cy = cycles[int(e["conn"])]
            s = "".join("%d:%d:" % (p["bin0"], int(np.float32(np.copysign(np.floor(np.abs(p["snr0"]) + np.float32(0.5)), p["snr0"])))) for p in cy["pk"][:cy["npk"]])
            out.append((int(e["conn"]), "EXT WSPR_PEAKS=" + s))
    return out


class Wspr:
    """nconn wspr_t / wspr_buf_t pairs (wspr.h:223-312) on the GPU (kg_wspr)"""

    def __init__(self, ctx=None, nconn=1, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nconn = int(nconn)
        h = C.c_void_p()
        check(self.lib.kg_wspr_create(self.ctx.h, int(nconn), C.byref(h)), "kg_wspr_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None) and not getattr(self, "_borrowed", False):
                self.lib.kg_wspr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init(self, conn, snd_rate=12000.0):
        check(self.lib.kg_wspr_init(self.h, int(conn), float(snd_rate)), "kg_wspr_init")

    def set_capture(self, conn, capture):
        check(self.lib.kg_wspr_set_capture(self.h, int(conn), int(capture)), "kg_wspr_set_capture")

    def set_type(self, conn, wspr_type):
        check(self.lib.kg_wspr_set_type(self.h, int(conn), int(wspr_type)), "kg_wspr_set_type")

    def set_more_candidates(self, conn, on):
        check(self.lib.kg_wspr_set_more_candidates(self.h, int(conn), int(on)), "kg_wspr_set_more_candidates")

    def push(self, conns, iq, minute, second, nblk=None, rows=None, max_rows=None, max_events=None):
        """host arrays: iq complex64 [entries, blocks, ns], minute / second int [entries, blocks] -> (row bytes uint8, row map of
        row_dtype, events of ev_dtype, cycles of cycle_dtype per entry, counts int32 [entries, 4]); synchronises"""
        if getattr(self, "_borrowed", False):
            raise RuntimeError("a receiver bank's Wspr is fed by the bank's steps")
        iq = np.ascontiguousarray(iq, np.complex64)
        assert iq.ndim == 3 and iq.shape[2] >= 1
        nent, nb, ns = iq.shape
        conns = np.ascontiguousarray(conns, np.int32)
        nblk = np.full(nent, nb, np.int32) if nblk is None else np.ascontiguousarray(nblk, np.int32)
        minute = np.ascontiguousarray(np.broadcast_to(np.asarray(minute, np.int32), (nent, nb)))
        second = np.ascontiguousarray(np.broadcast_to(np.asarray(second, np.int32), (nent, nb)))
        assert conns.size == nent == nblk.size
        if max_rows is None:
            max_rows = nent * (nb * ns // NFFT + 2)
        if max_events is None:
            max_events = nent * (8 + 4 * nb)
        if rows is None:
            rows = np.zeros(max(max_rows, 1) * ROW_STRIDE, np.uint8)
        m = np.zeros(max(int(max_rows), 1), row_dtype)
        ev = np.zeros(max(int(max_events), 1), ev_dtype)
        cyc = np.zeros(nent, cycle_dtype)
        counts = np.zeros((nent, 4), np.int32)
        n, ne = C.c_int32(0), C.c_int32(0)
        check(self.lib.kg_wspr_push(self.h, ptr(conns), int(nent), ptr(nblk), int(ns), ptr(iq.view(np.float32)), int(max(nb, 1) * ns), ptr(minute), ptr(second),
                                    int(max(nb, 1)), ptr(rows), int(rows.size), ptr(m), int(max_rows), C.byref(n), ptr(ev), int(max_events), C.byref(ne), ptr(cyc),
                                    ptr(counts)), "kg_wspr_push")
        return rows, m[:n.value].copy(), ev[:ne.value].copy(), cyc, counts

    def plan(self, conns, nblk, ns, minute, second):
        """the schedule of push() walked on copies -> (ops, rows, events, cycle ends); changes nothing"""
        conns, nblk = np.ascontiguousarray(conns, np.int32), np.ascontiguousarray(nblk, np.int32)
        nb = max(int(nblk.max()) if nblk.size else 0, 1)
        minute = np.ascontiguousarray(np.broadcast_to(np.asarray(minute, np.int32), (conns.size, nb)))
        second = np.ascontiguousarray(np.broadcast_to(np.asarray(second, np.int32), (conns.size, nb)))
        o = [C.c_int32(0) for _ in range(4)]
        check(self.lib.kg_wspr_plan(self.h, ptr(conns), int(conns.size), ptr(nblk), int(ns), ptr(minute), ptr(second), nb, *[C.byref(v) for v in o]), "kg_wspr_plan")
        return tuple(v.value for v in o)

    def state(self, conn, planes=False, samples=False):
        """-> (info record of info_dtype, pwr_sampavg float32 [2, 512], pwr_samp [2, 512, 348] or None, i / q data [2 (i, q), 2, 45000] or None)"""
        info = np.zeros(1, info_dtype)
        avg = np.zeros((2, NFFT), np.float32)
        pl = np.zeros((2, NFFT, NT), np.float32) if planes else None
        iq = np.zeros((2, 2, TPOINTS), np.float32) if samples else None
        check(self.lib.kg_wspr_state(self.h, int(conn), ptr(info), ptr(avg), ptr(pl) if planes else None, ptr(iq) if samples else None), "kg_wspr_state")
        return info[0], avg, pl, iq

    def load(self, conn, half, pwr_samp, pwr_sampavg):
        """pwr_samp [512, 348] and pwr_sampavg [512] into a half, then the cycle end -> cycle record; synchronises"""
        ps = np.ascontiguousarray(pwr_samp, np.float32)
        pa = np.ascontiguousarray(pwr_sampavg, np.float32)
        assert ps.shape == (NFFT, NT) and pa.shape == (NFFT,)
        cyc = np.zeros(1, cycle_dtype)
        check(self.lib.kg_wspr_load(self.h, int(conn), int(half), ptr(ps), ptr(pa), ptr(cyc)), "kg_wspr_load")
        return cyc[0]

    # ---- stage 2
    def set_metric_table(self, mettab):
        """int32 [2, 256]: mettab of wspr_init (wspr.cpp:431-441), for the whole object"""
        mt = np.ascontiguousarray(mettab, np.int32)
        assert mt.shape == (2, 256)
        check(self.lib.kg_wspr_set_metric_table(self.h, ptr(mt)), "kg_wspr_set_metric_table")

    def load_iq(self, conn, half, iq, cands):
        """iq complex64 [45000] (or i_data, q_data as a pair of float32 arrays) into a half, and the candidates -- records of cand_dtype,
        or rows (freq0, shift0, drift0, sync0) -- as the connection's held list in SNR order, ignore cleared; synchronises"""
        if isinstance(iq, tuple):
            i_data, q_data = (np.ascontiguousarray(v, np.float32) for v in iq)
        else:
            iq = np.asarray(iq, np.complex64)
            i_data, q_data = np.ascontiguousarray(iq.real, np.float32), np.ascontiguousarray(iq.imag, np.float32)
        assert i_data.shape == (TPOINTS,) and q_data.shape == (TPOINTS,)
        if not (isinstance(cands, np.ndarray) and cands.dtype == cand_dtype):
            rows = list(cands)
            cands = np.zeros(len(rows), cand_dtype)
            for k, r in enumerate(rows):
                cands[k] = (r[0], r[1], r[2], r[3], k, 0)
        cands = np.ascontiguousarray(cands)
        check(self.lib.kg_wspr_load_iq(self.h, int(conn), int(half), ptr(i_data), ptr(q_data), ptr(cands) if cands.size else None, int(cands.size)), "kg_wspr_load_iq")

    def decode(self, conns, maxcycles=200, iifac=2, quickmode=False):
        """one pass of wspr.cpp:733-883 on the held candidates of every listed connection -> (records of dec_dtype [entries, 12],
        candidates per entry int32 [entries]); synchronises"""
        conns = np.ascontiguousarray(conns, np.int32)
        out = np.zeros((conns.size, MAX_NPK), dec_dtype)
        ncand = np.zeros(conns.size, np.int32)
        check(self.lib.kg_wspr_decode(self.h, ptr(conns), int(conns.size), int(maxcycles), int(iifac), int(bool(quickmode)), ptr(out), ptr(ncand)), "kg_wspr_decode")
        return out, ncand

    def decode_passes(self, conn, passes=4):
        """the reference's progression 200 / 2, 1000 / 1, 5000 / 1, 10000 / 1 on one connection until no candidate is left (every one
        ignored) or `passes` is spent -> the list of (records [ncand], maxcycles, iifac) per pass run"""
        done = []
        for maxcycles, iifac in PASSES[:int(passes)]:
            out, ncand = self.decode([conn], maxcycles, iifac)
            recs = out[0][:ncand[0]]
            if done and (recs["result"] == SKIPPED).all():
                break                                   # candidates == 0 (wspr.cpp:999): nothing left to do
            done.append((recs.copy(), maxcycles, iifac))
            if recs.size == 0:
                break
        return done

    def set_decode(self, conn, on):
        """on: a cycle end inside push() also runs pass 0 (200, 2) behind it; its records: decodes()"""
        check(self.lib.kg_wspr_set_decode(self.h, int(conn), int(on)), "kg_wspr_set_decode")

    def decodes(self, conn):
        """-> the records (dec_dtype, the connection's candidates) of the last pass 0 that a push ran for the connection; synchronises"""
        out, n = np.zeros(MAX_NPK, dec_dtype), C.c_int32(0)
        check(self.lib.kg_wspr_decodes(self.h, int(conn), ptr(out), C.byref(n)), "kg_wspr_decodes")
        return out[:n.value].copy()

    def fano(self, symbols, maxcycles=200):
        """fano alone on DEINTERLEAVED symbol sets uint8 [n, 162] -> (ok int32 [n], metric, cycles, maxnp uint32 [n], data uint8 [n, 10])"""
        sy = np.ascontiguousarray(symbols, np.uint8).reshape(-1, 162)
        n = sy.shape[0]
        ok = np.zeros(n, np.int32)
        metric, cycles, maxnp = (np.zeros(n, np.uint32) for _ in range(3))
        data = np.zeros((n, 10), np.uint8)
        check(self.lib.kg_wspr_fano(self.h, ptr(sy), int(n), int(maxcycles), ptr(ok), ptr(metric), ptr(cycles), ptr(maxnp), ptr(data)), "kg_wspr_fano")
        return ok, metric, cycles, maxnp, data

    messages = staticmethod(messages)
