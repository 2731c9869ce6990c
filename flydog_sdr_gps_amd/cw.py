"""The CW decoder extension over the C ABI (kg_cw): Morse code from the 16-bit mono audio a sound block ends as.

Reference                                                              here
  cw_decoder_msgs `SET cw_start=` / `SET cw_train=`  cw_decoder.cpp:135-167, CwDecode_Init uhsdr_cw_decoder.cpp:345-392
                                                                         -> CwDecoder.start
                  `SET cw_wpm=`     cw_decoder.cpp:186-190, CwDecode_wpm :628-633           -> CwDecoder.set_wpm
                  `SET cw_pboff=`   cw_decoder.cpp:179-183, CwDecode_pboff :394-402         -> CwDecoder.set_pboff
                  `SET cw_wsc=`     cw_decoder.cpp:193-197                                  -> CwDecoder.set_wsc
                  `SET cw_auto_thresh=` / `SET cw_threshold=`  cw_decoder.cpp:200-211       -> CwDecoder.set_auto_threshold / set_threshold
                  `SET cw_stop`     cw_decoder.cpp:155-160                                  -> CwDecoder.stop
  cw_task -> CwDecode_RxProcessor  cw_decoder.cpp:101, uhsdr_cw_decoder.cpp:609-625         -> CwDecoder.push (host arrays)

The schedule depends on the samples, so the decoder lives on the device and a push returns what the device counted: per listed
connection the events (ev_dtype) -- the messages of ext_send_msg / ext_send_msg_encoded, which messages() turns into the client's text
lines.  Time is an input: a push carries what timer_sec() answers during it.
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, load_library, ptr  # noqa: F401

CHARS, WPM, TRAIN, PLOT = 0, 1, 2, 3            # KG_CW_*
BLK, GBLK, EVENTS_PER_GBLK = 512, 88, 7
PROSIGNS = ("<aa>", "<ar>", "<as>", "<bk>", "<bt>", "<cl>", "<ct>", "<hh>", "<kn>", "<nj>", "<sk>", "<sn>")      # cw_code[0..11], :190-201

ev_dtype = np.dtype([(n, "<i4") for n in ("blk", "gblk", "kind", "a", "b", "c")])
_scalars = ([("process_samples", "<i4"), ("wpm_update", "<u4"), ("wsc", "<i4"), ("err_cnt", "<i4"), ("err_timeout", "<i4"), ("sampling_freq", "<f4"), ("speed", "<i4"),
             ("isAutoThreshold", "<i4"), ("weight_linear", "<u4"), ("threshold_linear", "<u4"), ("blocksize", "<i4"),
             ("g_a", "<i4"), ("g_b", "<f4"), ("g_sin", "<f4"), ("g_cos", "<f4"), ("g_r", "<f4"),
             ("sig_lastrx", "<i4"), ("sig_incount", "<i4"), ("sig_outcount", "<i4"), ("sig_timer", "<i4"),
             ("data_len", "<i4"), ("code", "<u4"), ("state", "<i4"), ("initialized", "<i4"), ("dash", "<i4"), ("wspace", "<i4"), ("timeout", "<i4"), ("track", "<i4"),
             ("pulse_avg", "<f4"), ("dot_avg", "<f4"), ("dash_avg", "<f4"), ("symspace_avg", "<f4"), ("cwspace_avg", "<f4"), ("w_space", "<i4"),
             ("timer_stepsize", "<i4"), ("cur_time", "<i4"), ("cur_outcount", "<i4"), ("last_outcount", "<i4"),
             ("CW_env", "<f4"), ("CW_mag", "<f4"), ("CW_noise", "<f4"), ("old_siglevel", "<f4"), ("speed_wpm_avg", "<f4"),
             ("prevstate", "<i4"), ("noisecancel_change", "<i4"), ("sample_counter", "<i4"), ("startpos", "<i4"), ("progress", "<i4"), ("initializing", "<i4"),
             ("processed", "<i4"), ("training_interval", "<i4"),
             ("snd_rate", "<i4"), ("slowdown", "<i4"), ("started", "<i4"), ("pad0", "<i4"), ("pad1", "<i4")])
info_dtype = np.dtype(_scalars + [("sig", "<u4", (256,)), ("data", "<u4", (40,)), ("raw", "<f4", (GBLK,))])
assert ev_dtype.itemsize == 24 and info_dtype.itemsize == 1760


def chars(code):
    """what cw_print sends for a CHARS event's code (:972-981)"""
    code = int(code)
    return "[err]" if code == 0xff else PROSIGNS[code] if code < 12 else chr(code)


def messages(evs):
    """events -> the text lines the client receives; the cw_chars text is sent encoded by the reference (:961) and stands plain here"""
    out = []
    for e in evs:
        k, a = int(e["kind"]), int(e["a"])
        if k == CHARS:
            out.append("EXT cw_chars=" + chars(a))
        elif k == WPM:
            out.append("EXT cw_wpm=%d" % a)
        elif k == TRAIN:
            out.append("EXT cw_train=%d" % a)
        else:
            f = np.array([a, int(e["c"])], np.int32).view(np.float32)
            out.append("EXT cw_plot=%.2f,%d,%.2f" % (float(f[0]), int(e["b"]), float(f[1])))
    return out


def text(evs):
    """the decoded text alone"""
    return "".join(chars(e["a"]) for e in evs if int(e["kind"]) == CHARS)


class CwDecoder:
    """nconn cw_decoder_t objects (uhsdr_cw_decoder.cpp:176) on the GPU (kg_cw)"""

    def __init__(self, ctx=None, nconn=1, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nconn = int(nconn)
        h = C.c_void_p()
        check(self.lib.kg_cw_create(self.ctx.h, int(nconn), C.byref(h)), "kg_cw_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None) and not getattr(self, "_borrowed", False):
                self.lib.kg_cw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def start(self, conn, training_interval=100, nom_rate=12000.0, srate=None):
        """the default interval is CwDecode_Init's (uhsdr_cw_decoder.h:26)"""
        check(self.lib.kg_cw_start(self.h, int(conn), int(training_interval), float(nom_rate), float(nom_rate if srate is None else srate)), "kg_cw_start")

    def set_wpm(self, conn, wpm, training_interval=100):
        """-> the message the reference sends from the command itself (:385), or None"""
        check(self.lib.kg_cw_set_wpm(self.h, int(conn), int(wpm), int(training_interval)), "kg_cw_set_wpm")
        return "EXT cw_train=0" if int(wpm) != 0 else None

    def set_pboff(self, conn, pboff):
        check(self.lib.kg_cw_set_pboff(self.h, int(conn), int(pboff) & 0xffffffff), "kg_cw_set_pboff")

    def set_wsc(self, conn, wsc):
        check(self.lib.kg_cw_set_wsc(self.h, int(conn), int(wsc)), "kg_cw_set_wsc")

    def set_auto_threshold(self, conn, on):
        check(self.lib.kg_cw_set_auto_threshold(self.h, int(conn), int(on)), "kg_cw_set_auto_threshold")

    def set_threshold(self, conn, threshold):
        check(self.lib.kg_cw_set_threshold(self.h, int(conn), int(threshold)), "kg_cw_set_threshold")

    def stop(self, conn):
        check(self.lib.kg_cw_stop(self.h, int(conn)), "kg_cw_stop")

    def max_events(self, nblk):
        n = self.lib.kg_cw_max_events(int(nblk))
        if n < 0:
            raise ValueError("nblk %d" % nblk)
        return n

    def push(self, conns, s16, now_sec, nblk=None):
        """host arrays: s16 int16 [entries, blocks, 512], now_sec [entries] -> per entry the events (ev_dtype); synchronises"""
        if getattr(self, "_borrowed", False):
            raise RuntimeError("a receiver bank's CwDecoder is fed by the bank's steps")
        s16 = np.ascontiguousarray(s16, np.int16)
        assert s16.ndim == 3 and s16.shape[2] == BLK
        nent, nb, _ = s16.shape
        conns = np.ascontiguousarray(conns, np.int32)
        now_sec = np.ascontiguousarray(now_sec, np.uint32)
        nblk = np.full(nent, nb, np.int32) if nblk is None else np.ascontiguousarray(nblk, np.int32)
        assert conns.size == nent == nblk.size == now_sec.size
        me = max(self.max_events(int(nblk.max()) if nent else 0), 1)
        evs = np.zeros((nent, me), ev_dtype)
        counts = np.zeros(4 * nent, np.int32)
        check(self.lib.kg_cw_push(self.h, ptr(conns), int(nent), ptr(nblk), ptr(s16), int(max(nb, 1) * BLK), ptr(now_sec), ptr(evs), int(me), ptr(counts)),
              "kg_cw_push")
        counts = counts.reshape(nent, 4)
        self.last_counts = counts                # per entry: events, Goertzel blocks completed, overflow, 0
        assert not counts[:, 2].any(), "the event capacity was exceeded"
        return [evs[i, :counts[i, 0]].copy() for i in range(nent)]

    def state(self, conn):
        """-> the info record of info_dtype: the scalars, the ring and data[]; synchronises"""
        info = np.zeros(1, info_dtype)
        check(self.lib.kg_cw_state(self.h, int(conn), ptr(info)), "kg_cw_state")
        return info[0]
