"""Ephemeris decode and satellite position and clock over the C ABI (kg_eph): what turns validated frames into numbers.

Reference                                                                       here
  EPHEM::Subframe, Subframe1..4, LoadPage18   gps/ephemeris.cpp:51-110, :228-252   -> Ephemerides.push_frames / push_frames_dev
  decode_page_e1b, decode_word0..6, 10        gps/GNSS-SDRLIB/sdrnav_gal.cpp       -> (inside the kernels)
  EPHEM::PageN, Page0..6, Valid               gps/ephemeris.cpp:218-224, :256-370  -> Ephemerides.get
  SNAPSHOT::GetClock, LoadFromReplicas' body  gps/solve.cpp:168-244, :319-361      -> Ephemerides.sv / sv_dev
  GetClockCorrection, GetXYZ, ...             gps/ephemeris.cpp:114-207            -> (inside the kernel)

Not here: PosSolver and everything behind GNSSDataForEpoch (pos.py has them), the glitch guard, probation / alert / abort, tow_time, almanac words.

subframe_words() and inav_word() are ENCODERS (raw integer fields -> the words nav.l1_subframe / nav.e1b_page take): input generators
for tests and synthetic scenes, not part of the measured path.
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, ptr  # noqa: F401
from . import nav

NAVSTAR, CA, E1B = 0, 1, 2
MAX_SATS, MAX_CHANS = 64, 12
SV_NOT_VALID, SV_POWER, SV_TOW_DELAYED, SV_BAD, SV_TOO_OLD = 1, 2, 4, 8, 16

ephem_dtype = np.dtype([
    ("IODN", "<u4", (4,)), ("IODC", "<u4"), ("t_oc", "<u4"), ("t_gd", "<f8"), ("a_f", "<f8", (3,)),
    ("IODE2", "<u4"), ("t_oe", "<u4"), ("C_rs", "<f8"), ("dn", "<f8"), ("M_0", "<f8"), ("C_uc", "<f8"), ("e", "<f8"), ("C_us", "<f8"), ("sqrtA", "<f8"),
    ("IODE3", "<u4"), ("kind", "<u4"), ("C_ic", "<f8"), ("OMEGA_0", "<f8"), ("C_is", "<f8"), ("i_0", "<f8"), ("C_rc", "<f8"), ("omega", "<f8"),
    ("OMEGA_dot", "<f8"), ("IDOT", "<f8"), ("alpha", "<f8", (4,)), ("beta", "<f8", (4,)),
    ("week", "<u4"), ("tow", "<u4"), ("sub", "<u4"), ("tow_pg", "<u4"), ("A_0G", "<f8"), ("A_1G", "<f8"), ("t_0G", "<u4"), ("WN_0G", "<u4"),
    ("valid", "<i4"), ("pad_", "<i4"), ("tow_bit", "<u8")])
note_dtype = np.dtype([("applied", "<i4"), ("tow_updated", "<i4"), ("sub", "<i4"), ("valid", "<i4"), ("tow", "<u4"), ("week", "<u4"), ("bit_next", "<u8")])
snap_dtype = np.dtype([("sat", "<i4"), ("bits", "<i4"), ("bits_tow", "<i4"), ("ms", "<i4"), ("chips", "<i4"), ("cg_phase", "<i4"), ("power", "<f4")])
sv_dtype = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("ct", "<f8"), ("t_k", "<f8"), ("week", "<i4"), ("flags", "<i4")])
assert (ephem_dtype.itemsize, note_dtype.itemsize, snap_dtype.itemsize, sv_dtype.itemsize) == (312, 32, 28, 48)


class Ephemerides:
    """64 satellite slots fed by nchan channels on the GPU (kg_eph)"""

    def __init__(self, ctx=None, nchan=MAX_CHANS, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nchan = int(nchan)
        h = C.c_void_p()
        check(self.lib.kg_eph_create(self.ctx.h, int(nchan), C.byref(h)), "kg_eph_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.lib.kg_eph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sat(self, ch, sat, kind=NAVSTAR):
        """binds a channel to a satellite slot as CHANNEL::Start does (sat = -1 unbinds); the channel's Galileo state and the slot stay"""
        check(self.lib.kg_eph_set_sat(self.h, int(ch), int(sat), int(kind)), "kg_eph_set_sat")

    def clear_sat(self, sat):
        check(self.lib.kg_eph_clear_sat(self.h, int(sat)), "kg_eph_clear_sat")

    def clear_chan(self, ch):
        check(self.lib.kg_eph_clear_chan(self.h, int(ch)), "kg_eph_clear_chan")

    def push_frames_dev(self, d_frames, frame_stride, d_counts, cap, d_notes, note_stride):
        """enqueue only: the rows and counts of NavSync.push_dev / push_epochs_dev (device addresses), cap that call's cap"""
        check(self.lib.kg_eph_push_frames_dev(self.h, C.c_void_p(int(d_frames)), int(frame_stride), C.c_void_p(int(d_counts)), int(cap),
                                              C.c_void_p(int(d_notes)), int(note_stride)), "kg_eph_push_frames_dev")

    def push_frames(self, frames):
        """frames: one nav.frame_dtype array per channel (any may be empty) -> [note_dtype array per channel]"""
        assert len(frames) == self.nchan
        rows = [np.ascontiguousarray(f, nav.frame_dtype).reshape(-1) for f in frames]
        counts = np.array([r.size for r in rows], np.int32)
        cap = int(counts.max())
        stride = max(cap, 1)
        host = np.zeros((self.nchan, stride), nav.frame_dtype)
        for ch, r in enumerate(rows):
            host[ch, :r.size] = r
        notes = np.zeros((self.nchan, stride), note_dtype)
        check(self.lib.kg_eph_push_frames(self.h, ptr(host), stride, ptr(counts), cap, ptr(notes), stride), "kg_eph_push_frames")
        return [notes[ch, :counts[ch]].copy() for ch in range(self.nchan)]

    def get(self, sat):
        """-> the satellite's kg_ephem (a 0-d ephem_dtype array); synchronises"""
        out = np.zeros((), ephem_dtype)
        check(self.lib.kg_eph_get(self.h, int(sat), ptr(out)), "kg_eph_get")
        return out

    def chan(self, ch):
        """-> dict(sat, week_gst, toes, toc_gst); synchronises"""
        sat = C.c_int32()
        g = np.zeros(3, np.uint32)
        check(self.lib.kg_eph_get_chan(self.h, int(ch), C.byref(sat), ptr(g)), "kg_eph_get_chan")
        return dict(sat=sat.value, week_gst=int(g[0]), toes=int(g[1]), toc_gst=int(g[2]))

    def utc(self):
        """-> dict(delta_tLS, delta_tLSF, tLS_valid); synchronises"""
        u = np.zeros(3, np.int32)
        check(self.lib.kg_eph_get_utc(self.h, ptr(u)), "kg_eph_get_utc")
        return dict(delta_tLS=int(u[0]), delta_tLSF=int(u[1]), tLS_valid=int(u[2]))

    def sv_dev(self, d_snaps, nsnap, d_out):
        """enqueue only: nsnap snap_dtype records at d_snaps -> sv_dtype records at d_out (device addresses)"""
        check(self.lib.kg_eph_sv_dev(self.h, C.c_void_p(int(d_snaps)), int(nsnap), C.c_void_p(int(d_out))), "kg_eph_sv_dev")

    def sv(self, snaps, out=None):
        """snaps: snap_dtype array -> sv_dtype array; a snapshot refused for NOT_VALID or POWER keeps what `out` held but for flags"""
        s = np.ascontiguousarray(snaps, snap_dtype).reshape(-1)
        o = np.zeros(s.size, sv_dtype) if out is None else out
        assert o.dtype == sv_dtype and o.size == s.size and o.flags["C_CONTIGUOUS"]
        check(self.lib.kg_eph_sv(self.h, ptr(s), s.size, ptr(o)), "kg_eph_sv")
        return o

    def replica(self, word):
        """the 18-bit replica word of Tracker.clocks -> (chips, cg_phase), by LoadAtomic's masks"""
        chips, cg = C.c_int32(), C.c_int32()
        self.lib.kg_eph_replica(int(word) & 0xFFFFFFFF, C.byref(chips), C.byref(cg))
        return chips.value, cg.value


# ---- encoders
# C/A: (first nav[] byte, bits taken from the top of the bytes from there on) as EPHEM::Subframe1..4 / LoadPage18 read them; nav[j] is
# byte j % 3 of the 24 data bits of word j // 3
L1_FIELDS = {
    1: dict(week=(6, 10), t_gd=(20, 8), IODC=(21, 8), t_oc=(22, 16), a_f2=(24, 8), a_f1=(25, 16), a_f0=(27, 22)),
    2: dict(IODE2=(6, 8), C_rs=(7, 16), dn=(9, 16), M_0=(11, 32), C_uc=(15, 16), e=(17, 32), C_us=(21, 16), sqrtA=(23, 32), t_oe=(27, 16)),
    3: dict(C_ic=(6, 16), OMEGA_0=(8, 32), C_is=(12, 16), i_0=(14, 32), C_rc=(18, 16), omega=(20, 32), OMEGA_dot=(24, 24), IODE3=(27, 8),
            IDOT=(28, 14)),
    4: dict(page=(6, 8), alpha0=(7, 8), alpha1=(8, 8), alpha2=(9, 8), alpha3=(10, 8), beta0=(11, 8), beta1=(12, 8), beta2=(13, 8), beta3=(14, 8),
            delta_tLS=(24, 8), delta_tLSF=(27, 8)),
    5: dict(),
}
PAGE18 = (1 << 6) + 56
# I/NAV: (first word bit, length); word bit k is page bit OFFSET1 + k below 112 and OFFSET2 + k - 112 from there
INAV_FIELDS = {
    0: dict(time=(6, 2), week=(96, 12), tow=(108, 20)),
    1: dict(iodc=(6, 10), toes=(16, 14), M0=(30, 32), e=(62, 32), sqrtA=(94, 32)),
    2: dict(iodc=(6, 10), OMG0=(16, 32), i0=(48, 32), omg=(80, 32), idot=(112, 14)),
    3: dict(iodc=(6, 10), OMGd=(16, 24), deln=(40, 16), cuc=(56, 16), cus=(72, 16), crc=(88, 16), crs=(104, 16)),
    4: dict(iodc=(6, 10), cic=(22, 16), cis=(38, 16), toc=(54, 14), f0=(68, 31), f1=(99, 21), f2=(120, 6)),
    5: dict(bgd_e5a=(47, 10), bgd_e5b=(57, 10), e5bhs=(67, 2), e1bhs=(69, 2), e5bdvs=(71, 1), e1bdvs=(72, 1), week=(73, 12), tow=(85, 20)),
    6: dict(tow=(105, 20)),
    10: dict(A_0G=(86, 16), A_1G=(102, 12), t_0G=(114, 8), WN_0G=(122, 6)),
}


def _put(bits, pos, n, value):
    v = int(value) & ((1 << n) - 1)                     # two's complement for negative raw fields
    bits[pos:pos + n] = [(v >> (n - 1 - k)) & 1 for k in range(n)]


def subframe_words(sub, fields, tow=0, fill=None):
    """Ten 24-bit source words for nav.l1_subframe: the preamble, `tow` (the 17-bit count, the seconds / 6) and subframe id `sub` in the
    hand-over word, and the raw integer `fields` (names of L1_FIELDS[sub]; negative values in two's complement) where EPHEM::Subframe
    reads them.  fill: 240 background bits (default zeros) for everything else."""
    bits = np.zeros(240, np.uint8) if fill is None else (np.asarray(fill, np.uint8).reshape(240) & 1).copy()
    _put(bits, 0, 8, 0x8B)
    _put(bits, 24, 17, tow)
    _put(bits, 24 + 19, 3, sub)
    table = L1_FIELDS.get(int(sub), {})
    for name, value in fields.items():
        byte, n = table[name]
        _put(bits, 8 * byte, n, value)
    return [int("".join(str(int(b)) for b in bits[24 * w:24 * w + 24]), 2) for w in range(10)]


def words_fields(sub, words24):
    """the inverse of subframe_words: -> (tow count, {name: raw unsigned field})"""
    bits = np.array([(int(w) >> (23 - k)) & 1 for w in words24 for k in range(24)], np.uint8)

    def get(pos, n):
        return int("".join(str(int(b)) for b in bits[pos:pos + n]), 2)
    return get(24, 17), {name: get(8 * byte, n) for name, (byte, n) in L1_FIELDS.get(int(sub), {}).items()}


def inav_word(wtype, fields, fill=None):
    """The 128 bits of one I/NAV word for nav.e1b_page: type `wtype` and the raw integer `fields` (names of INAV_FIELDS[wtype]) where
    decode_word0..6 / 10 read them.  fill: 128 background bits (default zeros)."""
    bits = np.zeros(128, np.uint8) if fill is None else (np.asarray(fill, np.uint8).reshape(128) & 1).copy()
    _put(bits, 0, 6, wtype)
    table = INAV_FIELDS.get(int(wtype), {})
    for name, value in fields.items():
        pos, n = table[name]
        _put(bits, pos, n, value)
    return bits


def inav_fields(word128_bits):
    """the inverse of inav_word: -> (type, {name: raw unsigned field})"""
    bits = np.asarray(word128_bits, np.uint8).reshape(128)

    def get(pos, n):
        return int("".join(str(int(b)) for b in bits[pos:pos + n]), 2)
    wtype = get(0, 6)
    return wtype, {name: get(pos, n) for name, (pos, n) in INAV_FIELDS.get(wtype, {}).items()}
