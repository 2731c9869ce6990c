"""A Python model of the ephemeris decode (kg_eph), a third implementation beside the reference's and csrc/kg_eph.h's: a frame is one big
integer, fields are shifts and masks, constants come from float.fromhex, doubles are Python floats (IEEE binary64, one rounding per
operation, in the reference's order).  Plain helper, imported like tests/nav_model.py."""
import struct

import numpy as np

from flydog_sdr_gps_amd import eph, nav

H = float.fromhex
# rtklib.h:421-444, sdrnav_gal.cpp:16-18: the doubles the decimal text gives
P2_5, P2_19, P2_21, P2_29, P2_30, P2_31, P2_34, P2_59 = (H("0x1p-5"), H("0x1p-19"), H("0x1p-21"), H("0x1p-29"), H("0x1p-30"), H("0x1p-31"), H("0x1p-34"),
                                                         H("0x1p-59"))
P2_32, P2_33, P2_35, P2_43, P2_46 = (H("0x1.fffffffffffffp-33"), H("0x1.fffffffffffffp-34"), H("0x1.fffffffffffffp-36"), H("0x1.ffffffffffffep-44"),
                                     H("0x1.ffffffffffffep-47"))
PI = SC2RAD = H("0x1.921fb54442d28p+1")                 # gps.h:87, rtklib.h:61: 3.1415926535898
CPS = H("0x1.f383p+19")
WEEK = 604800


def signed(v, n):
    return v - (1 << n) if v >> (n - 1) else v


class Bits:
    def __init__(self, data, nbytes):
        self.v, self.n = int.from_bytes(bytes(bytearray(data[:nbytes])), "big"), 8 * nbytes

    def u(self, pos, n):
        return (self.v >> (self.n - pos - n)) & ((1 << n) - 1)

    def s(self, pos, n):
        return signed(self.u(pos, n), n)


def gst2gpst(week_gst, sec):
    """-> (tow, week) in GPS time: GST starts 1024 weeks after GPS time"""
    t = WEEK * (1024 + week_gst) + sec
    return t % WEEK, t // WEEK


class Model:
    def __init__(self, nchan=12):
        self.slot = np.zeros(eph.MAX_SATS, eph.ephem_dtype)
        self.chan = [dict(sat=-1, kind=0, week_gst=0, toes=0, toc_gst=0) for _ in range(nchan)]
        self.utc = dict(delta_tLS=0, delta_tLSF=0, tLS_valid=0)

    @staticmethod
    def valid(e):
        if e["kind"] == eph.E1B:
            return int(e["IODN"][0] != 0 and len(set(int(v) for v in e["IODN"])) == 1)
        return int(e["IODC"] != 0 and e["IODC"] == e["IODE2"] and e["IODC"] == e["IODE3"])

    def set_sat(self, ch, sat, kind):
        for c, st in enumerate(self.chan):
            if sat >= 0 and c != ch and st["sat"] == sat:
                raise ValueError("satellite %d is bound to channel %d" % (sat, c))
        self.chan[ch]["sat"], self.chan[ch]["kind"] = sat, kind
        if sat >= 0:
            self.slot[sat]["kind"] = kind
            self.slot[sat]["valid"] = self.valid(self.slot[sat])

    def clear_sat(self, sat):
        k = self.slot[sat]["kind"]
        self.slot[sat] = np.zeros((), eph.ephem_dtype)
        self.slot[sat]["kind"] = k

    def clear_chan(self, ch):
        self.chan[ch].update(week_gst=0, toes=0, toc_gst=0)

    # ---- one frame
    def push(self, ch, fr):
        """fr: one nav.frame_dtype record -> the note (a 0-d note_dtype array)"""
        c = self.chan[ch]
        n = np.zeros((), eph.note_dtype)
        n["bit_next"] = int(fr["bit"]) + int(fr["consumed"])
        if c["sat"] < 0:
            return n
        e = self.slot[c["sat"]]
        err = int(fr["err"])
        if c["kind"] == eph.E1B:
            applied = err in (0, nav.ERR_OOS)
            upd = self._e1b(e, c, fr) if applied else 0
        else:
            applied = err == 0
            upd = self._ca(e, c, fr) if applied else 0
        if applied:
            e["valid"] = self.valid(e)
            if upd:
                e["tow_bit"] = n["bit_next"]
        n["applied"], n["tow_updated"], n["sub"], n["valid"], n["tow"], n["week"] = int(applied), upd, e["sub"], e["valid"], e["tow"], e["week"]
        return n

    def _ca(self, e, c, fr):
        raw = Bits(fr["data"], 38)
        v = 0
        for w in range(10):                             # the 24 data bits of every word: nav[30] as one integer
            v = (v << 24) | raw.u(30 * w, 24)
        b = Bits(v.to_bytes(30, "big"), 30)
        sub = raw.u(49, 3)
        e["sub"] = e["tow_pg"] = sub
        e["tow"] = b.u(8 * 3, 17) * 6
        B = lambda byte, n: b.u(8 * byte, n)            # noqa: E731
        S = lambda byte, n: b.s(8 * byte, n)            # noqa: E731
        if sub == 1:
            e["week"] = B(6, 10)
            e["t_gd"] = 2.0 ** -31 * S(20, 8)
            e["IODC"] = B(21, 8)
            e["t_oc"] = 16 * B(22, 16)
            e["a_f"] = [2.0 ** -31 * S(27, 22), 2.0 ** -43 * S(25, 16), 2.0 ** -55 * S(24, 8)]
        elif sub == 2:
            e["IODE2"] = B(6, 8)
            e["C_rs"] = 2.0 ** -5 * S(7, 16)
            e["dn"] = 2.0 ** -43 * S(9, 16) * PI
            e["M_0"] = 2.0 ** -31 * S(11, 32) * PI
            e["C_uc"] = 2.0 ** -29 * S(15, 16)
            e["e"] = 2.0 ** -33 * B(17, 32)
            e["C_us"] = 2.0 ** -29 * S(21, 16)
            e["sqrtA"] = 2.0 ** -19 * B(23, 32)
            e["t_oe"] = 16 * B(27, 16)
        elif sub == 3:
            e["C_ic"] = 2.0 ** -29 * S(6, 16)
            e["OMEGA_0"] = 2.0 ** -31 * S(8, 32) * PI
            e["C_is"] = 2.0 ** -29 * S(12, 16)
            e["i_0"] = 2.0 ** -31 * S(14, 32) * PI
            e["C_rc"] = 2.0 ** -5 * S(18, 16)
            e["omega"] = 2.0 ** -31 * S(20, 32) * PI
            e["OMEGA_dot"] = 2.0 ** -43 * S(24, 24) * PI
            e["IODE3"] = B(27, 8)
            e["IDOT"] = 2.0 ** -43 * S(28, 14) * PI
        elif sub == 4 and B(6, 8) == (1 << 6) + 56:
            e["alpha"] = [2.0 ** -30 * S(7, 8), 2.0 ** -27 * S(8, 8), 2.0 ** -24 * S(9, 8), 2.0 ** -24 * S(10, 8)]
            e["beta"] = [2.0 ** 11 * S(11, 8), 2.0 ** 14 * S(12, 8), 2.0 ** 16 * S(13, 8), 2.0 ** 16 * S(14, 8)]
            if c["kind"] == eph.NAVSTAR:
                self.utc = dict(delta_tLS=S(24, 8), delta_tLSF=S(27, 8), tLS_valid=1)
        return 1

    def _e1b(self, e, c, fr):
        page = Bits(fr["data"], 30)
        w = Bits((((page.v >> (240 - 114)) & ((1 << 112) - 1)) << 16 | ((page.v >> (240 - 138)) & 0xFFFF)).to_bytes(16, "big"), 16)    # the 128 word bits
        wt = w.u(0, 6)
        e["sub"] = 999 if wt >= 7 else wt
        upd = 0

        def tow_from(sec):
            e["tow"], e["week"] = gst2gpst(c["week_gst"], sec)
            e["tow_pg"] = wt
            return 1
        if wt == 0:
            if w.u(6, 2) == 2:
                c["week_gst"] = w.u(96, 12)
                upd = tow_from(w.u(108, 20) + 2)
        elif wt == 1:
            c["toes"] = w.u(16, 14) * 60
            e["IODN"][0] = w.u(6, 10)
            e["M_0"] = w.s(30, 32) * P2_31 * SC2RAD
            e["e"] = w.u(62, 32) * P2_33
            e["sqrtA"] = w.u(94, 32) * P2_19
            if c["week_gst"] != 0:
                toe = gst2gpst(c["week_gst"], c["toes"])[0]
                if toe != 0:
                    e["t_oe"] = toe
        elif wt == 2:
            e["IODN"][1] = w.u(6, 10)
            e["OMEGA_0"] = w.s(16, 32) * P2_31 * SC2RAD
            e["i_0"] = w.s(48, 32) * P2_31 * SC2RAD
            e["omega"] = w.s(80, 32) * P2_31 * SC2RAD
            e["IDOT"] = w.s(112, 14) * P2_43 * SC2RAD
        elif wt == 3:
            e["IODN"][2] = w.u(6, 10)
            e["OMEGA_dot"] = w.s(16, 24) * P2_43 * SC2RAD
            e["dn"] = w.s(40, 16) * P2_43 * SC2RAD
            e["C_uc"] = w.s(56, 16) * P2_29
            e["C_us"] = w.s(72, 16) * P2_29
            e["C_rc"] = w.s(88, 16) * P2_5
            e["C_rs"] = w.s(104, 16) * P2_5
        elif wt == 4:
            c["toc_gst"] = w.u(54, 14) * 60
            e["IODN"][3] = w.u(6, 10)
            e["C_ic"] = w.s(22, 16) * P2_29
            e["C_is"] = w.s(38, 16) * P2_29
            e["a_f"] = [w.s(68, 31) * P2_34, w.s(99, 21) * P2_46, w.s(120, 6) * P2_59]
            if c["week_gst"] != 0:
                toc = gst2gpst(c["week_gst"], c["toc_gst"])[0]
                if toc != 0:
                    e["t_oc"] = toc
        elif wt == 5:
            c["week_gst"] = w.u(73, 12)
            upd = tow_from(w.u(85, 20) + 2)
            e["t_gd"] = w.s(57, 10) * P2_32
            for src, dst in (("toc_gst", "t_oc"), ("toes", "t_oe")):
                if c[src] != 0:
                    t = gst2gpst(c["week_gst"], c[src])[0]
                    if t != 0:
                        e[dst] = t
        elif wt == 6:
            if c["week_gst"] != 0:
                upd = tow_from(w.u(105, 20) + 2)
        elif wt == 10:
            e["A_0G"] = w.s(86, 16) * P2_35
            e["A_1G"] = w.s(102, 12) * P2_30 * P2_21
            e["t_0G"] = w.u(114, 8) * 3600
            e["WN_0G"] = w.u(122, 6)
        return upd

    # ---- SNAPSHOT::GetClock
    def get_clock(self, s):
        """s: one snap_dtype record of a Valid satellite -> (clock, flags)"""
        e = self.slot[int(s["sat"])]
        e1b = e["kind"] == eph.E1B
        ms, chips, cg, bits, bits_tow = (int(s[k]) for k in ("ms", "chips", "cg_phase", "bits", "bits_tow"))
        if e1b and ((ms != 0 and ms != 4) or chips < 0 or chips > 4091):
            return float("nan"), eph.SV_BAD
        flags = 0
        if bits != bits_tow and bits_tow < 2500:
            bits, flags = bits_tow, eph.SV_TOW_DELAYED
        tow = float(int(e["tow"]))
        if e1b:
            return tow + bits / 250.0 + ms * 1e-3 + chips / CPS + 0.25 / CPS + cg * 2.0 ** -6 / CPS, flags
        return tow + bits / 50.0 + ms * 1e-3 + chips / CPS + cg * 2.0 ** -6 / CPS, flags


def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def run(events, frames, nchan=12):
    """the events of a golden scenario through a fresh model -> (model, [(ephem bytes, (week_gst, toes, toc_gst), utc tuple, note bytes) per frame])"""
    m = Model(nchan)
    out = [None] * len(frames)
    for op, ch, a, b in events:
        if op == 0:
            m.set_sat(int(ch), int(a), int(b))
            continue
        n = m.push(int(ch), frames[a])
        c = m.chan[ch]
        out[a] = (m.slot[c["sat"]].tobytes(), (c["week_gst"], c["toes"], c["toc_gst"]), (m.utc["delta_tLS"], m.utc["delta_tLSF"], m.utc["tLS_valid"]),
                  n.tobytes())
    return m, out
