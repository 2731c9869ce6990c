"""Generates tests/golden/eph_ref.npz from the REFERENCE ITSELF: EPHEM::Subframe and the Galileo word decoders with EPHEM::Page*, then
SNAPSHOT::GetClock, GetClockCorrection, TimeOfEphemerisAge and GetXYZ as LoadFromReplicas calls them.

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  In the manner of tools/make_ref_nav_golden.py it cuts line ranges of the reference into a temporary directory
(deleted on exit), checks the text at both ends of every cut, the text of every statement the harness restates and the decimal text of
every constant, compiles tools/ref/ref_eph_main.cpp around them, runs it on seeded frames (built here with the encoders of
flydog_sdr_gps_amd/eph.py and nav.py) and keeps only data: the frames, the snapshots and the records the reference's code printed.
The conditions at the end keep every later test from passing on an empty set.

    python tools/make_ref_eph_golden.py
"""
import os
import subprocess
import tempfile

import numpy as np

import ref_cut
from ref_cut import ROOT, read  # ref_cut puts the repository root on sys.path
from flydog_sdr_gps_amd import eph, nav  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
GPSH, GPSC, EH, EC, SOLVE, CH = "gps/gps.h", "gps/gps.cpp", "gps/ephemeris.h", "gps/ephemeris.cpp", "gps/solve.cpp", "gps/channel.cpp"
RTKH, RTK, NAVC, GAL, SDRH = ("gps/GNSS-SDRLIB/rtklib.h", "gps/GNSS-SDRLIB/rtkcmn.cpp", "gps/GNSS-SDRLIB/sdrnav.cpp", "gps/GNSS-SDRLIB/sdrnav_gal.cpp",
                              "gps/GNSS-SDRLIB/gnss_sdrlib.h")

# (file, macro, first, last, text of the first line, text of the last line)
CUTS = [
    (GPSH, "EPH_CUT_GPS_RATES", 46, 55, "#define CPS 1.023e6", "#define E1B_BPS 250.0"),
    (GPSH, "EPH_CUT_GPS_CONST", 87, 94, "const double PI = 3.1415926535898;", "const double F = -4.442807633e-10;"),
    (GPSH, "EPH_CUT_GPSERR", 187, 191, "#define GPS_ERR_SLIP    1", "#define GPS_ERR_PAGE    5"),
    (GPSH, "EPH_CUT_UMS", 289, 296, "struct UMS {", "};"),
    (GPSC, "EPH_CUT_BIN", 32, 36, "unsigned bin(char *s, int n) {", "}"),
    (EH, "EPH_CUT_EPHEM_H", 23, 82, "class EPHEM {", "};"),
    (EC, "EPH_CUT_EPHEM_TIME", 31, 47, "static double TimeFromEpoch(double t, double t_ref) {", "};"),
    (EC, "EPH_CUT_EPHEM_SUB", 51, 110, "void EPHEM::Subframe1(char *nav) {", "}"),
    (EC, "EPH_CUT_EPHEM_POS", 114, 207, "double EPHEM::TimeOfEphemerisAge(double t) const {", "}"),
    (EC, "EPH_CUT_EPHEM_FRAME", 211, 252, "void EPHEM::Init(int sat) {", "}"),
    (EC, "EPH_CUT_EPHEM_PAGES", 256, 370, "void EPHEM::PageN(unsigned page) {", "}"),
    (SOLVE, "EPH_CUT_SNAPSHOT", 42, 52, "struct SNAPSHOT {", "};"),
    (SOLVE, "EPH_CUT_GETCLOCK", 168, 244, "double SNAPSHOT::GetClock() const {", "}"),
    (RTKH, "EPH_CUT_SC2RAD", 61, 61, "#define SC2RAD      3.1415926535898 ", "#define SC2RAD"),
    (RTKH, "EPH_CUT_P2", 421, 444, "#define P2_5        0.03125 ", "#define P2_55       2.775557561562891E-17"),
    (RTKH, "EPH_CUT_GTIME", 464, 467, "typedef struct {        /* time struct */", "} gtime_t;"),
    (RTKH, "EPH_CUT_EPH_T", 525, 544, "typedef struct {        /* GPS/QZS/GAL broadcast ephemeris type */", "} eph_t;"),
    (RTK, "EPH_CUT_EPOCHS", 125, 126, "const static double gpst0[]={1980,1, 6,0,0,0};", "const static double gst0 []={1999,8,22,0,0,0};"),
    (RTK, "EPH_CUT_GETBIT", 598, 610, "extern unsigned int getbitu(", "}"),
    (RTK, "EPH_CUT_EPOCH2TIME", 1201, 1215, "extern gtime_t epoch2time(const double *ep)", "}"),
    (RTK, "EPH_CUT_TIME2GPST", 1261, 1269, "extern double time2gpst(gtime_t t, int *week)", "}"),
    (RTK, "EPH_CUT_GST2TIME", 1276, 1284, "extern gtime_t gst2time(int week, double sec)", "}"),
    (NAVC, "EPH_CUT_GETBIT2", 94, 104, "extern uint32_t getbitu2(", "}"),
    (GAL, "EPH_CUT_GAL_DEFS", 16, 20, "#define P2_34       5.820766091346741E-11", "#define OFFSET2     122"),
    (GAL, "EPH_CUT_GAL_WORDS", 28, 286, "void decode_word1(const uint8_t *buff, sdrnav_t *nav)", "}"),
    (GAL, "EPH_CUT_GAL_PAGE", 327, 359, "extern int decode_page_e1b(const uint8_t *buff1, const uint8_t *buff2,", "}"),
]
# what the harness restates: (file, line, text)
PINS = [
    (SDRH, 134, "#define ON            1"), (SDRH, 483, "double tow_gpst;"), (SDRH, 484, "int week_gpst;"), (SDRH, 490, "double toc_gst;"),
    (SDRH, 491, "int week_gst;"), (RTKH, 537, "double toes;"),
    ("kiwi.config", 251, "MAX_NAV_BITS\t128"), ("kiwi.config", 267, "L1_CODELEN      1023"), ("kiwi.config", 271, "E1B_CODELEN     4092"),
    (GPSH, 98, "typedef enum { Navstar, SBAS, QZSS, E1B } sat_e;"), (GPSH, 118, "#define is_Navstar(sat)     (Sats[sat].type == Navstar)"),
    (GPSH, 121, "#define is_E1B(sat)         (Sats[sat].type == E1B)"), (GPSH, 123, "#define MAX_SATS    64"),
    (CH, 274, "this->sat = sat;"), (CH, 276, "nav.sat = sat;"), (CH, 277, "Ephemeris[sat].Init(sat);"),
    (CH, 754, "nav.tow_updated = 0;"), (CH, 756, "int id = E1B_subframe(&nav, &error);"),
    (CH, 758, "if (error == GPS_ERR_SLIP) return *nbits = E1B_TSYM_PP;"),
    (CH, 759, "if (error && (error != GPS_ERR_ALERT && error != GPS_ERR_OOS)) {"), (CH, 764, "if (nav.tow_updated)"),
    (CH, 825, "Ephemeris[sat].Subframe(buf);"), (CH, 827, "bits_tow = holding - subframe_bits;"),
    (GAL, 478, "if (!err && getbitu(dec_e1b1,1,1) && getbitu(dec_e1b2,1,1)) {"), (GAL, 480, "err = GPS_ERR_ALERT;"), (GAL, 483, "if (!err) {"),
    (GAL, 485, "id = decode_page_e1b(dec_e1b1, dec_e1b2, nav, &err);"),
    (SOLVE, 71, "&& Ephemeris[sat].Valid()) {"), (SOLVE, 73, "isE1B = is_E1B(sat);"), (SOLVE, 77, "chips = ((dn[0] & 0x3) << 10) | (dn[-1] & 0x3FF);"),
    (SOLVE, 79, "cg_phase = dn[-1] >> 10;"), (SOLVE, 81, "memcpy(&eph, Ephemeris+sat, sizeof eph);"),
    (SOLVE, 327, "_weight[_chans] = replicas[i].power;"), (SOLVE, 330, "if (_weight[_chans] < 1e5 || _weight[_chans] > 5e6)"),
    (SOLVE, 334, "double t_tx = replicas[i].GetClock();"), (SOLVE, 335, "if (t_tx == NAN)"),
    (SOLVE, 339, "t_tx -= replicas[i].eph.GetClockCorrection(t_tx);"), (SOLVE, 340, "_sv[3][_chans] = C*t_tx;"),
    (SOLVE, 342, "double t_k = replicas[i].eph.TimeOfEphemerisAge(t_tx);"), (SOLVE, 343, "UMS hms(fabs(t_k)/60/60);"),
    (SOLVE, 345, "gps.ch[i].too_old = (hms.u >= 4);"), (SOLVE, 354, "t_tx);"), (SOLVE, 360, "_week[_chans] = replicas[i].eph.week;"),
    (SOLVE, 221, "#define MAX_TOW_DELAY   (5*500)"),
]
# the decimal text of every constant and the double it is: (file, line, name, text, hex)
CONSTS = [
    (RTKH, 421, "P2_5", "0.03125", "0x1.0000000000000p-5"), (RTKH, 426, "P2_19", "1.907348632812500E-06", "0x1.0000000000000p-19"),
    (RTKH, 428, "P2_21", "4.768371582031250E-07", "0x1.0000000000000p-21"), (RTKH, 432, "P2_29", "1.862645149230957E-09", "0x1.0000000000000p-29"),
    (RTKH, 433, "P2_30", "9.313225746154785E-10", "0x1.0000000000000p-30"), (RTKH, 434, "P2_31", "4.656612873077393E-10", "0x1.0000000000000p-31"),
    (RTKH, 435, "P2_32", "2.328306436538696E-10", "0x1.fffffffffffffp-33"), (RTKH, 436, "P2_33", "1.164153218269348E-10", "0x1.fffffffffffffp-34"),
    (RTKH, 437, "P2_35", "2.910383045673370E-11", "0x1.fffffffffffffp-36"), (RTKH, 441, "P2_43", "1.136868377216160E-13", "0x1.ffffffffffffep-44"),
    (GAL, 16, "P2_34", "5.820766091346741E-11", "0x1.0000000000000p-34"), (GAL, 17, "P2_46", "1.421085471520200E-14", "0x1.ffffffffffffep-47"),
    (GAL, 18, "P2_59", "1.734723475976807E-18", "0x1.0000000000000p-59"),
    (RTKH, 61, "SC2RAD", "3.1415926535898", "0x1.921fb54442d28p+1"), (RTKH, 57, "PI", "3.1415926535897932", "0x1.921fb54442d18p+1"),
    (GPSH, 87, "PI", "3.1415926535898", "0x1.921fb54442d28p+1"), (GPSH, 89, "MU", "3.986005e14", "0x1.6a866935b5000p+48"),
    (GPSH, 90, "OMEGA_E", "7.2921151467e-5", "0x1.31da7d7cb8d5bp-14"), (GPSH, 92, "C", "2.99792458e8", "0x1.1de784a000000p+28"),
    (GPSH, 94, "F", "-4.442807633e-10", "-0x1.e87deae177a99p-32"), (GPSH, 46, "CPS", "1.023e6", "0x1.f383000000000p+19"),
]
CONST = {(f, n): float(t) for f, _, n, t, _ in CONSTS}
SC2RAD, PI_EXACT = CONST[(RTKH, "SC2RAD")], CONST[(RTKH, "PI")]

REF_KIND = {eph.NAVSTAR: 0, eph.CA: 2, eph.E1B: 3}                     # sat_e: Navstar, SBAS, QZSS, E1B


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS)
    for f, ln, name, t, hx in CONSTS:
        words = read(f)[ln - 1].replace("=", " ").replace(";", " ").split()
        assert name in words and t in words, ("a constant's text changed", f, ln, name, t)
        assert float(t).hex() == hx, (name, float(t).hex(), hx)
    exe = os.path.join(tmp, "eph_ref")
    cmd = (["g++", "-O2", "-w", "-std=gnu++11", "-ffp-contract=off", "-I" + tmp] + ref_cut.cut_macros(CUTS) +
           ["-o", exe, os.path.join(ROOT, "tools", "ref", "ref_eph_main.cpp")])
    subprocess.run(cmd, check=True)
    return exe


# ---- frames as kg_nav leaves them
rng = np.random.Generator(np.random.PCG64(0x45504801))


def rbits(n):
    return rng.integers(0, 2, n).astype(np.uint8)


def ri(lo, hi):
    return int(rng.integers(lo, hi))


def ca_frame(sub, fields, tow, bit, inverted=0):
    """one C/A record with err 0: the 300 bits as buf holds them after L1_parity (source data bits, parity as transmitted)"""
    words = eph.subframe_words(sub, fields, tow=tow, fill=rbits(240))
    d30 = inverted
    tx = nav.l1_subframe(words, inverted, inverted)
    fixed = tx.copy()
    for w in range(10):
        fixed[30 * w:30 * w + 24] ^= d30
        d30 = int(tx[30 * w + 29])
    r = np.zeros((), nav.frame_dtype)
    r["bit"], r["err"], r["consumed"], r["inverted"], r["id"] = bit, 0, 300, inverted, sub & 7
    r["data"][:38] = np.packbits(fixed)
    return r


def ca_parity_frame(word, bit):
    r = np.zeros((), nav.frame_dtype)
    r["bit"], r["err"], r["consumed"], r["inverted"], r["id"] = bit, nav.ERR_PARITY, 30 * (word + 1), 0, word
    return r


def e1b_frame(wtype, fields, bit, err=0, alert=0, inverted=0):
    """one E1B record: dec_e1b1 and dec_e1b2 of a page that decoded without symbol errors; err as kg_nav reports it"""
    w = eph.inav_word(wtype, fields, fill=rbits(128))
    even = np.concatenate(([0, alert], w[:112])).astype(np.uint8)
    odd = np.concatenate(([1, alert], w[112:], rbits(64))).astype(np.uint8)
    crc = nav.crc24q_bits(np.concatenate((even, odd)))
    if err == nav.ERR_CRC:
        crc ^= 0x5A5
    crc_bits = np.array([(crc >> (23 - k)) & 1 for k in range(24)], np.uint8)
    halves = [np.concatenate((even, np.zeros(6, np.uint8))), np.concatenate((odd, crc_bits, rbits(8), np.zeros(6, np.uint8)))]
    if err == nav.ERR_SLIP:
        halves = halves[::-1]
    r = np.zeros((), nav.frame_dtype)
    r["bit"], r["err"], r["inverted"] = bit, err, inverted
    r["consumed"] = 250 if err == nav.ERR_SLIP else 500
    r["id"] = 0 if err in (nav.ERR_SLIP, nav.ERR_ALERT) else wtype
    r["data"][:30] = np.packbits(np.concatenate(halves))
    return r


# ---- plausible raw fields
def ca_orbit(e_raw=None, toe=None, iod=None):
    """-> {sub: fields} of one complete C/A ephemeris; toe in seconds (a multiple of 16)"""
    iod = ri(1, 256) if iod is None else iod
    toe = 16 * ri(0, 37800) if toe is None else toe
    e_raw = ri(0, int(0.025 * 2 ** 33)) if e_raw is None else e_raw
    return {
        1: dict(week=ri(0, 1024), t_gd=ri(-40, 40), IODC=iod, t_oc=toe // 16, a_f2=ri(-2, 3), a_f1=ri(-3000, 3000), a_f0=ri(-2 ** 20, 2 ** 20)),
        2: dict(IODE2=iod, C_rs=ri(-4000, 4000), dn=ri(8000, 16000), M_0=ri(-2 ** 31, 2 ** 31), C_uc=ri(-3000, 3000), e=e_raw, C_us=ri(-3000, 3000),
                sqrtA=int(round(5153.6 * 2 ** 19)) + ri(-2 ** 18, 2 ** 18), t_oe=toe // 16),
        3: dict(C_ic=ri(-200, 200), OMEGA_0=ri(-2 ** 31, 2 ** 31), C_is=ri(-200, 200), i_0=int(0.3 * 2 ** 31) + ri(-2 ** 26, 2 ** 26), C_rc=ri(4000, 11000),
                omega=ri(-2 ** 31, 2 ** 31), OMEGA_dot=ri(-24000, -21000), IODE3=iod, IDOT=ri(-900, 900)),
    }


def page18():
    return dict(page=eph.PAGE18, alpha0=ri(-128, 128), alpha1=ri(-128, 128), alpha2=ri(-128, 128), alpha3=ri(-128, 128), beta0=ri(-128, 128),
                beta1=ri(-128, 128), beta2=ri(-128, 128), beta3=ri(-128, 128), delta_tLS=ri(10, 30), delta_tLSF=ri(10, 30))


def gal_orbit(iod=None, toes_min=None, e_raw=None):
    """-> {word: fields} of one complete Galileo ephemeris; toes / toc in minutes"""
    iod = ri(1, 1024) if iod is None else iod
    toes_min = ri(1, 10080) if toes_min is None else toes_min
    e_raw = ri(0, int(0.001 * 2 ** 33)) if e_raw is None else e_raw
    return {
        1: dict(iodc=iod, toes=toes_min, M0=ri(-2 ** 31, 2 ** 31), e=e_raw, sqrtA=int(round(5440.6 * 2 ** 19)) + ri(-2 ** 17, 2 ** 17)),
        2: dict(iodc=iod, OMG0=ri(-2 ** 31, 2 ** 31), i0=int(0.31 * 2 ** 31) + ri(-2 ** 25, 2 ** 25), omg=ri(-2 ** 31, 2 ** 31), idot=ri(-900, 900)),
        3: dict(iodc=iod, OMGd=ri(-18000, -15000), deln=ri(6000, 12000), cuc=ri(-3000, 3000), cus=ri(-3000, 3000), crc=ri(3000, 9000),
                crs=ri(-4000, 4000)),
        4: dict(iodc=iod, cic=ri(-200, 200), cis=ri(-200, 200), toc=toes_min, f0=ri(-2 ** 24, 2 ** 24), f1=ri(-2 ** 12, 2 ** 12), f2=ri(-3, 4)),
    }


def word5(week, tow, e1bhs=0, e1bdvs=0):
    return dict(bgd_e5a=ri(-200, 200), bgd_e5b=ri(-400, 400), e5bhs=0, e1bhs=e1bhs, e5bdvs=0, e1bdvs=e1bdvs, week=week, tow=tow)


def word10():
    return dict(A_0G=ri(-2 ** 15, 2 ** 15), A_1G=ri(-2 ** 11, 2 ** 11), t_0G=ri(0, 168), WN_0G=ri(0, 64))


class Stream:
    """the events of one scenario: binds and frames, channel by channel; the bit index of every channel runs on"""

    def __init__(self):
        self.ev, self.frames, self.bit = [], [], {}

    def bind(self, ch, sat, kind):
        self.ev.append((0, ch, sat, kind))
        self.bit[ch] = 0

    def _add(self, ch, r):
        self.ev.append((1, ch, len(self.frames), 0))
        self.frames.append(r.reshape(1))
        self.bit[ch] += int(r["consumed"])

    def ca(self, ch, sub, fields, tow, inverted=0):
        self._add(ch, ca_frame(sub, fields, tow // 6, self.bit[ch], inverted))

    def ca_parity(self, ch, word):
        self._add(ch, ca_parity_frame(word, self.bit[ch]))

    def e1b(self, ch, wtype, fields, **kw):
        self._add(ch, e1b_frame(wtype, fields, self.bit[ch], **kw))


def scenario_ca():
    s = Stream()
    kinds = [eph.NAVSTAR] * 11
    kinds[6] = eph.CA
    for ch in range(11):
        s.bind(ch, ch, kinds[ch])
    # 0: Navstar in order, page 18, subframe 5, a parity error in between
    o = ca_orbit(toe=7200 * 20)
    tow = 7200 * 20 + 3000
    s.ca(0, 1, o[1], tow)
    s.ca_parity(0, 3)
    s.ca(0, 2, o[2], tow + 6)
    s.ca(0, 3, o[3], tow + 12, inverted=1)
    s.ca(0, 4, page18(), tow + 18)
    s.ca(0, 5, {}, tow + 24)
    # 1: out of order, another subframe-4 page, then the same ephemeris again with a new IOD
    o = ca_orbit(toe=7200 * 30)
    tow = 7200 * 30 - 1800
    s.ca(1, 3, o[3], tow)
    s.ca(1, 4, dict(page=(1 << 6) + 25, alpha0=77, beta3=-5, delta_tLS=99), tow + 6)
    s.ca(1, 2, o[2], tow + 12)
    s.ca(1, 1, o[1], tow + 18)
    o2 = ca_orbit(toe=7200 * 31)
    for k, sub in enumerate((1, 2, 3)):
        s.ca(1, sub, o2[sub], tow + 7200 + 6 * k)
    # 2: e = 0;  3: e at the field's maximum
    for ch, e_raw in ((2, 0), (3, 2 ** 32 - 1)):
        o = ca_orbit(e_raw=e_raw, toe=7200 * (40 + ch))
        for k, sub in enumerate((2, 1, 3)):
            s.ca(ch, sub, o[sub], 7200 * (40 + ch) + 600 + 6 * k, inverted=k & 1)
    # 4: IODC != IODE2, never mended;  5: the same, then mended
    o = ca_orbit(toe=7200 * 50, iod=17)
    o[2]["IODE2"] = 18
    for k, sub in enumerate((1, 2, 3, 4, 5)):
        s.ca(4, sub, o.get(sub, page18() if sub == 4 else {}), 7200 * 50 + 6 * k)
    o = ca_orbit(toe=7200 * 51, iod=200)
    o3 = dict(o[3], IODE3=201)
    s.ca(5, 1, o[1], 7200 * 51)
    s.ca(5, 2, o[2], 7200 * 51 + 6)
    s.ca(5, 3, o3, 7200 * 51 + 12)
    s.ca_parity(5, 0)
    s.ca_parity(5, 9)
    s.ca(5, 3, o[3], 7200 * 51 + 42)
    # 6: QZSS with page 18 (UTC stays)
    o = ca_orbit(toe=7200 * 60)
    for k, sub in enumerate((1, 2, 3, 4)):
        s.ca(6, sub, o.get(sub, page18()), 7200 * 60 + 900 + 6 * k)
    # 7 / 8: t - t_oe on both sides of +302400 / -302400 within the bits a snapshot adds
    o = ca_orbit(toe=7200 * 10)
    for k, sub in enumerate((1, 2, 3)):
        s.ca(7, sub, o[sub], 7200 * 10 + 302400 - 12 - 6 * (2 - k))
    o = ca_orbit(toe=7200 * 70)
    for k, sub in enumerate((1, 2, 3)):
        s.ca(8, sub, o[sub], 7200 * 70 - 302400 - 12 - 6 * (2 - k))
    # 9 / 10: the week wrap: t_oe at the start of the week and the TOW at its end, and the other way round
    o = ca_orbit(toe=0)
    for k, sub in enumerate((1, 2, 3)):
        s.ca(9, sub, o[sub], 604800 - 60 + 6 * k)
    o = ca_orbit(toe=604784)
    for k, sub in enumerate((3, 2, 1)):
        s.ca(10, sub, o[sub], 6 * k)
    return s, list(range(11))


def scenario_gal():
    s = Stream()
    for ch in range(5):
        s.bind(ch, 20 + ch, eph.E1B)
    week = 1290
    # ch 0 / sat 20: words 1..4 before the first word 5 (no t_oe / t_oc yet), then 5, then 1..4 again, 6, 0, 10, almanac and dummy words,
    # and frames that must leave everything untouched
    o = gal_orbit()
    for w in (1, 2, 3, 4):
        s.e1b(0, w, o[w])
    s.e1b(0, 6, dict(tow=5000))                                          # week_gst still 0: not applied to the TOW
    s.e1b(0, 5, word5(week, 200000), err=nav.ERR_CRC)
    s.e1b(0, 5, word5(week, 200000), err=nav.ERR_ALERT, alert=1)
    s.e1b(0, 2, o[2], err=nav.ERR_SLIP)
    s.e1b(0, 5, word5(week, 200000))
    for w in (4, 1, 3, 2):
        s.e1b(0, w, o[w], inverted=1)
    s.e1b(0, 6, dict(tow=200010))
    s.e1b(0, 0, dict(time=2, week=week, tow=200020))
    s.e1b(0, 0, dict(time=1, week=week + 5, tow=300000))
    s.e1b(0, 10, word10())
    for w in (7, 8, 9, 63, 17):
        s.e1b(0, w, {})
    s.e1b(0, 1, gal_orbit()[1], err=nav.ERR_CRC)
    # ch 1 / sat 21: word 5 first, an orbit with toes == 0, a word 5 with OOS (applied), IODN left unequal
    o = gal_orbit(toes_min=0)
    s.e1b(1, 5, word5(week, 300000))
    for w in (1, 2, 3, 4):
        s.e1b(1, w, o[w])
    s.e1b(1, 5, word5(week, 300030, e1bhs=1), err=nav.ERR_OOS)
    s.e1b(1, 5, word5(week, 300060, e1bdvs=1), err=nav.ERR_OOS)
    s.e1b(1, 3, dict(gal_orbit()[3], iodc=o[3]["iodc"] ^ 1))
    s.e1b(1, 10, word10())
    s.e1b(1, 0, dict(time=2, week=week, tow=300090))
    s.e1b(1, 6, dict(tow=300100))
    # ch 2 / sat 22: a week that rolls into the next (tow_gst beyond the week), toes beyond the week
    o = gal_orbit(toes_min=10081 + 30)
    s.e1b(2, 0, dict(time=2, week=week, tow=604790))
    for w in (2, 3, 4, 1):
        s.e1b(2, w, o[w])
    s.e1b(2, 5, word5(week, 604799))
    s.e1b(2, 6, dict(tow=604800 + 20))
    s.e1b(2, 10, word10())
    # ch 3 / sat 23: plain
    o = gal_orbit(toes_min=3000)
    s.e1b(3, 5, word5(week, 3000 * 60 + 1200))
    for w in (1, 2, 3, 4):
        s.e1b(3, w, o[w])
    s.e1b(3, 6, dict(tow=3000 * 60 + 1230))
    s.e1b(3, 0, dict(time=2, week=week, tow=3000 * 60 + 1260))
    s.e1b(3, 10, word10())
    # ch 4 / sat 24: never sees a week: no t_oe, IODN complete -> Valid with t_oe 0
    o = gal_orbit()
    for w in (1, 2, 3, 4, 10):
        s.e1b(4, w, o[w] if w != 10 else word10())
    # ch 0 rebound to sat 25 carrying its week_gst: words 1..4 alone give t_oe and t_oc
    s.bind(0, 25, eph.E1B)
    o = gal_orbit(toes_min=3400)
    for w in (1, 2, 3, 4):
        s.e1b(0, w, o[w])
    s.e1b(0, 6, dict(tow=3400 * 60 + 600))
    s.e1b(0, 10, word10())
    # ch 3 rebound to sat 26: only half an ephemeris
    s.bind(3, 26, eph.E1B)
    o = gal_orbit()
    s.e1b(3, 1, o[1])
    s.e1b(3, 2, o[2])
    return s, list(range(20, 27))


def snapshots(sats, kinds, final):
    """per satellite a spread of replicas, then the special ones"""
    out = []

    def add(sat, bits, bits_tow, ms, chips, cg, power):
        r = np.zeros((), eph.snap_dtype)
        r["sat"], r["bits"], r["bits_tow"], r["ms"], r["chips"], r["cg_phase"], r["power"] = sat, bits, bits_tow, ms, chips, cg, power
        out.append(r.reshape(1))

    for sat in sats:
        e1b = kinds[sat] == eph.E1B
        for k in range(16):
            bits = ri(0, 700 if e1b else 1200)
            add(sat, bits, bits, (0, 4)[k & 1] if e1b else ri(0, 21), ri(0, 4092 if e1b else 1023), ri(0, 64), float(rng.uniform(1.2e5, 4.5e6)))
        for k in range(3):                                              # the TOW delayed: bits_tow below 2500 and unequal
            add(sat, ri(0, 300), ri(300, 2499), 0 if e1b else ri(0, 20), ri(0, 1023), ri(0, 64), 2e5)
        add(sat, 100, 2500, 0, 5, 6, 3e5)                               # bits_tow at MAX_TOW_DELAY: not substituted
        add(sat, 100, 4000, 0, 5, 6, 3e5)
        for p in (99999.0, 1e5, 5e6, 5000001.0, 0.0, float("inf")):    # the power gate, both ends, on and beside the bound
            add(sat, 10, 10, 0, 1, 2, p)
        if e1b:
            add(sat, 10, 10, 1, 100, 3, 2e5)                            # bad ms
            add(sat, 10, 10, 0, 4092, 3, 2e5)                           # bad chips
            add(sat, 10, 10, 4, -1, 3, 2e5)
            add(sat, -5, -5, 0, 4091, 63, 2e5)                          # not bad: the bits test cannot fire
        else:
            add(sat, 10, 10, 25, 2000, 70, 2e5)                         # C/A: nothing is bad
    return np.concatenate(out)


def run_ref(exe, s, kinds_of, snaps):
    script = []
    for sat, kind in kinds_of.items():
        script.append("K %d %d" % (sat, REF_KIND[kind]))
    kind_of_ch = {}
    for op, ch, a, b in s.ev:
        if op == 0:
            script.append("S %d %d" % (ch, a))
            kind_of_ch[ch] = b
        else:
            r = s.frames[a][0]
            if kind_of_ch[ch] == eph.E1B:
                script.append("G %d %d %s" % (ch, int(r["err"]), bytes(r["data"][:30]).hex()))
            elif r["err"] == 0:
                script.append("C %d %s" % (ch, "".join("01"[b] for b in np.unpackbits(r["data"])[:300])))
            else:
                script.append("X %d %d" % (ch, int(r["err"])))
    for v in snaps:
        script.append("V %d %d %d %d %d %d %s" % (v["sat"], v["bits"], v["bits_tow"], v["ms"], v["chips"], v["cg_phase"], float(v["power"]).hex()))
    p = subprocess.run([exe], input=("\n".join(script) + "\n").encode(), stdout=subprocess.PIPE, check=True)
    E, V = [], []
    for line in p.stdout.decode().splitlines():
        f = line.split()
        if f and f[0] == "E":
            E.append(f[1:])
        elif f and f[0] == "V":
            V.append(f[1:])
    return E, V


EPH_INT = {"IODN", "IODC", "t_oc", "IODE2", "t_oe", "IODE3", "week", "tow", "sub", "tow_pg", "t_0G", "WN_0G"}
EPH_ORDER = ["IODN", "IODC", "t_oc", "t_gd", "a_f", "IODE2", "t_oe", "C_rs", "dn", "M_0", "C_uc", "e", "C_us", "sqrtA", "IODE3", "C_ic", "OMEGA_0", "C_is",
             "i_0", "C_rc", "omega", "OMEGA_dot", "IDOT", "alpha", "beta", "week", "tow", "sub", "tow_pg", "A_0G", "A_1G", "t_0G", "WN_0G"]


def parse_ephem(tok, kind, valid):
    e = np.zeros((), eph.ephem_dtype)
    k = 0
    for name in EPH_ORDER:
        n = int(np.prod(eph.ephem_dtype[name].shape)) if eph.ephem_dtype[name].shape else 1
        vals = [int(t) if name in EPH_INT else float.fromhex(t) for t in tok[k:k + n]]
        e[name] = vals if eph.ephem_dtype[name].shape else vals[0]
        k += n
    assert k == len(tok)
    e["kind"], e["valid"] = kind, valid
    return e


def records(s, E, kinds_of):
    """the reference's lines -> per frame the satellite's kg_ephem, the channel's Galileo state, the UTC fields and the note"""
    nf = len(s.frames)
    assert len(E) == nf
    out = dict(eph=np.zeros(nf, eph.ephem_dtype), chan=np.zeros((nf, 3), np.uint32), utc=np.zeros((nf, 3), np.int32), notes=np.zeros(nf, eph.note_dtype),
               err=np.zeros(nf, np.int32))
    sat_of, tow_bit = {}, {}
    for op, ch, a, b in s.ev:
        if op == 0:
            sat_of[ch] = a
            continue
        r, tok = s.frames[a][0], E[a]
        applied, tow_updated, err = int(tok[0]), int(tok[1]), int(tok[2])
        sat = sat_of[ch]
        bit_next = int(r["bit"]) + int(r["consumed"])
        if tow_updated:
            tow_bit[sat] = bit_next
        e = parse_ephem(tok[tok.index("|") + 1:], kinds_of[sat], int(tok[9]))
        e["tow_bit"] = tow_bit.get(sat, 0)
        out["eph"][a] = e
        out["chan"][a] = [int(tok[3]), int(tok[4]), int(tok[5])]
        out["utc"][a] = [int(tok[6]), int(tok[7]), int(tok[8])]
        n = out["notes"][a]
        n["applied"], n["tow_updated"], n["sub"], n["valid"], n["tow"], n["week"], n["bit_next"] = (applied, tow_updated, int(e["sub"]), int(e["valid"]),
                                                                                                    int(e["tow"]), int(e["week"]), bit_next)
        out["err"][a] = err
        assert err == int(r["err"]), ("the reference's err differs from the frame's", a, err, int(r["err"]))
    return out


def main():
    out, names = {}, []
    tally = dict(sub={}, word={}, valid_ca=0, valid_gal=0, invalid=0, inexact={}, sc2rad=0, flags={}, wrap_lo=0, wrap_hi=0, nsnap=0)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, make in (("ca", scenario_ca), ("gal", scenario_gal)):
            s, sats = make()
            kinds_of = {}
            for op, ch, a, b in s.ev:
                if op == 0:
                    kinds_of[a] = b
            E0, _ = run_ref(exe, s, kinds_of, [])
            rec = records(s, E0, kinds_of)
            final = {}
            sat_of = {}
            for op, ch, a, b in s.ev:
                if op == 0:
                    sat_of[ch] = a
                else:
                    final[sat_of[ch]] = rec["eph"][a]
            snaps = snapshots(sats, kinds_of, final)
            E, V = run_ref(exe, s, kinds_of, snaps)
            assert E == E0 and len(V) == len(snaps)
            svd = np.array([[float.fromhex(t) for t in v[1:8]] for v in V], np.float64)       # clock, correction, ct, t_k, x, y, z
            svi = np.array([[int(v[0]), int(v[8])] for v in V], np.int32)                     # flags, week
            names.append(name)
            out[name + "_ev"] = np.array(s.ev, np.int32)
            out[name + "_frames"] = np.concatenate(s.frames).view(np.uint8).reshape(-1, 64)
            out[name + "_eph"] = rec["eph"].view(np.uint8).reshape(-1, eph.ephem_dtype.itemsize)
            out[name + "_chan"], out[name + "_utc"] = rec["chan"], rec["utc"]
            out[name + "_notes"] = rec["notes"].view(np.uint8).reshape(-1, eph.note_dtype.itemsize)
            out[name + "_snaps"] = snaps.view(np.uint8).reshape(-1, eph.snap_dtype.itemsize)
            out[name + "_svd"], out[name + "_svi"] = svd, svi
            # ---- what the file holds
            sat_of = {}
            for op, ch, a, b in s.ev:
                if op == 0:
                    sat_of[ch] = a
                    continue
                r, n, e = s.frames[a][0], rec["notes"][a], rec["eph"][a]
                if not n["applied"]:
                    continue
                if kinds_of[sat_of[ch]] != eph.E1B:
                    tally["sub"][int(r["id"])] = tally["sub"].get(int(r["id"]), 0) + 1
                    continue
                wt = int(r["id"])
                tally["word"][wt] = tally["word"].get(wt, 0) + 1
                _, raw = eph.inav_fields(np.concatenate((np.unpackbits(r["data"][:15])[2:114], np.unpackbits(r["data"][15:30])[2:18])))

                def sg(v, nbits):
                    return v - (1 << nbits) if v >> (nbits - 1) else v
                exact = []                                              # (name, the reference's value, raw * 2^-n with the exact power)
                if wt == 1:
                    exact += [("e", e["e"], raw["e"] * 2.0 ** -33)]
                    tally["sc2rad"] += float(e["M_0"]) != sg(raw["M0"], 32) * 2.0 ** -31 * PI_EXACT
                elif wt == 2:
                    exact += [("idot", e["IDOT"], sg(raw["idot"], 14) * 2.0 ** -43 * SC2RAD)]
                elif wt == 3:
                    exact += [("OMGd", e["OMEGA_dot"], sg(raw["OMGd"], 24) * 2.0 ** -43 * SC2RAD), ("deln", e["dn"], sg(raw["deln"], 16) * 2.0 ** -43 * SC2RAD)]
                elif wt == 4:
                    exact += [("f1", e["a_f"][1], sg(raw["f1"], 21) * 2.0 ** -46)]
                elif wt == 5:
                    exact += [("tgd", e["t_gd"], sg(raw["bgd_e5b"], 10) * 2.0 ** -32)]
                elif wt == 10:
                    exact += [("A_0G", e["A_0G"], sg(raw["A_0G"], 16) * 2.0 ** -35)]
                for nm, got, ex in exact:
                    tally["inexact"][nm] = tally["inexact"].get(nm, 0) + (float(got) != float(ex))
            for sat in sats:
                v = int(final[sat]["valid"])
                if v and kinds_of[sat] == eph.E1B:
                    tally["valid_gal"] += 1
                elif v:
                    tally["valid_ca"] += 1
                else:
                    tally["invalid"] += 1
            for v, (fl, _), d in zip(snaps, svi, svd):
                for b in (1, 2, 4, 8, 16):
                    tally["flags"][b] = tally["flags"].get(b, 0) + bool(fl & b)
                if fl & (1 | 2 | 8):
                    continue
                tally["nsnap"] += 1
                t_tx = d[2] / CONST[(GPSH, "C")]
                raw_tk = t_tx - float(final[int(v["sat"])]["t_oe"])
                tally["wrap_hi"] += raw_tk > 302400
                tally["wrap_lo"] += raw_tk < -302400
            print("eph_ref.npz: %-4s %3d frames, %3d applied, %3d snapshots" % (name, len(s.frames), int(rec["notes"]["applied"].sum()), len(snaps)))
    print(tally)
    assert all(tally["sub"].get(k, 0) >= 3 for k in (1, 2, 3, 4)), tally["sub"]
    assert all(tally["word"].get(k, 0) >= 3 for k in (0, 1, 2, 3, 4, 5, 6, 10)), tally["word"]
    assert tally["valid_ca"] >= 4 and tally["valid_gal"] >= 3 and tally["invalid"] >= 2, tally
    assert all(tally["inexact"].get(k, 0) >= 5 for k in ("e", "tgd", "OMGd", "deln", "idot", "f1", "A_0G")), tally["inexact"]
    assert tally["sc2rad"] >= 3, tally
    assert tally["nsnap"] >= 200 and tally["flags"][4] >= 5 and tally["flags"][2] >= 5 and tally["flags"][8] >= 3 and tally["flags"][16] >= 5, tally
    assert tally["flags"][1] >= 5 and tally["wrap_lo"] >= 5 and tally["wrap_hi"] >= 5, tally
    out["names"] = np.array(names)
    path = os.path.join(GOLD, "eph_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
