// kg_eph.h -- the arithmetic of ephemeris decode and of satellite position and clock: what reads a validated frame into numbers
// (EPHEM::Subframe, Subframe1..4, LoadPage18, Valid, gps/ephemeris.cpp:51-110, :218-252; decode_page_e1b and decode_word0..6 / 10,
// gps/GNSS-SDRLIB/sdrnav_gal.cpp:28-286, :327-359, with EPHEM::PageN / Page0..6, ephemeris.cpp:256-370) and what the solver asks of
// the result (SNAPSHOT::GetClock, gps/solve.cpp:168-244; EPHEM::GetClockCorrection, TimeOfEphemerisAge, EccentricAnomaly, GetXYZ,
// ephemeris.cpp:114-207; the per-replica body of LoadFromReplicas, solve.cpp:319-361), for the device (kg_eph.hip) and, compiled by
// a host compiler, for tools/eph_host_driver.cpp -- as kg_nav.h is.
//
// Every double is formed by the reference's operations in the reference's order; build without floating-point contraction.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KG_EPH_FN __host__ __device__ static inline
#else
#define KG_EPH_FN static inline
#endif

namespace kg_eph_cf {

enum { KIND_NAVSTAR = 0, KIND_CA = 1, KIND_E1B = 2, MAX_SATS = 64,
       NAV_ERR_OOS = 4,                                 // GPS_ERR_OOS, gps/gps.h:190
       SV_NOT_VALID = 1, SV_POWER = 2, SV_TOW_DELAYED = 4, SV_BAD = 8, SV_TOO_OLD = 16,
       MAX_TOW_DELAY = 5 * 500,                         // solve.cpp:221
       E1B_CODE_PERIOD = 4, E1B_CODELEN = 4092 };       // gps.h:54 with kiwi.config's E1B_CODELEN

// rtklib.h:421-444 and sdrnav_gal.cpp:16-18 write 2^-n as DECIMAL text; five of them are not powers of two as doubles
constexpr double P2_5 = 0x1p-5, P2_19 = 0x1p-19, P2_21 = 0x1p-21, P2_29 = 0x1p-29, P2_30 = 0x1p-30, P2_31 = 0x1p-31, P2_34 = 0x1p-34,
                 P2_59 = 0x1p-59,
                 P2_32 = 0x1.fffffffffffffp-33,         // 2.328306436538696E-10
                 P2_33 = 0x1.fffffffffffffp-34,         // 1.164153218269348E-10
                 P2_35 = 0x1.fffffffffffffp-36,         // 2.910383045673370E-11
                 P2_43 = 0x1.ffffffffffffep-44,         // 1.136868377216160E-13
                 P2_46 = 0x1.ffffffffffffep-47;         // 1.421085471520200E-14
// gps.h:87's PI and rtklib.h:61's SC2RAD are the same text, 3.1415926535898: one double for C/A and Galileo angles, 16 ulp above pi
constexpr double PI = 0x1.921fb54442d28p+1, SC2RAD = 0x1.921fb54442d28p+1;
constexpr double MU = 0x1.6a866935b5p+48,               // 3.986005e14
                 OMEGA_E = 0x1.31da7d7cb8d5bp-14,       // 7.2921151467e-5
                 C_LIGHT = 0x1.1de784ap+28,             // 2.99792458e8
                 F_REL = -0x1.e87deae177a99p-32,        // -4.442807633e-10
                 CPS = 0x1.f383p+19;                    // 1.023e6

struct ephem {                            // == kg_ephem (include/kiwigpu.h): the data members of EPHEM the decode writes
    uint32_t IODN[4];
    uint32_t IODC, t_oc;
    double t_gd, a_f[3];
    uint32_t IODE2, t_oe;
    double C_rs, dn, M_0, C_uc, e, C_us, sqrtA;
    uint32_t IODE3, kind;
    double C_ic, OMEGA_0, C_is, i_0, C_rc, omega, OMEGA_dot, IDOT;
    double alpha[4], beta[4];
    uint32_t week, tow, sub, tow_pg;
    double A_0G, A_1G;
    uint32_t t_0G, WN_0G;
    int32_t valid, pad_;
    uint64_t tow_bit;
};

struct chanst { int32_t sat, kind; uint32_t week_gst, toes, toc_gst, pad_; };           // sat < 0: not bound.  CHANNEL::nav.sdreph's three
struct utc { int32_t delta_tLS, delta_tLSF, tLS_valid, pad_; };                         // gps.delta_tLS, delta_tLSF, tLS_valid

struct note {                             // == kg_eph_note
    int32_t applied, tow_updated, sub, valid;
    uint32_t tow, week;
    uint64_t bit_next;
};

struct upd {                              // the field kernel's answer for one frame: raw fields scaled, no state read
    int32_t apply, id;                    // id: bin(buf + 49, 3) (C/A), the word type (E1B)
    uint32_t tow, u[3];
    double d[8];
};

struct snap { int32_t sat, bits, bits_tow, ms, chips, cg_phase; float power; };         // == kg_eph_snap
struct sv { double x, y, z, ct, t_k; int32_t week, flags; };                            // == kg_eph_pos

// ---- rtkcmn.cpp:598-610, sdrnav.cpp:94-104 on the 30 bytes of a page
KG_EPH_FN uint32_t getbitu(const uint8_t *b, int pos, int len)
{
    uint32_t v = 0;
    for (int i = pos; i < pos + len; i++) v = (v << 1) + ((b[i >> 3] >> (7 - (i & 7))) & 1u);
    return v;
}
KG_EPH_FN int32_t getbits(const uint8_t *b, int pos, int len)
{
    const uint32_t v = getbitu(b, pos, len);
    if (len <= 0 || 32 <= len || !(v & (1u << (len - 1)))) return (int32_t) v;
    return (int32_t) (v | (~0u << len));
}
KG_EPH_FN uint32_t getbitu2(const uint8_t *b, int p1, int l1, int p2, int l2) { return (getbitu(b, p1, l1) << l2) + getbitu(b, p2, l2); }
KG_EPH_FN int32_t getbits2(const uint8_t *b, int p1, int l1, int p2, int l2)
{
    if (getbitu(b, p1, 1)) return (int32_t) (((uint32_t) getbits(b, p1, l1) << l2) + getbitu(b, p2, l2));
    return (int32_t) getbitu2(b, p1, l1, p2, l2);
}

// ---- ephemeris.cpp:40-47: PACK left-aligns up to four bytes; u(n) / s(n) take the top n bits
KG_EPH_FN uint32_t pack(uint32_t a, uint32_t b = 0, uint32_t c = 0, uint32_t d = 0) { return (a << 24) | (b << 16) | (c << 8) | d; }
KG_EPH_FN uint32_t pk_u(uint32_t v, int n) { return v >> (32 - n); }
KG_EPH_FN int32_t pk_s(uint32_t v, int n) { return (int32_t) v >> (32 - n); }

// time2gpst(gst2time(week_gst, sec)) for a whole sec >= 0 (rtkcmn.cpp:1261-1284): epoch2time(gst0) lies 1024 weeks behind
// epoch2time(gpst0).  The reference forms 86400 * 7 * week in int, which holds up to week_gst 2526 (the year 2048); so does this.
KG_EPH_FN uint32_t gst2gpst(uint32_t week_gst, uint32_t sec, uint32_t *week)
{
    const int64_t t = (int64_t) 604800 * (1024 + (int64_t) week_gst) + (int64_t) sec;
    const int64_t w = t / 604800;
    if (week) *week = (uint32_t) w;
    return (uint32_t) (t - w * 604800);
}

// ---- the field kernel's work: one frame's payload -> upd
// EPHEM::Subframe's unpacking (nav[j]: the 8 bits at 30 (j / 3) + 8 (j % 3) of the corrected 300) and Subframe1..4 / LoadPage18
KG_EPH_FN void fields_ca(const uint8_t *data, upd &o)
{
    uint32_t nav[30];
    for (int j = 0; j < 30; j++) nav[j] = getbitu(data, 30 * (j / 3) + 8 * (j % 3), 8);
    o.apply = 1;
    o.id = (int32_t) getbitu(data, 49, 3);
    o.tow = pk_u(pack(nav[3], nav[4], nav[5]), 17) * 6;
    for (int k = 0; k < 3; k++) o.u[k] = 0;
    for (int k = 0; k < 8; k++) o.d[k] = 0.0;
    switch (o.id) {
    case 1:
        o.u[0] = pk_u(pack(nav[6], nav[7]), 10);                                // week
        o.d[0] = 0x1p-31 * pk_s(pack(nav[20]), 8);                              // t_gd
        o.u[1] = pk_u(pack(nav[21]), 8);                                        // IODC
        o.u[2] = (1u << 4) * pk_u(pack(nav[22], nav[23]), 16);                  // t_oc
        o.d[3] = 0x1p-55 * pk_s(pack(nav[24]), 8);                              // a_f[2]
        o.d[2] = 0x1p-43 * pk_s(pack(nav[25], nav[26]), 16);                    // a_f[1]
        o.d[1] = 0x1p-31 * pk_s(pack(nav[27], nav[28], nav[29]), 22);           // a_f[0]
        break;
    case 2:
        o.u[0] = pk_u(pack(nav[6]), 8);                                         // IODE2
        o.d[0] = 0x1p-5 * pk_s(pack(nav[7], nav[8]), 16);                       // C_rs
        o.d[1] = 0x1p-43 * pk_s(pack(nav[9], nav[10]), 16) * PI;                // dn
        o.d[2] = 0x1p-31 * pk_s(pack(nav[11], nav[12], nav[13], nav[14]), 32) * PI;     // M_0
        o.d[3] = 0x1p-29 * pk_s(pack(nav[15], nav[16]), 16);                    // C_uc
        o.d[4] = 0x1p-33 * pk_u(pack(nav[17], nav[18], nav[19], nav[20]), 32);  // e
        o.d[5] = 0x1p-29 * pk_s(pack(nav[21], nav[22]), 16);                    // C_us
        o.d[6] = 0x1p-19 * pk_u(pack(nav[23], nav[24], nav[25], nav[26]), 32);  // sqrtA
        o.u[1] = (1u << 4) * pk_u(pack(nav[27], nav[28]), 16);                  // t_oe
        break;
    case 3:
        o.d[0] = 0x1p-29 * pk_s(pack(nav[6], nav[7]), 16);                      // C_ic
        o.d[1] = 0x1p-31 * pk_s(pack(nav[8], nav[9], nav[10], nav[11]), 32) * PI;       // OMEGA_0
        o.d[2] = 0x1p-29 * pk_s(pack(nav[12], nav[13]), 16);                    // C_is
        o.d[3] = 0x1p-31 * pk_s(pack(nav[14], nav[15], nav[16], nav[17]), 32) * PI;     // i_0
        o.d[4] = 0x1p-5 * pk_s(pack(nav[18], nav[19]), 16);                     // C_rc
        o.d[5] = 0x1p-31 * pk_s(pack(nav[20], nav[21], nav[22], nav[23]), 32) * PI;     // omega
        o.d[6] = 0x1p-43 * pk_s(pack(nav[24], nav[25], nav[26]), 24) * PI;      // OMEGA_dot
        o.u[0] = pk_u(pack(nav[27]), 8);                                        // IODE3
        o.d[7] = 0x1p-43 * pk_s(pack(nav[28], nav[29]), 14) * PI;               // IDOT
        break;
    case 4:
        o.u[0] = pk_u(pack(nav[6]), 8) == ((1u << 6) + 56);                     // page 18
        o.d[0] = 0x1p-30 * pk_s(pack(nav[7]), 8);
        o.d[1] = 0x1p-27 * pk_s(pack(nav[8]), 8);
        o.d[2] = 0x1p-24 * pk_s(pack(nav[9]), 8);
        o.d[3] = 0x1p-24 * pk_s(pack(nav[10]), 8);
        o.d[4] = 0x1p+11 * pk_s(pack(nav[11]), 8);
        o.d[5] = 0x1p+14 * pk_s(pack(nav[12]), 8);
        o.d[6] = 0x1p+16 * pk_s(pack(nav[13]), 8);
        o.d[7] = 0x1p+16 * pk_s(pack(nav[14]), 8);
        o.u[1] = (uint32_t) pk_s(pack(nav[24]), 8);                             // delta_tLS
        o.u[2] = (uint32_t) pk_s(pack(nav[27]), 8);                             // delta_tLSF
        break;
    default:
        break;
    }
}

// decode_page_e1b's id and decode_word0..6 / 10 up to where they read the channel: b = dec_e1b1[15] then dec_e1b2[15]
KG_EPH_FN void fields_e1b(const uint8_t *b, upd &o)
{
    enum { O1 = 2, O2 = 122 };                          // OFFSET1, OFFSET2
    o.apply = 1;
    o.id = (int32_t) getbitu(b, 2, 6);
    o.tow = 0;
    for (int k = 0; k < 3; k++) o.u[k] = 0;
    for (int k = 0; k < 8; k++) o.d[k] = 0.0;
    switch (o.id) {
    case 0:
        o.u[2] = getbitu(b, O1 + 6, 2) == 2;
        o.u[0] = getbitu(b, O1 + 96, 12);                                       // week_gst
        o.u[1] = getbitu2(b, O1 + 108, 4, O2 + 0, 16) + 2;                      // tow_gst
        break;
    case 1:
        o.u[0] = getbitu(b, O1 + 6, 10);                                        // iodc
        o.u[1] = getbitu(b, O1 + 16, 14) * 60;                                  // toes
        o.d[0] = getbits(b, O1 + 30, 32) * P2_31 * SC2RAD;                      // M0
        o.d[1] = getbitu(b, O1 + 62, 32) * P2_33;                               // e
        o.d[2] = getbitu2(b, O1 + 94, 18, O2 + 0, 14) * P2_19;                  // sqrtA
        break;
    case 2:
        o.u[0] = getbitu(b, O1 + 6, 10);
        o.d[0] = getbits(b, O1 + 16, 32) * P2_31 * SC2RAD;                      // OMG0
        o.d[1] = getbits(b, O1 + 48, 32) * P2_31 * SC2RAD;                      // i0
        o.d[2] = getbits(b, O1 + 80, 32) * P2_31 * SC2RAD;                      // omg
        o.d[3] = getbits(b, O2 + 0, 14) * P2_43 * SC2RAD;                       // idot
        break;
    case 3:
        o.u[0] = getbitu(b, O1 + 6, 10);
        o.d[0] = getbits(b, O1 + 16, 24) * P2_43 * SC2RAD;                      // OMGd
        o.d[1] = getbits(b, O1 + 40, 16) * P2_43 * SC2RAD;                      // deln
        o.d[2] = getbits(b, O1 + 56, 16) * P2_29;                               // cuc
        o.d[3] = getbits(b, O1 + 72, 16) * P2_29;                               // cus
        o.d[4] = getbits(b, O1 + 88, 16) * P2_5;                                // crc
        o.d[5] = getbits2(b, O1 + 104, 8, O2 + 0, 8) * P2_5;                    // crs
        break;
    case 4:
        o.u[0] = getbitu(b, O1 + 6, 10);
        o.d[0] = getbits(b, O1 + 22, 16) * P2_29;                               // cic
        o.d[1] = getbits(b, O1 + 38, 16) * P2_29;                               // cis
        o.u[1] = getbitu(b, O1 + 54, 14) * 60;                                  // toc_gst
        o.d[2] = getbits(b, O1 + 68, 31) * P2_34;                               // f0
        o.d[3] = getbits2(b, O1 + 99, 13, O2 + 0, 8) * P2_46;                   // f1
        o.d[4] = getbits(b, O2 + 8, 6) * P2_59;                                 // f2
        break;
    case 5:
        o.d[0] = getbits(b, O1 + 57, 10) * P2_32;                               // tgd[1], BGD E5b/E1
        o.u[0] = getbitu(b, O1 + 73, 12);                                       // week_gst
        o.u[1] = getbitu(b, O1 + 85, 20) + 2;                                   // tow_gst
        break;
    case 6:
        o.u[1] = getbitu2(b, O1 + 105, 7, O2 + 0, 13) + 2;
        break;
    case 10:
        o.d[0] = getbits(b, O1 + 86, 16) * P2_35;                               // A_0G
        o.d[1] = getbits2(b, O1 + 102, 10, O2 + 0, 2) * P2_30 * P2_21;          // A_1G
        o.u[0] = getbitu(b, O2 + 2, 8) * 3600;                                  // t_0G
        o.u[1] = getbitu(b, O2 + 10, 6);                                        // WN_0G
        break;
    default:
        break;
    }
}

// which frames reach Ephemeris[sat].Subframe / decode_page_e1b: C/A err == 0 (channel.cpp:824-825); E1B err == 0 or GPS_ERR_OOS, which
// decode_word5 raises after Page5 has been applied (channel.cpp:756-762, sdrnav_gal.cpp:483-485, :196-204)
KG_EPH_FN void fields(int32_t kind, int32_t err, const uint8_t *data, upd &o)
{
    if (kind == KIND_E1B) {
        if (err == 0 || err == NAV_ERR_OOS) { fields_e1b(data, o); return; }
    } else if (err == 0) {
        fields_ca(data, o);
        return;
    }
    o.apply = 0; o.id = 0; o.tow = 0;
    for (int k = 0; k < 3; k++) o.u[k] = 0;
    for (int k = 0; k < 8; k++) o.d[k] = 0.0;
}

KG_EPH_FN int32_t valid(const ephem &e)                 // EPHEM::Valid
{
    return e.kind == KIND_E1B ? (e.IODN[0] != 0 && e.IODN[0] == e.IODN[1] && e.IODN[0] == e.IODN[2] && e.IODN[0] == e.IODN[3])
                              : (e.IODC != 0 && e.IODC == e.IODE2 && e.IODC == e.IODE3);
}

// ---- the walk kernel's work: one frame's fields applied to the channel's satellite -> nav.tow_updated; *leap: page 18 of a Navstar
KG_EPH_FN int32_t apply(ephem &e, chanst &c, const upd &o, utc *leap, int32_t *has_leap)
{
    int32_t tow_updated = 0;
    if (c.kind != KIND_E1B) {                           // EPHEM::Subframe
        e.sub = e.tow_pg = (uint32_t) o.id;
        e.tow = o.tow;
        tow_updated = 1;                                // bits_tow = holding - subframe_bits, channel.cpp:827
        switch (o.id) {
        case 1:
            e.week = o.u[0]; e.t_gd = o.d[0]; e.IODC = o.u[1]; e.t_oc = o.u[2];
            e.a_f[2] = o.d[3]; e.a_f[1] = o.d[2]; e.a_f[0] = o.d[1];
            break;
        case 2:
            e.IODE2 = o.u[0]; e.C_rs = o.d[0]; e.dn = o.d[1]; e.M_0 = o.d[2]; e.C_uc = o.d[3]; e.e = o.d[4]; e.C_us = o.d[5];
            e.sqrtA = o.d[6]; e.t_oe = o.u[1];
            break;
        case 3:
            e.C_ic = o.d[0]; e.OMEGA_0 = o.d[1]; e.C_is = o.d[2]; e.i_0 = o.d[3]; e.C_rc = o.d[4]; e.omega = o.d[5];
            e.OMEGA_dot = o.d[6]; e.IODE3 = o.u[0]; e.IDOT = o.d[7];
            break;
        case 4:
            if (o.u[0]) {                               // LoadPage18
                for (int k = 0; k < 4; k++) { e.alpha[k] = o.d[k]; e.beta[k] = o.d[4 + k]; }
                if (c.kind == KIND_NAVSTAR) {
                    leap->delta_tLS = (int32_t) o.u[1]; leap->delta_tLSF = (int32_t) o.u[2]; leap->tLS_valid = 1;
                    *has_leap = 1;
                }
            }
            break;
        default:
            break;
        }
        return tow_updated;
    }
    uint32_t wk = 0;
    e.sub = o.id >= 7 ? 999u : (uint32_t) o.id;         // PageN
    switch (o.id) {
    case 0:
        if (!o.u[2]) break;                             // "E1B word0 time field != 2"
        c.week_gst = o.u[0];
        e.tow = gst2gpst(c.week_gst, o.u[1], &wk); e.week = wk; e.tow_pg = 0;
        tow_updated = 1;
        break;
    case 1:
        c.toes = o.u[1];
        e.IODN[0] = o.u[0]; e.M_0 = o.d[0]; e.e = o.d[1]; e.sqrtA = o.d[2];
        if (c.week_gst != 0) {
            const uint32_t toe = gst2gpst(c.week_gst, c.toes, nullptr);
            if (toe != 0) e.t_oe = toe;
        }
        break;
    case 2:
        e.IODN[1] = o.u[0]; e.OMEGA_0 = o.d[0]; e.i_0 = o.d[1]; e.omega = o.d[2]; e.IDOT = o.d[3];
        break;
    case 3:
        e.IODN[2] = o.u[0]; e.OMEGA_dot = o.d[0]; e.dn = o.d[1]; e.C_uc = o.d[2]; e.C_us = o.d[3]; e.C_rc = o.d[4]; e.C_rs = o.d[5];
        break;
    case 4:
        c.toc_gst = o.u[1];
        e.IODN[3] = o.u[0]; e.C_ic = o.d[0]; e.C_is = o.d[1]; e.a_f[0] = o.d[2]; e.a_f[1] = o.d[3]; e.a_f[2] = o.d[4];
        if (c.week_gst != 0) {
            const uint32_t toc = gst2gpst(c.week_gst, c.toc_gst, nullptr);
            if (toc != 0) e.t_oc = toc;
        }
        break;
    case 5: {
        c.week_gst = o.u[0];
        e.tow = gst2gpst(c.week_gst, o.u[1], &wk); e.week = wk; e.tow_pg = 5;
        tow_updated = 1;
        e.t_gd = o.d[0];
        const uint32_t toc = c.toc_gst != 0 ? gst2gpst(c.week_gst, c.toc_gst, nullptr) : 0u;
        const uint32_t toe = c.toes != 0 ? gst2gpst(c.week_gst, c.toes, nullptr) : 0u;
        if (toc != 0) e.t_oc = toc;
        if (toe != 0) e.t_oe = toe;
        break;
    }
    case 6:
        if (c.week_gst != 0) {
            e.tow = gst2gpst(c.week_gst, o.u[1], &wk); e.week = wk; e.tow_pg = 6;
            tow_updated = 1;
        }
        break;
    case 10:
        e.A_0G = o.d[0]; e.A_1G = o.d[1]; e.t_0G = o.u[0]; e.WN_0G = o.u[1];
        break;
    default:
        break;
    }
    return tow_updated;
}

// one frame of a channel: its fields applied (or not), the note written
KG_EPH_FN void step(ephem *slots, chanst &c, const upd &o, uint64_t bit_next, note *n, utc *leap, int32_t *has_leap)
{
    n->applied = 0; n->tow_updated = 0; n->sub = 0; n->valid = 0; n->tow = 0; n->week = 0; n->bit_next = bit_next;
    if (c.sat < 0) return;
    ephem &e = slots[c.sat];
    if (o.apply) {
        n->applied = 1;
        n->tow_updated = apply(e, c, o, leap, has_leap);
        e.valid = valid(e);
        if (n->tow_updated) e.tow_bit = bit_next;
    }
    n->sub = (int32_t) e.sub; n->valid = e.valid; n->tow = e.tow; n->week = e.week;
}

// ---- position and clock
KG_EPH_FN double time_from_epoch(double t, double t_ref)
{
    t -= t_ref;
    if (t > 302400) t -= 604800;
    else if (t < -302400) t += 604800;
    return t;
}

KG_EPH_FN double ecc_anomaly(const ephem &e, double t_k)
{
    const double A = e.sqrtA * e.sqrtA;
    const double n_0 = sqrt(MU / (A * A * A));
    const double n = n_0 + e.dn;
    const double M_k = e.M_0 + n * t_k;
    double E_k = M_k;
    for (int i = 0; i < 10000; i++) {
        const double temp = E_k;
        E_k = M_k + e.e * sin(E_k);
        if (fabs(E_k - temp) < 1e-10) break;
    }
    return E_k;
}

KG_EPH_FN void get_xyz(const ephem &e, double *x, double *y, double *z, double t)
{
    const double t_k = time_from_epoch(t, e.t_oe);
    const double E_k = ecc_anomaly(e, t_k);
    const double v_k = atan2(sqrt(1 - e.e * e.e) * sin(E_k), cos(E_k) - e.e);
    const double AOL = v_k + e.omega;
    const double s2 = sin(2 * AOL), c2 = cos(2 * AOL);
    const double du_k = e.C_us * s2 + e.C_uc * c2;
    const double dr_k = e.C_rs * s2 + e.C_rc * c2;
    const double di_k = e.C_is * s2 + e.C_ic * c2;
    const double u_k = AOL + du_k;
    const double r_k = (e.sqrtA * e.sqrtA) * (1 - e.e * cos(E_k)) + dr_k;
    const double i_k = e.i_0 + di_k + e.IDOT * t_k;
    const double x_kp = r_k * cos(u_k);
    const double y_kp = r_k * sin(u_k);
    const double OMEGA_k = e.OMEGA_0 + (e.OMEGA_dot - OMEGA_E) * t_k - OMEGA_E * e.t_oe;
    const double so = sin(OMEGA_k), co = cos(OMEGA_k), ci = cos(i_k);
    *x = x_kp * co - y_kp * ci * so;
    *y = x_kp * so + y_kp * ci * co;
    *z = y_kp * sin(i_k);
}

KG_EPH_FN double clock_correction(const ephem &e, double t)
{
    const double t_k = time_from_epoch(t, e.t_oe);
    const double E_k = ecc_anomaly(e, t_k);
    const double t_R = F_REL * e.e * e.sqrtA * sin(E_k);
    t = time_from_epoch(t, e.t_oc);
    return e.a_f[0] + e.a_f[1] * t + e.a_f[2] * (t * t) + t_R - e.t_gd;          // pow(t, 1) is t; pow(t, 2) within an ulp of t * t
}

// SNAPSHOT::GetClock: of its "bad" tests only ms and chips can fire, and only for E1B (the others join two exclusive
// comparisons with &&); *flags gains SV_BAD (-> NaN) or SV_TOW_DELAYED
KG_EPH_FN double get_clock(const ephem &e, const snap &s, int32_t *flags)
{
    const bool isE1B = e.kind == KIND_E1B;
    if (isE1B && ((s.ms != 0 && s.ms != E1B_CODE_PERIOD) || s.chips < 0 || s.chips > E1B_CODELEN - 1)) {
        *flags |= SV_BAD;
        return NAN;
    }
    int32_t bits = s.bits;
    if (bits != s.bits_tow && s.bits_tow < MAX_TOW_DELAY) {
        bits = s.bits_tow;
        *flags |= SV_TOW_DELAYED;
    }
    return isE1B ? (e.tow + bits / 250.0 + s.ms * 1e-3 + s.chips / CPS + 0.25 / CPS + s.cg_phase * 0x1p-6 / CPS)
                 : (e.tow + bits / 50.0 + s.ms * 1e-3 + s.chips / CPS + s.cg_phase * 0x1p-6 / CPS);
}

// LoadAtomic's Valid() gate, then the body of LoadFromReplicas for one replica.  A snapshot refused by the gate or by the power
// test has only its flags written.  A bad clock is NaN in the reference and runs through (`t_tx == NAN` is never true): every
// value comes out NaN, here without the 10000 turns of the Kepler loop that NaN costs there.
KG_EPH_FN void sv_one(const ephem *slots, const snap &s, sv *out)
{
    if (s.sat < 0 || s.sat >= MAX_SATS || !slots[s.sat].valid) { out->flags = SV_NOT_VALID; return; }
    const double weight = s.power;
    if (weight < 1e5 || weight > 5e6) { out->flags = SV_POWER; return; }
    const ephem &e = slots[s.sat];
    int32_t flags = 0;
    double t_tx = get_clock(e, s, &flags);
    double x, y, z, t_k;
    if (flags & SV_BAD) {
        x = y = z = t_k = t_tx;
    } else {
        t_tx -= clock_correction(e, t_tx);
        t_k = time_from_epoch(t_tx, e.t_oe);            // TimeOfEphemerisAge
        if (fabs(t_k) / 60 / 60 >= 4) flags |= SV_TOO_OLD;                               // UMS(..).u >= 4
        get_xyz(e, &x, &y, &z, t_tx);
    }
    out->x = x; out->y = y; out->z = z; out->ct = C_LIGHT * t_tx; out->t_k = t_k;
    out->week = (int32_t) e.week; out->flags = flags;
}

// the 18-bit replica word of kg_trk_get_clocks, {~cg_phase[31], cg_phase[30:26], chips[9:0], chips[11:10]} (kg_trk.h replica()), is
// what LoadAtomic reads as dn[-1] (its upper 16 bits) and dn[0] (the two below): solve.cpp:77-79
KG_EPH_FN void replica_split(uint32_t word, int32_t *chips, int32_t *cg_phase)
{
    const uint32_t dn0 = word & 3, dn1 = (word >> 2) & 0xFFFF;
    *chips = (int32_t) (((dn0 & 0x3) << 10) | (dn1 & 0x3FF));
    *cg_phase = (int32_t) (dn1 >> 10);
}

}  // namespace kg_eph_cf
