// ref_eph_main.cpp -- the harness tools/make_ref_eph_golden.py compiles around text CUT from the reference tree at build time (never
// committed): ephemeris decode (C/A subframes, Galileo I/NAV words) and satellite position and clock, run on scripted frames and
// snapshots, the whole EPHEM printed after every frame.
//
//   cut (the EPH_CUT_* macros name the files the generator writes):
//     gps/gps.h              CPS .. E1B_BPS (:46-55), PI .. F (:87-94), GPS_ERR_* (:187-191), UMS (:289-296)
//     gps/gps.cpp            bin (:32-36)
//     gps/ephemeris.h        class EPHEM (:23-82), compiled with `class` read as `struct` so that the harness can print the members
//     gps/ephemeris.cpp      TimeFromEpoch, PACK (:31-47), Subframe1..4, LoadPage18 (:51-110), TimeOfEphemerisAge .. GetClockCorrection
//                            (:114-207), Init, Valid, Subframe (:211-252), PageN, Page0..6 (:256-370)
//     gps/solve.cpp          SNAPSHOT (:42-52), SNAPSHOT::GetClock (:168-244)
//     GNSS-SDRLIB/rtklib.h   SC2RAD (:61), P2_* (:421-444), gtime_t (:464-467), eph_t (:525-544)
//     GNSS-SDRLIB/rtkcmn.cpp gpst0, gst0 (:125-126), getbitu, getbits (:598-610), epoch2time (:1201-1215), time2gpst (:1261-1269),
//                            gst2time (:1276-1284)
//     GNSS-SDRLIB/sdrnav.cpp getbitu2, getbits2 (:94-104)
//     GNSS-SDRLIB/sdrnav_gal.cpp   P2_34 .. OFFSET2 (:16-20), decode_word1 .. decode_word0 (:28-286), decode_page_e1b (:327-359)
//   restated here and pinned by text in the generator: the members of sdreph_t and sdrnav_t the cut text names (gnss_sdrlib.h), ON,
//     L1_CODELEN / E1B_CODELEN / MAX_NAV_BITS (kiwi.config), is_Navstar / is_E1B and the sat_e order (gps.h:98, :118-121), MAX_SATS,
//     CHANNEL::Start's two statements (channel.cpp:274-278), ParityCheck's call sites (channel.cpp:751-762, :824-827), E1B_subframe's
//     `if (!err)` hand-over to decode_page_e1b (sdrnav_gal.cpp:483-485), LoadAtomic's Valid gate (solve.cpp:71) and the per-replica
//     body of LoadFromReplicas (solve.cpp:327-360).
//
// script (stdin):
//   K <sat> <type>                 Sats[sat].type = Navstar (0) / QZSS (2) / E1B (3)
//   S <ch> <sat>                   CHANNEL::Start: nav.sat = sat, Ephemeris[sat].Init(sat)
//   C <ch> <300 bits>              a C/A subframe that passed L1_parity -> Ephemeris[sat].Subframe
//   X <ch> <err>                   a frame that does not reach the decode (C/A parity): the state printed as it is
//   G <ch> <err> <60 hex digits>   dec_e1b1, dec_e1b2 and the err kg_nav reports: 0 / GPS_ERR_OOS reach decode_page_e1b
//   V <sat> <bits> <bits_tow> <ms> <chips> <cg_phase> <power as %a>    one replica
// output: per frame "E <applied> <tow_updated> <err out> <week_gst> <toes> <toc_gst> <delta_tLS> <delta_tLSF> <tLS_valid> <valid> | EPHEM"
// (integers %u, doubles %a, in kg_ephem's order); per replica "V <flags> <clock> <correction> <ct> <t_k> <x> <y> <z> <week>".
#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <iostream>
#include <string>

typedef unsigned int u4_t;
typedef unsigned char u1_t;
#define L1_CODELEN 1023
#define E1B_CODELEN 4092
#define MAX_NAV_BITS 128
#define MAX_SATS 64
#define ON 1
#define trace(...) ((void) 0)
#define lprintf(...) ((void) 0)
#define PRN(s) ""
static u4_t timer_ms() { return 0; }

#include EPH_CUT_GPS_RATES
#include EPH_CUT_GPS_CONST
#include EPH_CUT_GPSERR
#include EPH_CUT_UMS
#include EPH_CUT_BIN

typedef enum { Navstar, SBAS, QZSS, E1B } sat_e;
static struct { int prn; sat_e type; } Sats[MAX_SATS];
#define is_Navstar(sat) (Sats[sat].type == Navstar)
#define is_E1B(sat) (Sats[sat].type == E1B)
static struct { int delta_tLS, delta_tLSF; bool tLS_valid; } gps;

#define class struct
#include EPH_CUT_EPHEM_H
#undef class
EPHEM Ephemeris[MAX_SATS];
#include EPH_CUT_EPHEM_TIME
#include EPH_CUT_EPHEM_SUB
#include EPH_CUT_EPHEM_POS
#include EPH_CUT_EPHEM_FRAME
#include EPH_CUT_EPHEM_PAGES

#include EPH_CUT_SNAPSHOT
#include EPH_CUT_GETCLOCK

#include EPH_CUT_SC2RAD
#include EPH_CUT_P2
#include EPH_CUT_GTIME
#include EPH_CUT_EPH_T
#include EPH_CUT_EPOCHS
#include EPH_CUT_GETBIT
#include EPH_CUT_EPOCH2TIME
#include EPH_CUT_TIME2GPST
#include EPH_CUT_GST2TIME
#include EPH_CUT_GETBIT2

typedef struct { eph_t eph; double tow_gpst; int week_gpst; int cnt; int update; double toc_gst; int week_gst; } sdreph_t;
typedef struct { int sat; int tow_updated; sdreph_t sdreph; } sdrnav_t;

#include EPH_CUT_GAL_DEFS
#include EPH_CUT_GAL_WORDS
#include EPH_CUT_GAL_PAGE

struct CHANNEL { int sat; sdrnav_t nav; };
static CHANNEL chans[16];

static void print_state(int ch, int applied, int tow_updated, int err)
{
    const CHANNEL &c = chans[ch];
    EPHEM &e = Ephemeris[c.sat];
    printf("E %d %d %d %d %u %u %d %d %d %d |", applied, tow_updated, err, c.nav.sdreph.week_gst, (unsigned) c.nav.sdreph.eph.toes,
           (unsigned) c.nav.sdreph.toc_gst, gps.delta_tLS, gps.delta_tLSF, (int) gps.tLS_valid, (int) e.Valid());
    printf(" %u %u %u %u %u %u %a %a %a %a", e.IODN[0], e.IODN[1], e.IODN[2], e.IODN[3], e.IODC, e.t_oc, e.t_gd, e.a_f[0], e.a_f[1], e.a_f[2]);
    printf(" %u %u %a %a %a %a %a %a %a", e.IODE2, e.t_oe, e.C_rs, e.dn, e.M_0, e.C_uc, e.e, e.C_us, e.sqrtA);
    printf(" %u %a %a %a %a %a %a %a %a", e.IODE3, e.C_ic, e.OMEGA_0, e.C_is, e.i_0, e.C_rc, e.omega, e.OMEGA_dot, e.IDOT);
    for (int k = 0; k < 4; k++) printf(" %a", e.alpha[k]);
    for (int k = 0; k < 4; k++) printf(" %a", e.beta[k]);
    printf(" %u %u %u %u %a %a %u %u\n", e.week, e.tow, e.sub, e.tow_pg, e.A_0G, e.A_1G, e.t_0G, e.WN_0G);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const char *p = line.c_str() + 2;
        if (line[0] == 'K') {
            int sat, type;
            if (sscanf(p, "%d %d", &sat, &type) != 2) return 2;
            Sats[sat].type = (sat_e) type;
        } else if (line[0] == 'S') {
            int ch, sat;
            if (sscanf(p, "%d %d", &ch, &sat) != 2) return 2;
            chans[ch].sat = sat;                        // CHANNEL::Start, channel.cpp:274-277
            chans[ch].nav.sat = sat;
            Ephemeris[sat].Init(sat);
        } else if (line[0] == 'C') {
            int ch, n = 0;
            if (sscanf(p, "%d %n", &ch, &n) != 1) return 2;
            char buf[300];
            if (strlen(p + n) < 300) return 2;
            for (int i = 0; i < 300; i++) buf[i] = p[n + i] - '0';
            Ephemeris[chans[ch].sat].Subframe(buf);     // channel.cpp:825
            print_state(ch, 1, 1, 0);                   // bits_tow = holding - subframe_bits, :827
        } else if (line[0] == 'X') {
            int ch, err;
            if (sscanf(p, "%d %d", &ch, &err) != 2) return 2;
            print_state(ch, 0, 0, err);
        } else if (line[0] == 'G') {
            int ch, err_in, n = 0;
            if (sscanf(p, "%d %d %n", &ch, &err_in, &n) != 2) return 2;
            uint8_t dec[30];
            for (int i = 0; i < 30; i++) { unsigned v; if (sscanf(p + n + 2 * i, "%2x", &v) != 1) return 2; dec[i] = (uint8_t) v; }
            sdrnav_t *nav = &chans[ch].nav;
            nav->tow_updated = 0;                       // channel.cpp:754
            int err = (err_in == GPS_ERR_OOS) ? 0 : err_in, applied = 0;
            if (!err) {                                 // sdrnav_gal.cpp:483-485
                decode_page_e1b(dec, dec + 15, nav, &err);
                applied = 1;
            }
            print_state(ch, applied, nav->tow_updated, err);
        } else if (line[0] == 'V') {
            static SNAPSHOT r;
            double power;
            if (sscanf(p, "%d %d %d %d %d %d %la", &r.sat, &r.bits, &r.bits_tow, &r.ms, &r.chips, &r.cg_phase, &power) != 7) return 2;
            r.power = (float) power;
            int flags = 0, week = 0;
            double clock = 0, corr = 0, ct = 0, t_k = 0, x = 0, y = 0, z = 0;
            if (!Ephemeris[r.sat].Valid()) {            // LoadAtomic, solve.cpp:71
                flags = 1;
            } else {
                r.isE1B = is_E1B(r.sat);                // solve.cpp:73
                memcpy(&r.eph, Ephemeris + r.sat, sizeof r.eph);       // :81
                const double weight = r.power;          // _weight[_chans] = replicas[i].power, :327
                if (weight < 1e5 || weight > 5e6) {     // :330
                    flags = 2;
                } else {
                    double t_tx = r.GetClock();         // :334
                    clock = t_tx;
                    if (t_tx != t_tx) flags |= 8;
                    else if (r.tow_delayed) flags |= 4;
                    corr = r.eph.GetClockCorrection(t_tx);
                    t_tx -= corr;                       // :339
                    ct = C * t_tx;                      // :340
                    t_k = r.eph.TimeOfEphemerisAge(t_tx);       // :342
                    if (t_k == t_k) {                   // (int) NaN is undefined; x86 gives INT_MIN, which is not >= 4
                        UMS hms(fabs(t_k) / 60 / 60);   // :343
                        if (hms.u > 9) hms.u = 9;
                        if (hms.u >= 4) flags |= 16;    // :345
                    }
                    r.eph.GetXYZ(&x, &y, &z, t_tx);     // :351
                    week = r.eph.week;                  // :360
                }
            }
            printf("V %d %a %a %a %a %a %a %a %d\n", flags, clock, corr, ct, t_k, x, y, z, week);
        }
    }
    return 0;
}
