// ref_nav_main.cpp -- the harness tools/make_ref_nav_golden.py compiles around text CUT from the reference tree at build time (never
// committed): the frame-sync part of CHANNEL::Tracking() run on scripted bit streams, every judged head printed.
//
//   cut (the NAV_CUT_* macros name the files the generator writes):
//     gps/channel.cpp        L1_PRELEN .. E1BpreambleInverse (:120-145), the polynomial / create lines of Tracking() (:414-416), the
//                            `while (holding >= subframe_bits)` loop up to its memmove (:452-506), CHANNEL::ParityCheck (:731-832)
//     gps/gps.h              GPS_ERR_* (:187-191)
//     GNSS-SDRLIB/sdrnav_gal.cpp   OFFSET1 / OFFSET2 (:19-20), word 5's health statements (:162-174), checkcrc_e1b (:293-319),
//                            E1B_subframe (:382-514)
//     GNSS-SDRLIB/sdrnav.cpp bits2byte, interleave (:154-190)
//     GNSS-SDRLIB/rtkcmn.cpp tbl_CRC24Q (:271-304), getbitu (:598-604), crc24q (:662-671)
//   linked where it lies: gps/ka9q-fec/viterbi27_port.cpp (parity() comes with its fec.h)
//   restated here and pinned by text in the generator: MAXBITS (gnss_sdrlib.h:136); the append of new bits to buf (:441-450 takes them
//     from the firmware's 16-bit ring: here one byte per bit, buf[holding++] = bit); the locals and resets Tracking() makes before its
//     loop (:398-409) and subframe_bits (CHANNEL::Reset, :278); decode_page_e1b reduced to its id statement (:336), `case 5` (:346) and
//     its error hand-over (:357); the members of CHANNEL and sdrnav_t that the cut text names.
//   C/A's `inverted` is not a variable of the reference (ParityCheck sets p[4] = p[5]); the harness reads it off the same memcmp
//     before the call, since L1_parity then corrects the preamble's bits in place.
//
// script (stdin): "T <isE1B>" enters Tracking(); "P <bits as 0/1 characters>" appends and runs the loop; output per judged head
// "F <bit> <err> <consumed> <inverted> <id> <80 hex digits>", per push "H <holding> <index of buf[0]>".
#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <iostream>

#include "fec.h"
void set_viterbi27_polynomial_port(int polys[2]);
int update_viterbi27_blk_port(void *p, unsigned char *syms, int nbits);

#define QUIET
#define MAXBITS 3000
#define trace(...) ((void) 0)
#define KG_NAV_ERR_PARITY 16
typedef unsigned int u4_t;

#include NAV_CUT_GPSERR
#include NAV_CUT_CRCTAB
#include NAV_CUT_GETBITU
#include NAV_CUT_CRC24Q
#include NAV_CUT_SDRNAV

typedef struct { int flen; char *fbits; int polarity; void *fec; int sat; int tow_updated; } sdrnav_t;

#include NAV_CUT_OFFSETS
#include NAV_CUT_CHECKCRC

extern int decode_page_e1b(const uint8_t *buff1, const uint8_t *buff2, sdrnav_t *nav, int *error)
{
    int id;
    uint8_t both[30];
    const uint8_t *buff = both;
    memcpy(both, buff1, 15); memcpy(&both[15], buff2, 15);
    id = getbitu(buff, 2, 6);
    int err = 0;
    if (id == 5) {
        unsigned int e1bdvs, e1bhs, e5bdvs, e5bhs;
#include NAV_CUT_WORD5
        (void) e5bdvs; (void) e5bhs;
    }
    if (err && error) *error = err;
    return id;
}

static uint8_t cap_dec[2][15];
static int cap_n, cap_err, cap_id;
static int chainback_capture(void *p, unsigned char *data, unsigned int nbits, unsigned int endstate)
{
    const int r = chainback_viterbi27_port(p, data, nbits, endstate);
    memcpy(cap_dec[cap_n++ & 1], data, 15);
    return r;
}
#define chainback_viterbi27_port chainback_capture
#include NAV_CUT_E1B_SUBFRAME
#undef chainback_viterbi27_port
static int E1B_subframe_capture(sdrnav_t *nav, int *error)
{
    cap_n = 0;
    const int id = E1B_subframe(nav, error);
    cap_err = *error; cap_id = id;
    return id;
}

#include NAV_CUT_PREAMBLES

#define GPSstat(...) ((void) 0)
#define PRN(s) ""
#define STAT_SUB 0
#define PARITY 0
static int gps_debug = 0;
static struct { int prn; } Sats[1];
static struct { int include_alert_gps, kick_lo_pll_ch; } gps;
static struct { int sub, tow_pg, tow; void Subframe(char *) {} } Ephemeris[1];
static u4_t timer_sec() { return 0; }

struct CHANNEL {
    int ch, sat, isE1B, inverted, nsync, total_bits, probation, holding, subframe_bits, bits_tow, expecting_preamble, drop_seq, LASTsub, ACF_mode;
    bool alert, abort;
    sdrnav_t nav;
    char buf[1 << 17];
    uint64_t appended;
    void Status() {}
    void Subframe(char *) {}
    int ParityCheck(char *buf, int *nbits);
    int Recorded(char *buf, int *nbits);
    void Enter(int e1b);
    void Loop();
};

#define E1B_subframe E1B_subframe_capture
#include NAV_CUT_PARITYCHECK
#undef E1B_subframe

int CHANNEL::Recorded(char *b, int *nbits)
{
    const int inv_ca = memcmp(b, L1preambleInverse, L1_PRELEN) == 0;
    const int err = ParityCheck(b, nbits);
    if (*nbits == 1) return err;
    uint8_t data[40];
    memset(data, 0, sizeof data);
    int e, id, inv;
    if (isE1B) {
        e = cap_err; id = cap_id; inv = inverted;
        memcpy(data, cap_dec[0], 15); memcpy(data + 15, cap_dec[1], 15);
    } else if (err) {
        e = KG_NAV_ERR_PARITY; id = *nbits / 30 - 1; inv = inv_ca;
    } else {
        e = 0; inv = inv_ca; id = (b[49] << 2) | (b[50] << 1) | b[51];
        for (int i = 0; i < 300; i++) data[i >> 3] |= (uint8_t) ((b[i] & 1) << (7 - (i & 7)));
    }
    printf("F %llu %d %d %d %d ", (unsigned long long) (appended - (uint64_t) holding), e, *nbits, inv, id);
    for (int i = 0; i < 40; i++) printf("%02x", data[i]);
    printf("\n");
    return err;
}

void CHANNEL::Enter(int e1b)
{
    isE1B = e1b; subframe_bits = isE1B ? E1B_TSYM_PW : 300;
    ch = 0; sat = 0; probation = 0; bits_tow = 0; LASTsub = 0; alert = false; abort = false; inverted = 0;
    holding = 0; nsync = 0; total_bits = 0; expecting_preamble = 0; drop_seq = 0; ACF_mode = 0;
    appended = 0;
    memset(&nav, 0, sizeof nav);
    if (isE1B) {
#include NAV_CUT_POLYS
    }
}

void CHANNEL::Loop()
{
    int watchdog = 0, seen_data = 0;
    float sumpwr = 0;
    u4_t t_last_data = 0;
#define ParityCheck Recorded
#include NAV_CUT_LOOP
    }
#undef ParityCheck
    (void) watchdog; (void) seen_data; (void) sumpwr; (void) t_last_data;
}

static CHANNEL chan;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        if (line[0] == 'T') {
            chan.Enter(atoi(line.c_str() + 2));
        } else if (line[0] == 'P') {
            for (size_t i = 2; i < line.size(); i++)
                if (line[i] == '0' || line[i] == '1') { chan.buf[chan.holding++] = line[i] - '0'; chan.appended++; }
            chan.Loop();
            printf("H %d %llu\n", chan.holding, (unsigned long long) (chan.appended - (uint64_t) chan.holding));
        }
    }
    return 0;
}
