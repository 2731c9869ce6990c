// eph_dropin.cpp -- validated frames -> ephemeris -> satellite position and clock through include/kiwigpu.h only (no HIP, no torch):
// the sequence INTEGRATION.md section 6c maps onto the reference's gps/channel.cpp, gps/ephemeris.cpp and gps/solve.cpp.
//
//   CHANNEL::Start        nav.sat = sat; Ephemeris[sat].Init(sat)                       -> kg_eph_set_sat
//   CHANNEL::ParityCheck  Ephemeris[sat].Subframe(buf) / E1B_subframe -> decode_page_e1b -> kg_eph_push_frames
//   LoadAtomic            Ephemeris[sat].Valid(); memcpy(&eph, Ephemeris + sat, ..)     -> kg_eph_get (only to look at it)
//   LoadFromReplicas      GetClock, GetClockCorrection, TimeOfEphemerisAge, GetXYZ      -> kg_eph_sv
//
//   eph_dropin
// Builds subframes 1, 2, 3 of one Navstar satellite from raw fields (the 24 data bits of each word; the decode skips the parity bits,
// which kg_nav has already checked), pushes them as the records kg_nav would leave, and asks for the position at three clock readings.
// output: "valid <d> week <u> tow <u> t_oe <u> sqrtA <f> e <f>", then per reading "flags <d> x <f> y <f> z <f> ct <f> t_k <f>".
#include "kiwigpu.h"

#include <cstdio>
#include <cstring>

#define CHECK(call)                                                                      \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ < 0) { fprintf(stderr, "%s -> %s\n", #call, kg_last_error()); return 1; } \
    } while (0)

// value (two's complement, n bits) into the top n bits of the bytes from nav[byte] on: where EPHEM::Subframe1..3 read PACK(..).u / .s
static void put(uint8_t *nav, int byte, int n, long long value)
{
    for (int k = 0; k < n; k++) {
        const int bit = 8 * byte + k;
        const uint8_t v = (uint8_t) ((value >> (n - 1 - k)) & 1);
        nav[bit >> 3] = (uint8_t) ((nav[bit >> 3] & ~(0x80 >> (bit & 7))) | (v << (7 - (bit & 7))));
    }
}

// nav[30] -> one kg_nav_frame: ten words of 24 data bits and 6 parity bits (left zero)
static kg_nav_frame frame(const uint8_t *nav, int sub, uint64_t bit)
{
    kg_nav_frame f;
    memset(&f, 0, sizeof f);
    f.bit = bit; f.consumed = 300; f.id = sub;
    for (int w = 0; w < 10; w++)
        for (int k = 0; k < 24; k++) {
            const int src = 24 * w + k, dst = 30 * w + k;
            if ((nav[src >> 3] >> (7 - (src & 7))) & 1) f.data[dst >> 3] |= (uint8_t) (0x80 >> (dst & 7));
        }
    return f;
}

int main()
{
    kg_ctx *ctx = nullptr;
    kg_eph *eph = nullptr;
    CHECK(kg_ctx_create(0, nullptr, &ctx));
    CHECK(kg_eph_create(ctx, 1, &eph));
    const int sat = 4;
    CHECK(kg_eph_set_sat(eph, 0, sat, KG_EPH_NAVSTAR));

    const unsigned tow_count = 24100, toe = 9000;           // TOW 144600 s, t_oe = t_oc = 144000 s
    kg_nav_frame frames[3];
    for (int sub = 1; sub <= 3; sub++) {
        uint8_t nav[30];
        memset(nav, 0, sizeof nav);
        put(nav, 0, 8, 0x8B);
        put(nav, 3, 17, tow_count + sub - 1);
        nav[5] = (uint8_t) (nav[5] | (sub << 2));
        if (sub == 1) {
            put(nav, 6, 10, 201); put(nav, 20, 8, -11); put(nav, 21, 8, 77); put(nav, 22, 16, toe);
            put(nav, 25, 16, -40); put(nav, 27, 22, 123456);
        } else if (sub == 2) {
            put(nav, 6, 8, 77); put(nav, 7, 16, 1200); put(nav, 9, 16, 11000); put(nav, 11, 32, 0x30000000LL); put(nav, 15, 16, -900);
            put(nav, 17, 32, 0x02000000LL); put(nav, 21, 16, 2500); put(nav, 23, 32, (long long) (5153.6 * 524288.0)); put(nav, 27, 16, toe);
        } else {
            put(nav, 6, 16, 30); put(nav, 8, 32, -0x20000000LL); put(nav, 12, 16, -45); put(nav, 14, 32, 0x26666666LL); put(nav, 18, 16, 7000);
            put(nav, 20, 32, 0x10000000LL); put(nav, 24, 24, -22000); put(nav, 27, 8, 77); put(nav, 28, 14, 300);
        }
        frames[sub - 1] = frame(nav, sub, 300u * (unsigned) (sub - 1));
    }
    const int32_t count = 3;
    kg_eph_note notes[3];
    CHECK(kg_eph_push_frames(eph, frames, 3, &count, 3, notes, 3));
    kg_ephem e;
    CHECK(kg_eph_get(eph, sat, &e));
    printf("valid %d week %u tow %u t_oe %u sqrtA %.6f e %.9f\n", e.valid, e.week, e.tow, e.t_oe, e.sqrtA, e.e);
    if (!e.valid || !notes[2].valid || notes[2].bit_next != 900 || e.tow_bit != 900) { fprintf(stderr, "the ephemeris did not come out Valid\n"); return 1; }

    kg_eph_snap snaps[3];
    memset(snaps, 0, sizeof snaps);
    for (int k = 0; k < 3; k++) {
        int32_t chips = 0, cg_phase = 0;
        kg_eph_replica((uint32_t) ((17u + 5u * (unsigned) k) << 12 | (511u << 2)), &chips, &cg_phase);     // a word as kg_trk_get_clocks returns it
        snaps[k].sat = sat;
        snaps[k].bits = snaps[k].bits_tow = 40 + 100 * k;   // bits pushed - e.tow_bit
        snaps[k].ms = 7; snaps[k].chips = chips; snaps[k].cg_phase = cg_phase;
        snaps[k].power = k == 2 ? 1e4f : 1e6f;              // the last one fails the power gate
    }
    kg_eph_pos pos[3];
    memset(pos, 0, sizeof pos);
    CHECK(kg_eph_sv(eph, snaps, 3, pos));
    for (int k = 0; k < 3; k++)
        printf("flags %d x %.3f y %.3f z %.3f ct %.3f t_k %.6f\n", pos[k].flags, pos[k].x, pos[k].y, pos[k].z, pos[k].ct, pos[k].t_k);
    if (pos[0].flags != 0 || pos[2].flags != KG_EPH_SV_POWER) { fprintf(stderr, "unexpected flags\n"); return 1; }
    kg_eph_destroy(eph);
    kg_ctx_destroy(ctx);
    return 0;
}
