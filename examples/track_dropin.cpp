// track_dropin.cpp -- acquire -> start -> track through include/kiwigpu.h only (no HIP, no torch): the sequence INTEGRATION.md
// section 6a maps onto the reference's gps/search.cpp and gps/channel.cpp for a host whose 1-bit IF stream stays in GPU memory.
//
//   SearchTask()      ChanReset(sat, codegen_init); Sample(); Correlate(); ChanStart(ch, sat, t_sample, lo_shift, ca_shift, snr)
//   CHANNEL::Reset    CmdSetSat, CmdSetRateCG (nominal), CmdSetGainCG / LO            -> kg_trk_set_sat ... kg_trk_set_gain_lo
//   Sample()          CmdSample: the sampler reset also resets the free channels      -> kg_trk_sampler_reset
//   CHANNEL::Start    CmdSetRateLO, CmdSetRateCG, CmdPause(ca_pause - 1)              -> kg_trk_set_rate_lo / _cg, kg_trk_pause
//   (the FPGA runs)   DEMOD + GPS_Method, one service per code epoch                  -> kg_trk_process_bits
//   CHANNEL::Service  CmdGetChan: nav bits, lock flag, loop integrators               -> kg_trk_get_chan
//
//   track_dropin <packed_bits_file> <navstar_prn>
// input: a 1-bit IF stream, LSB first, at least 65536 + 16368 bits; the first 65536 are the acquisition's samples.
// output: "acq snr <f> lo_shift <d> ca_shift <d> lo_rate 0x<x> ca_rate 0x<x> ca_pause <u>", then per 100 epochs
// "epoch <n> clock <u> ip <d> qp <d> unlocked <d>", and a last line "nav_bits <d> glitches <d> unlocked <d> lo_hz <f> ca_hz <f>".
#include "kiwigpu.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(call)                                                                      \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ < 0) { fprintf(stderr, "%s -> %s\n", #call, kg_last_error()); return 1; } \
    } while (0)

// Navstar PRN 1..32 G2 tap pairs (IS-GPS-200; the first 32 rows of gps/sats.cpp's Sats[])
static const int TAPS[32][2] = {
    {2, 6}, {3, 7}, {4, 8}, {5, 9}, {1, 9}, {2, 10}, {1, 8}, {2, 9}, {3, 10}, {2, 3}, {3, 4}, {5, 6}, {6, 7}, {7, 8},
    {8, 9}, {9, 10}, {1, 4}, {2, 5}, {3, 6}, {4, 7}, {5, 8}, {6, 9}, {1, 3}, {4, 6}, {5, 7}, {6, 8}, {7, 9}, {8, 10},
    {1, 6}, {2, 7}, {3, 8}, {4, 9},
};

static void cacode(int t0, int t1, uint8_t *chips)          // gps/cacode.h restated, as in search_dropin.cpp
{
    int g1[11], g2[11];
    for (int i = 1; i <= 10; i++) g1[i] = g2[i] = 1;
    for (int n = 0; n < 1023; n++) {
        chips[n] = (uint8_t) (g1[10] ^ g2[t0] ^ g2[t1]);
        g1[0] = g1[3] ^ g1[10];
        g2[0] = g2[2] ^ g2[3] ^ g2[6] ^ g2[8] ^ g2[9] ^ g2[10];
        for (int i = 10; i >= 1; i--) { g1[i] = g1[i - 1]; g2[i] = g2[i - 1]; }
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s packed_bits_file navstar_prn\n", argv[0]); return 2; }
    const int prn = atoi(argv[2]);
    if (prn < 1 || prn > 32) { fprintf(stderr, "this example knows the 32 Navstar rows only\n"); return 2; }
    std::vector<uint8_t> bits;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) bits.insert(bits.end(), buf, buf + n);
    fclose(f);
    const size_t FS = 16368000, NSAMPLES = KG_ACQ_NSAMPLES, total = bits.size() * 8;
    if (total < NSAMPLES + FS / 1000) { fprintf(stderr, "the stream is shorter than the acquisition's samples and one epoch\n"); return 2; }

    kg_ctx *kg = NULL;
    kg_acq *kacq = NULL;
    kg_trk *trk = NULL;
    const int sat = prn - 1, ch = 0;
    CHECK(kg_ctx_create(0, NULL, &kg));
    CHECK(kg_acq_create(kg, 64, -20, 20, 1, &kacq));
    CHECK(kg_trk_create(kg, 1, 0, 0, &trk));                   // 0, 0: the service delays of a channel serviced alone
    uint8_t chips[1023];
    cacode(TAPS[sat][0], TAPS[sat][1], chips);
    CHECK(kg_acq_set_code(kacq, sat, chips, 1023, 0, KG_ACQ_L1_LIMIT));

    // ChanReset(): CHANNEL::Reset
    CHECK(kg_trk_set_sat(trk, ch, (TAPS[sat][0] << 4) + TAPS[sat][1]));       // search.cpp:560
    CHECK(kg_trk_set_rate_cg(trk, ch, 1u << 28));                             // CPS / FS * 2^32
    CHECK(kg_trk_set_gain_cg(trk, ch, 20 - 9, 12));                           // channel.cpp:187-195
    CHECK(kg_trk_set_gain_lo(trk, ch, 20, 7));                                // :173-181
    // Sample(): the sampler reset falls on the stream's first clock; the channel runs free while the host correlates
    CHECK(kg_trk_sampler_reset(trk));
    CHECK(kg_acq_sample_bits(kacq, 0, bits.data()));
    kg_acq_result r;
    CHECK(kg_acq_correlate(kacq, 1, &sat, 1, &r, NULL));
    kg_chan_start cs;
    memset(&cs, 0, sizeof cs);
    kg_acq_chan_start(0, r.dop, r.idx * KG_ACQ_DECIM, (double) NSAMPLES / FS, &cs);
    printf("acq snr %.4f lo_shift %d ca_shift %d lo_rate 0x%08x ca_rate 0x%08x ca_pause %u\n", r.snr, r.dop, r.idx * KG_ACQ_DECIM, cs.lo_rate,
           cs.ca_rate, cs.ca_pause);
    if (!r.valid || r.snr < 16) { fprintf(stderr, "nothing found\n"); return 3; }

    std::vector<kg_trk_epoch> ep(NSAMPLES / KG_TRK_MIN_EPOCH + 2 + FS / 10 / KG_TRK_MIN_EPOCH + 2);
    int32_t count = 0;
    CHECK(kg_trk_process_bits(trk, bits.data(), NSAMPLES, ep.data(), ep.size(), (int) ep.size(), &count));
    // CHANNEL::Start
    CHECK(kg_trk_set_rate_lo(trk, ch, cs.lo_rate));
    CHECK(kg_trk_set_rate_cg(trk, ch, cs.ca_rate));
    if (cs.ca_pause) CHECK(kg_trk_pause(trk, ch, (int) cs.ca_pause - 1));
    // the stream, 100 ms at a time
    size_t clock = NSAMPLES, epochs = 0;
    while (clock < total) {
        const size_t step = total - clock < FS / 10 ? total - clock : FS / 10;
        CHECK(kg_trk_process_bits(trk, bits.data() + clock / 8, step, ep.data(), ep.size(), (int) ep.size(), &count));
        for (int i = 0; i < count; i++, epochs++)
            if (epochs % 100 == 0)
                printf("epoch %zu clock %llu ip %d qp %d unlocked %d\n", epochs, (unsigned long long) ep[i].clock, ep[i].ip, ep[i].qp,
                       (int) (ep[i].flags & KG_TRK_UNLOCKED));
        clock += step;
    }
    // CHANNEL::Service: UploadEmbeddedState
    uint8_t ul[KG_TRK_CHAN_BYTES];
    CHECK(kg_trk_get_chan(trk, ch, ul));
    uint16_t w[KG_TRK_CHAN_BYTES / 2];
    memcpy(w, ul, sizeof w);
    uint64_t ca = 0, lo = 0;                                  // ul.ca_freq, ul.lo_freq: little-endian 64-bit loop integrators
    for (int i = 3; i >= 0; i--) { ca = (ca << 16) | w[12 + i]; lo = (lo << 16) | w[16 + i]; }
    const double ca_frac = (double) ca / 18446744073709551616.0, lo_frac = (double) lo / 18446744073709551616.0;   // Get64_frac()
    printf("nav_bits %d glitches %d unlocked %d lo_hz %.1f ca_hz %.3f\n", w[1], w[2], w[36] ? 1 : 0, lo_frac * FS - 4.092e6, ca_frac * FS - 1.023e6);
    kg_trk_destroy(trk);
    kg_acq_destroy(kacq);
    kg_ctx_destroy(kg);
    return 0;
}
