// A host that has the reference's FT8 extension, handing its real-samples callbacks to the GPU (include/kiwigpu.h only).
//
// Where the reference calls decode_ft8_samples(rx_chan, samps, FASTFIR_OUTBUF_SIZE, ...) from its real-samples task
// (extensions/FT8/FT8.cpp:136) and reads the clock inside it (ft8_lib/decode_ft8.c:512), this host passes the callbacks AND the clock
// reading of each to kg_ft8_push.  A push returns the events (slot start, decode) and, for a slot that ended, a kg_ft8_slot: the
// candidates of ftx_find_candidates with freq_hz / time_sec / snr and log174, the input of the host's own bp_decode (ft8/decode.c:345).
// A host whose audio already lives on the GPU uses the receiver bank instead: kg_rxbank_ft8_init / _start / _set_now / _out.
// The program makes one slot of noise with a synthetic 8-FSK frame -- the three Costas groups and pseudo-random data tones -- whose first
// symbol sits on block 3 and whose lowest tone on bin 100, pushes it 8 callbacks at a time, and checks that the strongest candidate is
// that frame: exit status 0 and "found ..." on success.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "kiwigpu.h"

int main()
{
    const int ns = 512, block = 1920, ncb = 352;                     // 15 s of callbacks at 12000 Hz
    const int costas[7] = {3, 1, 4, 0, 6, 5, 2};
    const int time_offset = 3, freq_offset = 100;
    std::vector<int16_t> x((size_t) ncb * ns);
    std::vector<double> t((size_t) ncb);
    uint32_t lcg = 2024;
    for (size_t k = 0; k < x.size(); k++) { lcg = lcg * 1664525u + 1013904223u; x[k] = (int16_t) ((int) (lcg >> 24) - 128); }
    const double two_pi = 6.283185307179586, f0 = (16 + freq_offset) / 0.16;      // bin 16 is 100 Hz (monitor.c:103); a bin is 6.25 Hz
    const int s0 = time_offset * block - block;                      // symbol 0 centred on the analysis frame of block 3, time_sub 0
    double ph = 0;
    for (int sym = 0; sym < 79; sym++) {
        int tone;
        if (sym < 7 || (sym >= 36 && sym < 43) || sym >= 72) tone = costas[sym % 36];
        else { lcg = lcg * 1664525u + 1013904223u; tone = (int) (lcg >> 29); }
        for (int k = 0; k < block; k++) {
            ph += two_pi * (f0 + tone * 6.25) / 12000.0;
            x[(size_t) s0 + (size_t) sym * block + k] = (int16_t) (x[(size_t) s0 + (size_t) sym * block + k] + (int) lround(3000 * sin(ph)));
        }
    }
    for (int cb = 0; cb < ncb; cb++) t[cb] = 1500000000.0 + 0.8125 + cb * (ns / 12000.0);      // 1.5e9 is a multiple of 15: the first callback syncs

    kg_ctx *ctx = NULL;
    kg_ft8 *q = NULL;
    if (kg_ctx_create(0, NULL, &ctx) || kg_ft8_create(ctx, 1, &q) || kg_ft8_init(q, 0, KG_FT8_PROTO_FT8, 12000.0)) {
        fprintf(stderr, "setup: %s\n", kg_last_error());
        return 1;
    }
    static kg_ft8_slot slot;
    int found = 0;
    for (int cb = 0; cb < ncb; cb += 8) {
        kg_ft8_ev ev[8];
        int32_t conn = 0, n = ncb - cb < 8 ? ncb - cb : 8, nev = 0, nslots = 0;
        if (kg_ft8_push(q, &conn, 1, &n, ns, &x[(size_t) cb * ns], (size_t) n * ns, &t[cb], (size_t) n, ev, 8, &nev, &slot, 1, &nslots)) {
            fprintf(stderr, "push: %s\n", kg_last_error());
            return 1;
        }
        for (int e = 0; e < nev; e++)
            printf("callback %d: %s slot %d\n", cb + ev[e].cb, ev[e].kind == KG_FT8_EV_SLOT_START ? "start of" : "decode of", ev[e].kind == KG_FT8_EV_SLOT_START ? ev[e].a : ev[e].b);
        if (nslots) {
            printf("%d blocks, max %.1f dB, %d candidates\n", slot.num_blocks, (double) slot.max_mag, slot.ncand);
            for (int c = 0; c < slot.ncand && c < 3; c++)
                printf("  score %d at %+.2f s %.1f Hz (block %d.%d bin %d.%d) snr %.1f log174[0] %.3f\n", slot.cand[c].score, (double) slot.cand[c].time_sec,
                       (double) slot.cand[c].freq_hz, slot.cand[c].time_offset, slot.cand[c].time_sub, slot.cand[c].freq_offset, slot.cand[c].freq_sub, (double) slot.cand[c].snr,
                       (double) slot.log174[c][0]);
            found = slot.ncand > 0 && slot.cand[0].time_offset == time_offset && slot.cand[0].time_sub == 0 && slot.cand[0].freq_offset == freq_offset && slot.cand[0].freq_sub == 0;
        }
    }
    kg_ft8_destroy(q);
    kg_ctx_destroy(ctx);
    if (!found) { fprintf(stderr, "the planted frame is not the strongest candidate\n"); return 1; }
    printf("found the frame at block %d, bin %d\n", time_offset, freq_offset);
    return 0;
}
