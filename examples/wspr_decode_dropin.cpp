// A host that already has the reference's WSPR decoder, handing its candidates to the GPU (include/kiwigpu.h only).
//
// The reference makes mettab in wspr_init (extensions/wspr/wspr.cpp:431-441) from the float table it is compiled with:
//     mettab[0][i] = round(10 * (t[i] - 0.45));  mettab[1][i] = round(10 * (t[255 - i] - 0.45));
// The library does not carry that table: the host passes ITS mettab, once (kg_wspr_set_metric_table).  Here `t` is read from the file
// named on the command line -- 256 floats, the row of the host's table that its wspr_init uses -- or, without one, a stand-in of the same
// shape, which is enough for the clean signal this program makes.
// Then, per cycle: i_data / q_data of the decode half and the candidates of the peak list (freq0, shift0, drift0, sync0 in SNR order)
// go in (kg_wspr_load_iq; a host that feeds kg_wspr_push has them on the device already), and the passes of wspr_decode are calls of
// kg_wspr_decode with the reference's progression of maxcycles / iifac.  A record with result KG_WSPR_DECODED carries decdata for unpk_.
// The program encodes a message, decodes it and checks the bytes: exit status 0 and "decoded ..." on success.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kiwigpu.h"

static int parity32(uint32_t v) { v ^= v >> 16; v ^= v >> 8; v ^= v >> 4; v ^= v >> 2; v ^= v >> 1; return (int) (v & 1); }

int main(int argc, char **argv)
{
    // the host's table -> mettab, by the reference's own formula
    float t[256];
    for (int i = 0; i < 256; i++) t[i] = 1.0f - expf((float) (i - 128) / 32.0f);
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f || fread(t, sizeof(float), 256, f) != 256) { fprintf(stderr, "%s: 256 floats expected\n", argv[1]); return 2; }
        fclose(f);
    }
    static int32_t mettab[2][256];
    const float bias = 0.45f;
    for (int i = 0; i < 256; i++) {
        mettab[0][i] = (int32_t) lround(10 * (t[i] - bias));
        mettab[1][i] = (int32_t) lround(10 * (t[255 - i] - bias));
    }

    // a message: 50 bits, 31 zeros behind them, the K = 32 rate 1/2 code, the bit-reversal interleaver, 2 * bit + sync
    static const char *pr3 = "110000001000111000100101111000000010010100000010110011010001101000011010101010010010110001101010001000001001001110110011010001110000010100110000000110101100011000";
    uint8_t bits[81] = {0}, code[162], sent[162], want[10] = {0};
    for (int k = 0; k < 50; k++) bits[k] = (uint8_t) ((0x2b5f19c3a7e4dULL >> k) & 1);
    for (int k = 0; k < 80; k++) want[k / 8] = (uint8_t) (want[k / 8] | (bits[k] << (7 - k % 8)));
    uint32_t state = 0;
    for (int k = 0; k < 81; k++) {
        state = (state << 1) | bits[k];
        code[2 * k] = (uint8_t) parity32(state & 0xf2d05351u);
        code[2 * k + 1] = (uint8_t) parity32(state & 0xe4613c47u);
    }
    for (int i = 0, p = 0; i < 256 && p < 162; i++) {
        int j = 0;
        for (int b = 0; b < 8; b++) j |= ((i >> b) & 1) << (7 - b);
        if (j < 162) sent[j] = code[p++];
    }
    // 45000 samples at 375 Hz: the message 20.3 Hz above the centre from sample 750 on, amplitude 1000, a little deterministic dither
    const int np = KG_WSPR_TPOINTS, start = 750;
    const double f0 = 20.3, two_pi = 6.283185307179586;
    std::vector<float> id(np), qd(np);
    double ph = 0;
    uint32_t lcg = 12345;
    for (int k = 0; k < np; k++) {
        lcg = lcg * 1664525u + 1013904223u;
        const float dither = (float) ((int) (lcg >> 24) - 128);
        id[k] = dither; qd[k] = -dither;
        const int s = (k - start) / 256;
        if (k >= start && s < 162) {
            const int tone = 2 * sent[s] + (pr3[s] - '0');
            ph += two_pi * (f0 + (tone - 1.5) * 375.0 / 256) / 375.0;
            id[k] += (float) (1000 * cos(ph)); qd[k] += (float) (1000 * sin(ph));
        }
    }

    kg_ctx *ctx = NULL;
    kg_wspr *w = NULL;
    if (kg_ctx_create(0, NULL, &ctx) || kg_wspr_create(ctx, 1, &w) || kg_wspr_init(w, 0, 375.0) || kg_wspr_set_metric_table(w, mettab)) {
        fprintf(stderr, "setup: %s\n", kg_last_error());
        return 1;
    }
    // what the host's peak list and coarse search found: the bin nearest 20.3 Hz, the half-symbol step nearest 750
    kg_wspr_cand cand;
    memset(&cand, 0, sizeof cand);
    cand.freq0 = 28 * 0.732421875f; cand.shift0 = 768; cand.drift0 = 0.0f; cand.sync0 = 0.5f;
    if (kg_wspr_load_iq(w, 0, 0, id.data(), qd.data(), &cand, 1)) { fprintf(stderr, "load: %s\n", kg_last_error()); return 1; }
    static const int passes[4][2] = {{200, 2}, {1000, 1}, {5000, 1}, {10000, 1}};       // wspr.cpp:505-508 and the passes behind them
    int ok = 0;
    for (int ps = 0; ps < 4 && !ok; ps++) {
        kg_wspr_dec rec[KG_WSPR_MAX_NPK];
        int32_t ncand = 0, conn = 0;
        if (kg_wspr_decode(w, &conn, 1, (uint32_t) passes[ps][0], passes[ps][1], 0, rec, &ncand)) { fprintf(stderr, "decode: %s\n", kg_last_error()); return 1; }
        for (int c = 0; c < ncand; c++) {
            printf("pass %d candidate %d: result %d f1 %.3f shift1 %d drift1 %.1f sync1 %.3f jiggles %d cycles %u\n", ps, c, rec[c].result, (double) rec[c].f1,
                   rec[c].shift1, (double) rec[c].drift1, (double) rec[c].sync1, rec[c].idt, rec[c].cycles);
            if (rec[c].result == KG_WSPR_DECODED && !memcmp(rec[c].decdata, want, 10)) ok = 1;
        }
    }
    kg_wspr_destroy(w);
    kg_ctx_destroy(ctx);
    if (!ok) { fprintf(stderr, "not decoded\n"); return 1; }
    printf("decoded ");
    for (int k = 0; k < 10; k++) printf("%02x", want[k]);
    printf("\n");
    return 0;
}
