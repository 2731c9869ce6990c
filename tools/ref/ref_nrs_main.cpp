// Developer tool (CPU machine only; tools/make_ref_nrs_golden.py builds and runs it): NR_SPECTRAL as the reference runs it --
// c2s_sound()'s noise-reduction switch (rx/rx_sound.cpp:933-949), the two `SET nr` commands (rx/rx_sound_cmd.cpp:464-471, their
// shared declarations :473-475, :505-523) and the normalised passband (:252-266) as the reference's own statements, cut at build
// time into a temporary directory; rx/Teensy/NR_spectral.cpp #included where it lies (nr_spectral[] and tinc .. ap are
// file-static, and the end states are read from them); rx/wdsp/ANR.cpp #included and rx/kiwi/lms.cpp, rx/CMSIS/arm_cfft_f32.cpp,
// arm_cfft_radix8_f32.cpp and arm_bitreversal2.cpp linked where they lie.  Nothing of the reference's text enters the repository;
// only the data (tests/golden/nrs_ref.npz) does.
//
// What this harness adds:
//   * THE TWO TABLES THE REFERENCE TREE LACKS.  rx/CMSIS/arm_common_tables.h declares twiddleCoef_512[1024] and
//     armBitRevIndexTable512[448], and no file of the tree defines them.  The twiddles are read from tw.bin, which the builder
//     writes ((float) cos, (float) sin of 2 pi k / 512, evaluated in double) and stores in the golden file; the bit-reversal table
//     is made here as the 224 pairs (8 i, 8 rev(i)), i < rev(i), rev = reversal of the three base-8 digits.  The instance
//     arm_cfft_sR_f32_len512 is defined here instead of linking arm_const_structs.cpp (which names every other size's tables).
//   * assert_array_dim COUNTED instead of panicking: the builder asserts the count is 0 for every scenario.  The same macro reads
//     the local NN of nr_spectral_process at the call sites that have it in scope (a file-scope NN = -1 serves the others), for
//     the per-frame NN trace; it changes no arithmetic.
//   * a `switch (cmd_kind)` around the command cases, the connection start's two statements (rx_sound.cpp:236, :240), the stage's
//     enclosing `if (!IQ_or_DRM_or_stereo)` (:923).
//
//   nrs_ref snd_rate script.txt in.bin tw.bin out.bin st.bin tr.bin misc.bin
// script lines:
//   A algo / E type en / P type param pval / C / B n stereo     as tools/ref/ref_nr_main.cpp (n = 512 here: the stage asserts it)
//   M locut hicut        -> s->locut, s->hicut (already clamped, rx_sound_cmd.cpp:248-250), then :252-266
//   S                    -> st.bin: int32 first_time, init_counter; float final_gain, alpha, asnr, xih1r, pfac, tinc, tax, tap, ax,
//                           ap, norm_locut, norm_hicut; then last_sample_buffer, last_iFFT_result, NR_Nest, xt, pslp,
//                           NR_SNR_post, NR_SNR_prio, NR_Hk_old, NR_G (256 floats each)
// tr.bin: per B that ran the spectral stage, int32 NN of the block's phase-3 frames in order (0-padded to two), the number of bins
// with pslp > psthr after the block, first_time after the block.
// misc.bin: int32 out-of-bounds count; then sqrtHann_256 as the binary holds it (256 floats).
#define private public
#include "types.h"           // rx_sound.cpp:20-64 in its own order, as tools/ref/ref_nr_main.cpp
#include "options.h"
#include "config.h"
#include "kiwi.h"
#include "mode.h"
#include "printf.h"
#include "rx.h"
#include "rx_util.h"
#include "clk.h"
#include "mem.h"
#include "misc.h"
#include "str.h"
#include "timer.h"
#include "nbuf.h"
#include "web.h"
#include "spi.h"
#include "gps.h"
#include "coroutines.h"
#include "cuteSDR.h"
#include "rx_noise.h"
#include "teensy.h"
#include "agc.h"
#include "fir.h"
#include "iir.h"
#include "squelch.h"
#include "debug.h"
#include "data_pump.h"
#include "cfg.h"
#include "mongoose.h"
#include "ima_adpcm.h"
#include "ext_int.h"
#include "fastfir.h"
#include "noiseproc.h"
#include "lms.h"
#include "dx.h"
#include "noise_blank.h"
#include "rx_sound.h"
#include "rx_sound_cmd.h"
#include "rx_waterfall.h"
#include "rx_filter.h"
#include "wdsp.h"
#include "fpga.h"
#include "rf_attn.h"
#include "timing.h"
#include "noise_filter.h"
#include "arm_math.h"
#include "arm_const_structs.h"
#undef private
#undef printf
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int oob_count, cur_nn, frame_nn[2], frame_k;
static int NN = -1;              // what the counting macro sees where nr_spectral_process's local NN is not in scope
#undef assert_array_dim
#define assert_array_dim(ai, dim) \
    do { \
        if (!((ai) >= (0) && (ai) < (dim))) oob_count++; \
        if (NN > 0) cur_nn = NN; \
        else if (cur_nn > 0) { if (frame_k < 2) frame_nn[frame_k++] = cur_nn; cur_nn = 0; } \
    } while (0)
#undef assert
#define assert(e) do { if (!(e)) { fprintf(stderr, "assert %s\n", #e); exit(7); } } while (0)

int snd_rate;                                    // config.h:51-52
snd_t snd_inst[MAX_RX_CHANS];

static float tw512[1024];
static uint16_t br512[448];
extern "C" { const arm_cfft_instance_f32 arm_cfft_sR_f32_len512 = {512, tw512, br512, 448}; }

#include NR_ANR_CPP
#include NR_SPECTRAL_CPP

static int rev3(int i) { return ((i & 7) << 6) | (i & 0x38) | (i >> 6); }

enum { K_ALGO, K_TYPE };
static void nr_cmd(int rx_chan, snd_t *s, int cmd_kind, const char *cmd)
{
    bool did_cmd = false;
    int n;
    switch (cmd_kind == K_ALGO ? CMD_NR_ALGO : CMD_NR_TYPE) {
#include "NR_CUT_ALGO.inc"
#include "NR_CUT_DECLS.inc"
#include "NR_CUT_TYPE.inc"
    default: break;
    }
    (void) n;
    if (!did_cmd) { fprintf(stderr, "command not taken: %s\n", cmd); exit(5); }
}

static void passband(snd_t *s)
{
#include "NR_CUT_NORM.inc"
}

int main(int argc, char **argv)
{
    if (argc != 9) { fprintf(stderr, "usage: %s snd_rate script in.bin tw.bin out.bin st.bin tr.bin misc.bin\n", argv[0]); return 2; }
    snd_rate = atoi(argv[1]);
    FILE *sf = fopen(argv[2], "r"), *inf = fopen(argv[3], "rb"), *twf = fopen(argv[4], "rb"), *outf = fopen(argv[5], "wb"),
         *stf = fopen(argv[6], "wb"), *trf = fopen(argv[7], "wb"), *mf = fopen(argv[8], "wb");
    if (!sf || !inf || !twf || !outf || !stf || !trf || !mf) { fprintf(stderr, "cannot open files\n"); return 2; }
    if (fread(tw512, sizeof(float), 1024, twf) != 1024) return 2;
    int nbr = 0;
    for (int i = 0; i < 512; i++)
        if (i < rev3(i)) { br512[nbr++] = (uint16_t) (8 * i); br512[nbr++] = (uint16_t) (8 * rev3(i)); }
    if (nbr != 448) return 2;
    const int rx_chan = 0;
    snd_t *s = &snd_inst[rx_chan];
    static TYPEMONO16 out_samps_s2[4096];
    char line[1024], cmd[256];
    memset(s, 0, sizeof(snd_t)); s->nr_algo = NR_OFF_;                 // rx_sound.cpp:236, :240
    while (fgets(line, sizeof line, sf)) {
        const char op = line[0];
        if (op == 'A') {
            int a;
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            snprintf(cmd, sizeof cmd, "SET nr algo=%d", a);
            nr_cmd(rx_chan, s, K_ALGO, cmd);
        } else if (op == 'E') {
            int t, e;
            if (sscanf(line + 1, "%d %d", &t, &e) != 2) return 3;
            snprintf(cmd, sizeof cmd, "SET nr type=%d en=%d", t, e);
            nr_cmd(rx_chan, s, K_TYPE, cmd);
        } else if (op == 'P') {
            int t, p;
            char v[64];
            if (sscanf(line + 1, "%d %d %63s", &t, &p, v) != 3) return 3;
            snprintf(cmd, sizeof cmd, "SET nr type=%d param=%d pval=%s", t, p, v);
            nr_cmd(rx_chan, s, K_TYPE, cmd);
        } else if (op == 'M') {
            double lo, hi;
            if (sscanf(line + 1, "%lf %lf", &lo, &hi) != 2) return 3;
            s->locut = lo; s->hicut = hi;
            passband(s);
        } else if (op == 'C') {
            memset(s, 0, sizeof(snd_t)); s->nr_algo = NR_OFF_;
        } else if (op == 'B') {
            int ns_out, stereo;
            if (sscanf(line + 1, "%d %d", &ns_out, &stereo) != 2 || ns_out < 1 || ns_out > 4096) return 3;
            if (fread(out_samps_s2, sizeof(TYPEMONO16), ns_out, inf) != (size_t) ns_out) return 4;
            const bool IQ_or_DRM_or_stereo = stereo != 0;
            frame_nn[0] = frame_nn[1] = 0; cur_nn = 0; frame_k = 0;
            if (!IQ_or_DRM_or_stereo) {
#include "NR_CUT_STAGE.inc"
            fwrite(out_samps_s2, sizeof(TYPEMONO16), ns_out, outf);
            if (!IQ_or_DRM_or_stereo && s->nr_algo == NR_SPECTRAL) {
                const nr_spectral_t *w = &nr_spectral[rx_chan];
                int over = 0;
                for (int b = 0; b < FFT_HALF; b++) over += w->pslp[b] > psthr;
                const int tr[4] = {frame_nn[0], frame_nn[1], over, w->first_time};
                fwrite(tr, sizeof tr, 1, trf);
            }
        } else if (op == 'S') {
            const nr_spectral_t *w = &nr_spectral[rx_chan];
            const int iv[2] = {w->first_time, w->init_counter};
            const float fv[12] = {w->final_gain, w->alpha, w->asnr, w->xih1r, w->pfac, tinc, tax, tap, ax, ap, s->norm_locut, s->norm_hicut};
            fwrite(iv, sizeof iv, 1, stf);
            fwrite(fv, sizeof fv, 1, stf);
            fwrite(w->last_sample_buffer, sizeof(float), FFT_HALF, stf);
            fwrite(w->last_iFFT_result, sizeof(float), FFT_HALF, stf);
            fwrite(w->NR_Nest, sizeof(float), FFT_HALF, stf);
            fwrite(w->xt, sizeof(float), FFT_HALF, stf);
            fwrite(w->pslp, sizeof(float), FFT_HALF, stf);
            fwrite(w->NR_SNR_post, sizeof(float), FFT_HALF, stf);
            fwrite(w->NR_SNR_prio, sizeof(float), FFT_HALF, stf);
            fwrite(w->NR_Hk_old, sizeof(float), FFT_HALF, stf);
            fwrite(w->NR_G, sizeof(float), FFT_HALF, stf);
        } else if (op != '\n' && op != '#') return 3;
    }
    fwrite(&oob_count, sizeof oob_count, 1, mf);
    fwrite(sqrtHann_256, sizeof(float), 256, mf);
    fclose(outf); fclose(stf); fclose(trf); fclose(mf);
    return 0;
}
