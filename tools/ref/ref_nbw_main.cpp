// Developer tool (CPU machine only; tools/make_ref_nbw_golden.py builds and runs it): NB_WILD as the reference runs it -- the
// noise-blanker switch of c2s_sound()'s post-filter chain (rx/rx_sound.cpp:922-931) and the `SET nb` commands (rx/rx_sound_cmd.cpp
// :454-462, their shared declarations :473-475, :477-503) as the reference's own statements, cut at build time into a temporary
// directory; rx/Teensy/NB_Wild.cpp #included where it lies (nb_Wild[] is file-static, and the end states are read from it);
// rx/CuteSDR/noiseproc.cpp (the NB_STD case of the same command) and the eight CMSIS files NB_Wild.cpp calls linked where they lie.
// Nothing of the reference's text enters the repository; only the data (tests/golden/nbw_ref.npz) does.
//
// What this harness adds:
//   * assert_array_dim COUNTED instead of panicking: a failing one is counted (the builder asserts 0), and the ones with dimension
//     DIM_WBUF are counted apart -- the repair loop runs two of them per coefficient and hit (:199, :202), which gives the hits of a
//     block without touching the file;
//   * the floats a block hands to the int16 conversion (:260), which are locals of nb_Wild_process: the channel's state is saved,
//     nb_Wild_inner is run on a float copy of the block, the state is put back, and then the call site runs;
//   * a `switch` around the command cases, a wf_inst_t's three NB members, the connection start's statement (rx_sound.cpp:236).
//
//   nbw_ref script.txt in.bin out.bin st.bin tr.bin misc.bin frate
// frate is what the NB_STD case of the parameter command hands to SetupBlanker; NB_WILD has no rate.
// script lines:
//   A algo               -> SET nb algo=
//   E type en            -> SET nb type= en=
//   P type param pval    -> SET nb type= param= pval=      (pval as text)
//   C                    -> a new connection: memset(s)
//   B n stereo           -> the next n int16 of in.bin through the call site (IQ_or_DRM_or_stereo = stereo); out: the n int16 after it
//   S                    -> st.bin: int32 taps, impulse_samples, nb_algo, nb_enable[NB_BLANKER]; float thresh; working_buffer[0 .. 120)
//                           with everything from 2 * order + 2 * PL on written as 0
// tr.bin: per B that ran the stage, int32 hits; float largest |sample| handed to the int16 conversion (inf for a NaN).
// misc.bin: int32 failed assert_array_dim count, DIM_WBUF, FASTFIR_OUTBUF_SIZE as the binary holds them.
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
#undef private
#undef printf
#if defined(ARM_MATH_LOOPUNROLL) || defined(ARM_MATH_NEON) || defined(ARM_MATH_MVEF) || defined(ARM_MATH_AUTOVECTORIZE)
#error "the CMSIS routines would not compile in their plain scalar form"
#endif
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int oob_count, wbuf_checks;
#undef assert_array_dim
#define assert_array_dim(ai, dim) \
    do { \
        if (!((ai) >= (0) && (ai) < (dim))) oob_count++; \
        if ((dim) == DIM_WBUF) wbuf_checks++; \
    } while (0)

snd_t snd_inst[MAX_RX_CHANS];
CNoiseProc m_NoiseProc_snd[MAX_RX_CHANS];

#include NB_WILD_CPP

struct wf_nb_t { int nb_enable[NOISE_TYPES]; float nb_param[NOISE_TYPES][NOISE_PARAMS]; bool nb_param_change[NOISE_TYPES]; };

enum { K_ALGO, K_TYPE };
static void nb_cmd(int rx_chan, snd_t *s, wf_nb_t *wf, float frate, int cmd_kind, const char *cmd)
{
    bool did_cmd = false;
    int n;
    switch (cmd_kind == K_ALGO ? CMD_NB_ALGO : CMD_NB_TYPE) {
#include "NBW_CUT_ALGO.inc"
#include "NBW_CUT_DECLS.inc"
#include "NBW_CUT_TYPE.inc"
    default: break;
    }
    (void) n;
    if (!did_cmd) { fprintf(stderr, "command not taken: %s\n", cmd); exit(5); }
}

int main(int argc, char **argv)
{
    if (argc != 8) { fprintf(stderr, "usage: %s script in.bin out.bin st.bin tr.bin misc.bin frate\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *inf = fopen(argv[2], "rb"), *outf = fopen(argv[3], "wb"), *stf = fopen(argv[4], "wb"),
         *trf = fopen(argv[5], "wb"), *mf = fopen(argv[6], "wb");
    if (!sf || !inf || !outf || !stf || !trf || !mf) { fprintf(stderr, "cannot open files\n"); return 2; }
    const int rx_chan = 0;
    const float frate = strtof(argv[7], nullptr);
    snd_t *s = &snd_inst[rx_chan];
    static wf_nb_t wf_inst;
    wf_nb_t *wf = &wf_inst;
    static TYPEMONO16 out_samps_s2[4096];
    static float probe[4096];
    char line[1024], cmd[256];
    memset(s, 0, sizeof(snd_t));                                        // rx_sound.cpp:236
    while (fgets(line, sizeof line, sf)) {
        const char op = line[0];
        if (op == 'A') {
            int a;
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            snprintf(cmd, sizeof cmd, "SET nb algo=%d", a);
            nb_cmd(rx_chan, s, wf, frate, K_ALGO, cmd);
        } else if (op == 'E') {
            int t, e;
            if (sscanf(line + 1, "%d %d", &t, &e) != 2) return 3;
            snprintf(cmd, sizeof cmd, "SET nb type=%d en=%d", t, e);
            nb_cmd(rx_chan, s, wf, frate, K_TYPE, cmd);
        } else if (op == 'P') {
            int t, p;
            char v[64];
            if (sscanf(line + 1, "%d %d %63s", &t, &p, v) != 3) return 3;
            snprintf(cmd, sizeof cmd, "SET nb type=%d param=%d pval=%s", t, p, v);
            nb_cmd(rx_chan, s, wf, frate, K_TYPE, cmd);
        } else if (op == 'C') {
            memset(s, 0, sizeof(snd_t));
            memset(wf, 0, sizeof *wf);
        } else if (op == 'B') {
            int ns_out, stereo;
            if (sscanf(line + 1, "%d %d", &ns_out, &stereo) != 2 || ns_out < 1 || ns_out > 4096) return 3;
            if (fread(out_samps_s2, sizeof(TYPEMONO16), ns_out, inf) != (size_t) ns_out) return 4;
            const bool IQ_or_DRM_or_stereo = stereo != 0;
            const bool runs = !IQ_or_DRM_or_stereo && s->nb_enable[NB_BLANKER] && s->nb_algo == NB_WILD;
            float max_abs = 0;
            if (runs) {                                                 // the floats of :260, on a copy of the state
                const nb_Wild_t keep = nb_Wild[rx_chan];
                for (int i = 0; i < ns_out; i++) probe[i] = out_samps_s2[i];
                nb_Wild_inner(rx_chan, ns_out, probe);
                nb_Wild[rx_chan] = keep;
                for (int i = 0; i < ns_out; i++) {
                    if (probe[i] != probe[i]) max_abs = INFINITY;
                    else if (fabsf(probe[i]) > max_abs) max_abs = fabsf(probe[i]);
                }
            }
            wbuf_checks = 0;
#include "NBW_CUT_STAGE.inc"
            }                                                           // (the cut ends inside `if (!IQ_or_DRM_or_stereo) {`, :923)
            fwrite(out_samps_s2, sizeof(TYPEMONO16), ns_out, outf);
            if (runs) {
                if (nb_Wild[rx_chan].taps < 1 || wbuf_checks % (2 * nb_Wild[rx_chan].taps)) return 8;
                const int hits = wbuf_checks / (2 * nb_Wild[rx_chan].taps);
                fwrite(&hits, sizeof hits, 1, trf);
                fwrite(&max_abs, sizeof max_abs, 1, trf);
            }
        } else if (op == 'S') {
            const nb_Wild_t *w = &nb_Wild[rx_chan];
            const int iv[4] = {w->taps, w->impulse_samples, s->nb_algo, s->nb_enable[NB_BLANKER]};
            const int il = w->impulse_samples | 1, hist = 2 * w->taps + 2 * ((il - 1) / 2);
            float h[120];
            for (int i = 0; i < 120; i++) h[i] = (i < hist && i < DIM_WBUF) ? w->working_buffer[i] : 0.f;
            fwrite(iv, sizeof iv, 1, stf);
            fwrite(&w->thresh, sizeof(float), 1, stf);
            fwrite(h, sizeof h, 1, stf);
        } else if (op != '\n' && op != '#') return 3;
    }
    const int misc[3] = {oob_count, DIM_WBUF, FASTFIR_OUTBUF_SIZE};
    fwrite(misc, sizeof misc, 1, mf);
    fclose(outf); fclose(stf); fclose(trf); fclose(mf);
    return 0;
}
