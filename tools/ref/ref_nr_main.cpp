// Developer tool (CPU machine only; tools/make_ref_nr_golden.py builds and runs it): c2s_sound()'s noise-reduction switch
// (rx/rx_sound.cpp:933-949) and the two `SET nr` commands of rx/rx_sound_cmd.cpp (:464-471, their shared declarations :473-475,
// :505-523) as the reference's own statements, cut at build time into a temporary directory.  rx/kiwi/lms.cpp is linked where it
// lies; rx/wdsp/ANR.cpp is #included where it lies (its wdsp_ANR[][] table is file-static, and the end states are read from it).
// Nothing of the reference's text enters the repository; only the data (tests/golden/nr_ref.npz) does.
//
// What this harness adds (no arithmetic): a `switch (cmd_kind)` around the two command cases, the connection start's two
// statements (rx_sound.cpp:236, :240), the stage's enclosing `if (!IQ_or_DRM_or_stereo)` (:923), and never-called stubs for
// NR_SPECTRAL.
//
//   nr_ref script.txt in.bin out.bin
// script lines:
//   A algo                -> "SET nr algo=%d"
//   E type en             -> "SET nr type=%d en=%d"
//   P type param pval     -> "SET nr type=%d param=%d pval=%s" (pval written with 9 significant digits: the float round-trips)
//   C                     -> a new connection: memset(s), s->nr_algo = NR_OFF_
//   B n stereo            -> the stage on the next n int16 of in.bin, IQ_or_DRM_or_stereo = stereo; out: the n int16 after it
//   S                     -> the end state of both types: per type (DENOISE, AUTONOTCH) int32 in_idx, taps, delay, dlp, dlen,
//                            nr_type; float lidx, ngamma; then ANR w[512] and CLMS m_lmscoef[121] (floats)
#define private public           // CLMS's m_dlp / m_dlen / m_nr_type, for the end states only
#include "types.h"           // rx_sound.cpp:20-64 in its own order, as tools/ref/ref_sam_main.cpp
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
#undef private
#undef printf
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include NR_ANR_CPP

snd_t snd_inst[MAX_RX_CHANS];
void nr_spectral_init(int, TYPEREAL *) { abort(); }
void nr_spectral_process(int, int, TYPEMONO16 *, TYPEMONO16 *) { abort(); }

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

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s script in.bin out.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *inf = fopen(argv[2], "rb"), *outf = fopen(argv[3], "wb");
    if (!sf || !inf || !outf) { fprintf(stderr, "cannot open files\n"); return 2; }
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
        } else if (op == 'C') {
            memset(s, 0, sizeof(snd_t)); s->nr_algo = NR_OFF_;
        } else if (op == 'B') {
            int ns_out, stereo;
            if (sscanf(line + 1, "%d %d", &ns_out, &stereo) != 2 || ns_out < 1 || ns_out > 4096) return 3;
            if (fread(out_samps_s2, sizeof(TYPEMONO16), ns_out, inf) != (size_t) ns_out) return 4;
            const bool IQ_or_DRM_or_stereo = stereo != 0;
            if (!IQ_or_DRM_or_stereo) {
#include "NR_CUT_STAGE.inc"
            fwrite(out_samps_s2, sizeof(TYPEMONO16), ns_out, outf);
        } else if (op == 'S') {
            for (int t = 0; t < 2; t++) {
                const wdsp_ANR_t *w = &wdsp_ANR[t][rx_chan];
                const CLMS *m = &m_LMS[rx_chan][t];
                const int iv[6] = {w->in_idx, w->taps, w->delay, m->m_dlp, m->m_dlen, (int) m->m_nr_type};
                const float fv[2] = {w->lidx, w->ngamma};
                fwrite(iv, sizeof iv, 1, outf);
                fwrite(fv, sizeof fv, 1, outf);
                fwrite(w->w, sizeof(float), ANR_DLINE_SIZE, outf);
                fwrite(m->m_lmscoef, sizeof(float), LMSLEN, outf);
            }
        } else if (op != '\n' && op != '#') return 3;
    }
    fclose(outf);
    return 0;
}
