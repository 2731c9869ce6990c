// Developer tool (CPU machine only; tools/make_ref_post_golden.py builds and runs it): c2s_sound()'s body from
// `s_samps_c = fir_samps_c` down to the end of the noise-reduction switch (rx/rx_sound.cpp:676-949) as ONE program with every stage
// linked: tools/ref/ref_sam_main.cpp (the path 676-908 with the S-meter, CAgc, the AM / NBFM / SSB / IQ / SAM-family arms, the CFir
// tails, the squelch, the de-emphasis, the payload section that runs the AGC of an IQ block) with, cut in behind the path cut, the
// Wild stage (:922-931) and the NR switch (:933-949), and their command cuts of rx/rx_sound_cmd.cpp (`SET nb` :454-462, :473-475,
// :477-503; `SET nr` :464-471, :505-523; the normalised passband :252-266) as tools/ref/ref_nbw_main.cpp, ref_nr_main.cpp and
// ref_nrs_main.cpp have them.  All cuts are made at build time into a temporary directory; rx/wdsp/SAM_demod.cpp, rx/kiwi/lms.cpp,
// rx/CuteSDR/noiseproc.cpp and the CMSIS files are linked where they lie, rx/wdsp/ANR.cpp, rx/Teensy/NB_Wild.cpp and
// rx/Teensy/NR_spectral.cpp #included where they lie (their tables are file-static, and the end states are read from them).
// Nothing of the reference's text enters the repository; only the data (tests/golden/post_rand_ref.npz) does.
//
// What this harness adds (no arithmetic): what ref_sam_main.cpp adds; ref_nrs_main.cpp's two transform tables (twiddles from tw.bin,
// the bit-reversal pairs made here); assert_array_dim COUNTED instead of panicking (the builder asserts 0 failures; the checks made
// while the Wild stage runs give its hits, two per coefficient and hit); `switch`es around the command cases; a copy of out_samps_s2
// taken between :908 and :922.
//
//   post_ref script.txt in.bin tw.bin out.bin st.bin
// script lines: those of ref_sam_main.cpp (R A L Q E M G N W V C T P), and
//   nbA algo / nbE type en / nbP type param pval      -> SET nb algo= / SET nb type= en= / SET nb type= param= pval=
//   nrA algo / nrE type en / nrP type param pval      -> SET nr ...
//   nrM locut hicut                                   -> s->locut, s->hicut (already clamped), then rx_sound_cmd.cpp:252-266
// out.bin, per block: 7 floats (sMeterAvg_dB, sMeter_dBm, the two taps, s->squelched, wdsp_SAM_carrier, s->isChanNull); int32 hits of
// the Wild stage (-1 where it did not run); a mono block: out_samps_s2 before :922 and after :949 (n int16 each); a stereo or
// SAM-family block: agc_samps_c (2 n floats; an IQ block's is what the payload section's AGC wrote).
// st.bin, at the script's end: int32 m_WindowSamples, m_DelaySamples, failed assert_array_dim count; then the S records of
// ref_nr_main.cpp (both types), ref_nbw_main.cpp and ref_nrs_main.cpp.
#define private public           // CAgc's m_WindowSamples, CLMS's m_dlp / m_dlen / m_nr_type: echoes and end states only
#include "types.h"           // rx_sound.cpp:20-64 in its own order (rsid.h, the RSID decoder's DRM resampler headers, left out)
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
#if defined(ARM_MATH_LOOPUNROLL) || defined(ARM_MATH_NEON) || defined(ARM_MATH_MVEF) || defined(ARM_MATH_AUTOVECTORIZE)
#error "the CMSIS routines would not compile in their plain scalar form"
#endif
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int oob_count, dim_checks;     // dim_checks: the checks against DIM_WBUF (NB_Wild.cpp:199, :202: two per coefficient and hit)
#undef assert_array_dim
#define assert_array_dim(ai, dim) \
    do { \
        if (!((ai) >= (0) && (ai) < (dim))) oob_count++; \
        if ((dim) == DIM_WBUF) dim_checks++; \
    } while (0)
#undef assert
#define assert(e) do { if (!(e)) { fprintf(stderr, "assert %s\n", #e); exit(7); } } while (0)

#include SND_CUT_GPSCONST
snd_t snd_inst[MAX_RX_CHANS];                    // rx_sound.cpp:87
clk_t clk;                                       // init/clk.cpp:40
int fw_sel, nrx_samps, rx_decim;                 // main.cpp:65, config.h:51-52
CAgc m_Agc[MAX_RX_CHANS];                        // :148-160
CSquelch m_Squelch[MAX_RX_CHANS];
extern CFastFIR m_chan_null_FIR[MAX_RX_CHANS];   // (declared only: see the head of ref_sam_main.cpp)
CFir m_AM_FIR[MAX_RX_CHANS];
CFir m_nfm_deemp_FIR[MAX_RX_CHANS];
CFir m_am_ssb_deemp_FIR[MAX_RX_CHANS];
CNoiseProc m_NoiseProc_snd[MAX_RX_CHANS];
int S_meter_cal = -13;                           // rx/rx_init.cpp:127, :140, :314
int snd_rate;                                    // config.h:51-52
int CFastFIR::ProcessData(int, int, TYPECPX *, TYPECPX *) { return 0; }     // m_chan_null_FIR
ext_users_t ext_users[MAX_RX_CHANS];
dpump_t dpump;
kiwi_t kiwi;
struct rsid_never { void receive(int, TYPEMONO16 *) {} };
static rsid_never m_RsId[MAX_RX_CHANS];
extern "C" void _TaskWakeup(int, u4_t, void *) {}
static double g_rate;
double ext_update_get_sample_rateHz(int) { return g_rate; }
static float g_tap[2]; static int g_ntap;
static void smeter_hook(int, float v) { if (g_ntap < 2) g_tap[g_ntap] = v; g_ntap++; }

static float tw512[1024];
static uint16_t br512[448];
extern "C" { const arm_cfft_instance_f32 arm_cfft_sR_f32_len512 = {512, tw512, br512, 448}; }

#include NB_WILD_CPP
#include NR_ANR_CPP
#include NR_SPECTRAL_CPP

static int rev3(int i) { return ((i & 7) << 6) | (i & 0x38) | (i >> 6); }

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
    if (argc != 6) { fprintf(stderr, "usage: %s script in.bin tw.bin out.bin st.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *inf = fopen(argv[2], "rb"), *twf = fopen(argv[3], "rb"), *outf = fopen(argv[4], "wb"),
         *stf = fopen(argv[5], "wb");
    if (!sf || !inf || !twf || !outf || !stf) { fprintf(stderr, "cannot open files\n"); return 2; }
    if (fread(tw512, sizeof(float), 1024, twf) != 1024) return 2;
    int nbr = 0;
    for (int i = 0; i < 512; i++)
        if (i < rev3(i)) { br512[nbr++] = (uint16_t) (8 * i); br512[nbr++] = (uint16_t) (8 * rev3(i)); }
    if (nbr != 448) return 2;
    const int rx_chan = 0;
    snd_t *s = &snd_inst[rx_chan];
    rx_dpump_t *rx = (rx_dpump_t *) calloc(1, sizeof(rx_dpump_t));
    iq_buf_t *iq = (iq_buf_t *) calloc(1, sizeof(iq_buf_t));
    wf_inst_t *wf = (wf_inst_t *) calloc(1, sizeof(wf_inst_t));
    conn_t *conn = (conn_t *) calloc(1, sizeof(conn_t));
    static wf_nb_t wf_nb;
    int j;
    static TYPECPX fir_buf[FASTFIR_OUTBUF_SIZE];
    static TYPEMONO16 pre_s2[FASTFIR_OUTBUF_SIZE];
    char line[1024], cmd[256];
    double adc_base;
    if (!fgets(line, sizeof line, sf) || sscanf(line, "R %lf %d %d %d %lf", &g_rate, &fw_sel, &nrx_samps, &rx_decim, &adc_base) != 5) return 3;
    clk.adc_clock_base = adc_base;
    snd_rate = fabs(g_rate - 12000.0) < fabs(g_rate - 20250.0) ? 12000 : 20250;
    wdsp_SAM_demod_init();
    std::vector<std::pair<unsigned long long, int> > tq;        // the T lines waiting for their blocks
    ext_users[rx_chan].receive_S_meter = smeter_hook;
    memset(s, 0, sizeof(snd_t)); s->nr_algo = NR_OFF_;           // rx_sound.cpp:236, :240
    s->compression = 1; s->agc = 1;                              // rx_sound.cpp:237-238
#include SND_CUT_DECLS
#include SND_CUT_PKTINIT
#include SND_CUT_MASKED
#include SND_CUT_OVERLOAD
#include SND_CUT_NORM
    (void) ref_nrx_samps; (void) gps_delay2;
    (void) masked_area; (void) check_masked;
    m_Squelch[rx_chan].SetupParameters(rx_chan, frate);          // rx_sound.cpp:261-262
    m_Squelch[rx_chan].SetSquelch(0, 0);
    s->mode = MODE_USB;
    wdsp_SAM_PLL(rx_chan, PLL_MED);                              // rx_sound.cpp:302-303
    wdsp_SAM_PLL(rx_chan, PLL_RESET);
    while (fgets(line, sizeof line, sf)) {
        const char op = line[0];
        if (!strncmp(line, "nbA", 3)) {
            int a;
            if (sscanf(line + 3, "%d", &a) != 1) return 3;
            snprintf(cmd, sizeof cmd, "SET nb algo=%d", a);
            nb_cmd(rx_chan, s, &wf_nb, frate, K_ALGO, cmd);
        } else if (!strncmp(line, "nbE", 3)) {
            int t, e;
            if (sscanf(line + 3, "%d %d", &t, &e) != 2) return 3;
            snprintf(cmd, sizeof cmd, "SET nb type=%d en=%d", t, e);
            nb_cmd(rx_chan, s, &wf_nb, frate, K_TYPE, cmd);
        } else if (!strncmp(line, "nbP", 3)) {
            int t, p;
            char v[64];
            if (sscanf(line + 3, "%d %d %63s", &t, &p, v) != 3) return 3;
            snprintf(cmd, sizeof cmd, "SET nb type=%d param=%d pval=%s", t, p, v);
            nb_cmd(rx_chan, s, &wf_nb, frate, K_TYPE, cmd);
        } else if (!strncmp(line, "nrA", 3)) {
            int a;
            if (sscanf(line + 3, "%d", &a) != 1) return 3;
            snprintf(cmd, sizeof cmd, "SET nr algo=%d", a);
            nr_cmd(rx_chan, s, K_ALGO, cmd);
        } else if (!strncmp(line, "nrE", 3)) {
            int t, e;
            if (sscanf(line + 3, "%d %d", &t, &e) != 2) return 3;
            snprintf(cmd, sizeof cmd, "SET nr type=%d en=%d", t, e);
            nr_cmd(rx_chan, s, K_TYPE, cmd);
        } else if (!strncmp(line, "nrP", 3)) {
            int t, p;
            char v[64];
            if (sscanf(line + 3, "%d %d %63s", &t, &p, v) != 3) return 3;
            snprintf(cmd, sizeof cmd, "SET nr type=%d param=%d pval=%s", t, p, v);
            nr_cmd(rx_chan, s, K_TYPE, cmd);
        } else if (!strncmp(line, "nrM", 3)) {
            double lo, hi;
            if (sscanf(line + 3, "%lf %lf", &lo, &hi) != 2) return 3;
            s->locut = lo; s->hicut = hi;
            passband(s);
        } else if (op == 'A') {
            int on, hang, thr, man, slope, decay;
            if (sscanf(line + 1, "%d %d %d %d %d %d", &on, &hang, &thr, &man, &slope, &decay) != 6) return 3;
            s->agc = on;                                         // rx_sound_cmd.cpp:343
            m_Agc[rx_chan].SetParameters(on, hang, thr, man, slope, decay, frate);
        } else if (op == 'L') {
            float hbw, stop;
            if (sscanf(line + 1, "%f %f", &hbw, &stop) != 2) return 3;
            m_AM_FIR[rx_chan].InitLPFilter(0, 1.0, 50.0, hbw, stop, frate);
        } else if (op == 'Q') {
            int v, mx;
            if (sscanf(line + 1, "%d %d", &v, &mx) != 2) return 3;
            m_Squelch[rx_chan].SetSquelch(v, mx);
        } else if (op == 'E') {
            int de, de_nfm;
            if (sscanf(line + 1, "%d %d", &de, &de_nfm) != 2) return 3;
            s->deemp = de; s->deemp_nfm = de_nfm;
            const bool r12k = fabs(frate - 12000.0) < fabs(frate - 20250.0);         // snd_rate == SND_RATE_4CH
            if (de)     m_am_ssb_deemp_FIR[rx_chan].InitConstFir(N_DEEMP_TAPS, r12k ? am_ssb_deemp_12000[de - 1] : am_ssb_deemp_20250[de - 1], frate);
            if (de_nfm) m_nfm_deemp_FIR[rx_chan].InitConstFir(N_DEEMP_TAPS, r12k ? nfm_deemp_12000[de_nfm - 1] : nfm_deemp_20250[de_nfm - 1], frate);
        } else if (op == 'M') {
            int mode;
            if (sscanf(line + 1, "%d", &mode) != 1) return 3;
            if ((mode_flags[mode] & IS_SAM) && (mode_flags[s->mode] & IS_SAM) == 0) wdsp_SAM_PLL(rx_chan, PLL_RESET);   // rx_sound_cmd.cpp:222-225
            s->isChanNull = false;
            s->mode = mode;
        } else if (op == 'G') {
            int type;
            if (sscanf(line + 1, "%d", &type) != 1) return 3;
            wdsp_SAM_PLL(rx_chan, type);
        } else if (op == 'N') {
            unsigned mp;
            if (sscanf(line + 1, "%u", &mp) != 1) return 3;
            s->SAM_mparam = mp & MODE_FLAGS_SAM;
        } else if (op == 'W') {
            int comp, le;
            if (sscanf(line + 1, "%d %d", &comp, &le) != 2) return 3;
            s->compression = comp; s->little_endian = le != 0;
        } else if (op == 'V') {
            int ov;
            if (sscanf(line + 1, "%d", &ov) != 1) return 3;
            dpump.rx_adc_ovfl = ov;
        } else if (op == 'C') {
            unsigned long long t; double secs;
            if (sscanf(line + 1, "%llu %lf", &t, &secs) != 2) return 3;
            clk.ticks = t; clk.gps_secs = secs;
        } else if (op == 'T') {
            unsigned long long t; int fp;
            if (sscanf(line + 1, "%llu %d", &t, &fp) != 2) return 3;
            tq.push_back(std::make_pair(t, fp));
        } else if (op == 'P') {
            // one pass of the `while (TRUE)` loop of c2s_sound() from :459 on: one packet
#include SND_CUT_FLAGS
#include SND_CUT_HOOKS
            (void) isDRM; (void) receive_iq_pre_fir; (void) receive_iq_pre_agc; (void) receive_iq_pre_agc_tid; (void) bp_real_s2; (void) bp_iq_s2;
            int ns_out;
            char *q = line + 1;
            for (;;) {                                           // do { ... } while (bc < LOOP_BC): the script's block list
                char *e;
                ns_out = (int) strtol(q, &e, 10);
                if (e == q) break;
                q = e;
                if (ns_out < 1 || ns_out > FASTFIR_OUTBUF_SIZE) return 3;
                if (fread(fir_buf, sizeof(TYPECPX), ns_out, inf) != (size_t) ns_out) return 4;
                TYPECPX *fir_samps_c = fir_buf;
                g_ntap = 0; g_tap[0] = g_tap[1] = 0;
                int fir_pos = 0;
                rx->rd_pos = 0; rx->ticks[0] = 0;
                if (!tq.empty()) { rx->ticks[0] = tq.front().first; fir_pos = tq.front().second; tq.erase(tq.begin()); }
                {
#include SND_CUT_TICKS
#include SND_CUT_GPSSEC
#include SND_CUT_GPSSTAMP
                    (void) dt_to_pos_sol;
#include SND_CUT_PATH
                    if (!IQ_or_DRM_or_stereo) memcpy(pre_s2, out_samps_s2, ns_out * sizeof(TYPEMONO16));
                    const bool wild = !IQ_or_DRM_or_stereo && s->nb_enable[NB_BLANKER] && s->nb_algo == NB_WILD;
                    int wild_checks = 0;
                    dim_checks = 0;
#include "NBW_CUT_STAGE.inc"
                    wild_checks = dim_checks;                    // (inside `if (!IQ_or_DRM_or_stereo) {`, :923, which the next cut closes)
#include "NR_CUT_STAGE.inc"
                    int hits = -1;
                    if (wild) {
                        if (nb_Wild[rx_chan].taps < 1 || wild_checks % (2 * nb_Wild[rx_chan].taps)) return 8;
                        hits = wild_checks / (2 * nb_Wild[rx_chan].taps);
                    }
                    const bool sam = (mode_flags[s->mode] & IS_SAM) != 0;
#include SND_CUT_PACKET
                    const float hdr[7] = {sMeterAvg_dB, sMeter_dBm, g_tap[0], g_tap[1], (float) s->squelched, wdsp_SAM_carrier(rx_chan),
                                          (float) s->isChanNull};
                    fwrite(hdr, sizeof(float), 7, outf);
                    fwrite(&hits, sizeof hits, 1, outf);
                    if (!IQ_or_DRM_or_stereo) {
                        fwrite(pre_s2, sizeof(TYPEMONO16), ns_out, outf);
                        fwrite(out_samps_s2, sizeof(TYPEMONO16), ns_out, outf);
                    }
                    if (IQ_or_DRM_or_stereo || sam) fwrite(sam ? rx->agc_samples_c : fir_buf, sizeof(TYPECPX), ns_out, outf);
                }
            }
        } else if (op != '\n' && op != '#') return 3;
    }
    {
        const int echo[3] = {m_Agc[rx_chan].m_WindowSamples, m_Agc[rx_chan].GetDelaySamples(), oob_count};
        fwrite(echo, sizeof echo, 1, stf);
        for (int t = 0; t < 2; t++) {                            // ref_nr_main.cpp's S record
            const wdsp_ANR_t *w = &wdsp_ANR[t][rx_chan];
            const CLMS *m = &m_LMS[rx_chan][t];
            const int iv[6] = {w->in_idx, w->taps, w->delay, m->m_dlp, m->m_dlen, (int) m->m_nr_type};
            const float fv[2] = {w->lidx, w->ngamma};
            fwrite(iv, sizeof iv, 1, stf);
            fwrite(fv, sizeof fv, 1, stf);
            fwrite(w->w, sizeof(float), ANR_DLINE_SIZE, stf);
            fwrite(m->m_lmscoef, sizeof(float), LMSLEN, stf);
        }
        {                                                        // ref_nbw_main.cpp's
            const nb_Wild_t *w = &nb_Wild[rx_chan];
            const int iv[4] = {w->taps, w->impulse_samples, s->nb_algo, s->nb_enable[NB_BLANKER]};
            const int il = w->impulse_samples | 1, hist = 2 * w->taps + 2 * ((il - 1) / 2);
            float h[120];
            for (int i = 0; i < 120; i++) h[i] = (i < hist && i < DIM_WBUF) ? w->working_buffer[i] : 0.f;
            fwrite(iv, sizeof iv, 1, stf);
            fwrite(&w->thresh, sizeof(float), 1, stf);
            fwrite(h, sizeof h, 1, stf);
        }
        {                                                        // ref_nrs_main.cpp's
            const nr_spectral_t *w = &nr_spectral[rx_chan];
            const int iv[2] = {w->first_time, w->init_counter};
            const float fv[12] = {w->final_gain, w->alpha, w->asnr, w->xih1r, w->pfac, tinc, tax, tap, ax, ap, s->norm_locut, s->norm_hicut};
            fwrite(iv, sizeof iv, 1, stf);
            fwrite(fv, sizeof fv, 1, stf);
            const float *arr[9] = {w->last_sample_buffer, w->last_iFFT_result, w->NR_Nest, w->xt, w->pslp, w->NR_SNR_post, w->NR_SNR_prio,
                                   w->NR_Hk_old, w->NR_G};
            for (int a = 0; a < 9; a++) fwrite(arr[a], sizeof(float), FFT_HALF, stf);
        }
    }
    fclose(outf); fclose(stf);
    return 0;
}
