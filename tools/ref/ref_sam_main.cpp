// Developer tool (CPU machine only; tools/make_ref_sam_golden.py builds and runs it): the twin of oracle/ref/ref_sndpath_main.cpp that
// also reaches the synchronous-AM arm of c2s_sound()'s `switch (s->mode)` (rx/rx_sound.cpp:791-806), which sndpath_ref never selects.
// Same line cuts of rx/rx_sound.cpp (the path 676-908, the payload 1035-1140, the header 1222-1253 and the declarations around them),
// cut at build time into a temporary directory, so the SAM arm, the de-emphasis, the stereo packet branch (SAS / QAM send
// agc_samps_c as IQ payload, :1047-1049) and the header flags run as the reference's own statements; rx/wdsp/SAM_demod.cpp is linked
// where it lies.  Nothing of the reference's text enters the repository; only the data (tests/golden/sam_ref.npz) does.
//
// What this harness adds to the sndpath one (no arithmetic):
//   * `int snd_rate` (config.h:51-52; the server's nominal 12000 / 20250), wdsp_SAM_demod_init(), and the connection's
//     wdsp_SAM_PLL(PLL_MED), wdsp_SAM_PLL(PLL_RESET) (rx_sound.cpp:302-303) after the R line;
//   * a no-op CFastFIR::ProcessData for m_chan_null_FIR: with a channel null the arm hands it agc_samps_c with a NULL output
//     (:804); it only feeds the display spectrum, outside the audio path;
//   * script lines for the SAM commands (below) and the SAM parts of the mode command (rx_sound_cmd.cpp:214-226).
//
//   sam_ref script.txt in.bin out.bin
// script lines: those of ref_sndpath_main.cpp, with M doing the mode command's SAM part (a non-SAM -> SAM transition calls
// wdsp_SAM_PLL(PLL_RESET); s->isChanNull = false), and
//   G type                                         -> wdsp_SAM_PLL(rx_chan, type)                       (`SET sam_pll=`, :444-451)
//   N mparam                                       -> s->SAM_mparam = mparam & MODE_FLAGS_SAM           (:216)
// Output: as sndpath_ref, except that each block's record is 7 floats (the 5 of sndpath_ref, wdsp_SAM_carrier(0), s->isChanNull),
// that a mono SAM-family block appends agc_samps_c (2 n floats) after out_samps_s2, and that a SAS / QAM block's IQ floats are the
// agc_samps_c the packet section sends.
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
#undef printf
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include SND_CUT_GPSCONST
snd_t snd_inst[MAX_RX_CHANS];                    // rx_sound.cpp:87
clk_t clk;                                       // init/clk.cpp:40
int fw_sel, nrx_samps, rx_decim;                 // main.cpp:65, config.h:51-52
CAgc m_Agc[MAX_RX_CHANS];                        // :148-160
CSquelch m_Squelch[MAX_RX_CHANS];
extern CFastFIR m_chan_null_FIR[MAX_RX_CHANS];   // (declared only: see the head of this file)
CFir m_AM_FIR[MAX_RX_CHANS];
CFir m_nfm_deemp_FIR[MAX_RX_CHANS];
CFir m_am_ssb_deemp_FIR[MAX_RX_CHANS];
int S_meter_cal = -13;                           // rx/rx_init.cpp:127, :140, :314
int snd_rate;                                    // config.h:51-52
int CFastFIR::ProcessData(int, int, TYPECPX *, TYPECPX *) { return 0; }     // m_chan_null_FIR (see the head of this file)
ext_users_t ext_users[MAX_RX_CHANS];
dpump_t dpump;
kiwi_t kiwi;
struct rsid_never { void receive(int, TYPEMONO16 *) {} };
static rsid_never m_RsId[MAX_RX_CHANS];          // (see the head of this file)
extern "C" void _TaskWakeup(int, u4_t, void *) {}
static double g_rate;
double ext_update_get_sample_rateHz(int) { return g_rate; }
static float g_tap[2]; static int g_ntap;
static void smeter_hook(int, float v) { if (g_ntap < 2) g_tap[g_ntap] = v; g_ntap++; }

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s script in.bin out.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *inf = fopen(argv[2], "rb"), *outf = fopen(argv[3], "wb");
    if (!sf || !inf || !outf) { fprintf(stderr, "cannot open files\n"); return 2; }
    const int rx_chan = 0;
    snd_t *s = &snd_inst[rx_chan];
    rx_dpump_t *rx = (rx_dpump_t *) calloc(1, sizeof(rx_dpump_t));
    iq_buf_t *iq = (iq_buf_t *) calloc(1, sizeof(iq_buf_t));
    wf_inst_t *wf = (wf_inst_t *) calloc(1, sizeof(wf_inst_t));
    conn_t *conn = (conn_t *) calloc(1, sizeof(conn_t));
    int j;
    static TYPECPX fir_buf[FASTFIR_OUTBUF_SIZE];
    char line[1024];
    double adc_base;
    if (!fgets(line, sizeof line, sf) || sscanf(line, "R %lf %d %d %d %lf", &g_rate, &fw_sel, &nrx_samps, &rx_decim, &adc_base) != 5) return 3;
    clk.adc_clock_base = adc_base;
    snd_rate = fabs(g_rate - 12000.0) < fabs(g_rate - 20250.0) ? 12000 : 20250;
    wdsp_SAM_demod_init();
    std::vector<std::pair<unsigned long long, int> > tq;        // the T lines waiting for their blocks
    ext_users[rx_chan].receive_S_meter = smeter_hook;
    s->compression = 1; s->agc = 1;                              // rx_sound.cpp:237-238
#include SND_CUT_DECLS
#include SND_CUT_PKTINIT
#include SND_CUT_MASKED
#include SND_CUT_OVERLOAD
#include SND_CUT_NORM
    (void) ref_nrx_samps;
    {   // what the firmware-mode switch gave: norm_nrx_samps, and gps_delay2 (a double) as three floats that sum to it
        const float a = (float) gps_delay2, b = (float) (gps_delay2 - (double) a), c = (float) (gps_delay2 - (double) a - (double) b);
        const float cfg[4] = {(float) norm_nrx_samps, a, b, c};
        fwrite(cfg, sizeof(float), 4, outf);
    }
    (void) masked_area; (void) check_masked;
    m_Squelch[rx_chan].SetupParameters(rx_chan, frate);          // rx_sound.cpp:261-262
    m_Squelch[rx_chan].SetSquelch(0, 0);
    s->mode = MODE_USB;
    wdsp_SAM_PLL(rx_chan, PLL_MED);                              // rx_sound.cpp:302-303
    wdsp_SAM_PLL(rx_chan, PLL_RESET);
    while (fgets(line, sizeof line, sf)) {
        const char op = line[0];
        if (op == 'A') {
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
                    const float hdr[7] = {sMeterAvg_dB, sMeter_dBm, g_tap[0], g_tap[1], (float) s->squelched, wdsp_SAM_carrier(rx_chan),
                                          (float) s->isChanNull};
                    fwrite(hdr, sizeof(float), 7, outf);
                    const bool sam = (mode_flags[s->mode] & IS_SAM) != 0;
                    if (!IQ_or_DRM_or_stereo) {
                        for (int i = 0; i < ns_out; i++) { const float v = (float) out_samps_s2[i]; fwrite(&v, sizeof v, 1, outf); }
                        if (sam) fwrite(rx->agc_samples_c, sizeof(TYPECPX), ns_out, outf);
                    }
#include SND_CUT_PACKET
                    if (IQ_or_DRM_or_stereo) fwrite(sam ? rx->agc_samples_c : fir_buf, sizeof(TYPECPX), ns_out, outf);    // what the payload sent
                }
            }
#include SND_CUT_HEADER
            const u1_t *pkt = IQ_or_DRM_or_stereo ? (const u1_t *) &s->out_pkt_iq : (const u1_t *) &s->out_pkt_real;
            const int hsize = IQ_or_DRM_or_stereo ? (int) sizeof(s->out_pkt_iq.h) : (int) sizeof(s->out_pkt_real.h);
            const float sz[2] = {(float) hsize, (float) bc};
            fwrite(sz, sizeof(float), 2, outf);
            for (int i = 0; i < hsize + bc; i++) { const float v = (float) pkt[i]; fwrite(&v, sizeof v, 1, outf); }
        } else if (op != '\n' && op != '#') return 3;
    }
    fclose(outf);
    return 0;
}
