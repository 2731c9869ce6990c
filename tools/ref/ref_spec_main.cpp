// Developer tool (CPU machine only; tools/make_ref_spec_golden.py builds and runs it): the audio spectrum display as the reference
// runs it -- specAF_FFT (rx/rx_sound.cpp:175-220), its call from inside CFastFIR::ProcessData (rx/CuteSDR/fastfir.cpp:247, :251-253,
// :64, :175, :255-272, :301-302, :306-311, :319-323), `SET spc_=` (rx/rx_sound_cmd.cpp:333-337), the mode command's reset (:227-228) and the
// channel-null call site (rx/rx_sound.cpp:802-804), as the reference's own statements, cut at build time into a temporary
// directory.  Nothing of the reference's text enters the repository; only the data (tests/golden/spec_ref.npz) does.  No FFT runs.
//
// What this harness adds:
//   * timer_ms() answering a scripted clock and snd_send_msg_data() capturing the row;
//   * CFastFIR's constructor and ProcessData built from the cuts, with everything between the fill test (:272) and the display
//     call (:301-302) -- both transforms and the multiply -- replaced by copying a block handed in by the caller into m_pFFTBuf:
//     position, fill and the specAF_FFT_post decision are the reference's;
//   * CFastFIR::SetupParameters keeping its instance only (:175), called by the passband command's two statements
//     (rx_sound_cmd.cpp:274-275);
//   * wdsp_SAM_demod() answering what SAM_demod.cpp:176 answers (mode == MODE_SAM && chan_null_which != CHAN_NULL_NONE; pinned by
//     text) and touching no sample;
//   * around :227-228 the condition of :202 and the SAM_mparam statement of :215-216 (pinned by text, restated here).
//
//   spec_ref rows    in.bin out.bin          every 1024-point complex float spectrum of in.bin through specAF_FFT with isChanNull
//                                            false, then true (the clock far enough on for every call to fire): 2 rows of 1024 u8 each
//   spec_ref limiter clocks.bin out.bin      one connection (specAF_last_ms = 0), one call per u32 clock: int32 fired, u32 last_ms
//   spec_ref emit    script.txt blocks.bin out.bin
//       script lines:  P n            `SET spc_=n`
//                      M mode mparam n5   the mode command with _mode = mode (mode.h's number), s->mparam = mparam, n == 5 when n5
//                      B              one 512-sample sound block: m_PassbandFIR, then for the SAM family :802-804
//       blocks.bin: 1024-point complex float blocks, handed out in turn at every fill of either filter
//       out.bin per B: int32 rows, then per row int32 instance, int32 isChanNull at the call, int32 index of the block handed over,
//       1024 u8
#define private public
#include "types.h"           // rx_sound.cpp:20-64 in its own order, as tools/ref/ref_nbw_main.cpp
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
#undef private
#undef printf
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

snd_t snd_inst[MAX_RX_CHANS];

static u4_t clock_ms;
u4_t timer_ms() { return clock_ms; }

static int sent;
static u1_t sent_row[CONV_FFT_SIZE];
void snd_send_msg_data(int rx_chan, bool debug, u1_t cmd, u1_t *bytes, int nbytes)
{
    if (rx_chan != 0 || debug || cmd != 0x00 || nbytes != CONV_FFT_SIZE) { fprintf(stderr, "unexpected snd_send_msg_data\n"); exit(7); }
    memcpy(sent_row, bytes, nbytes);
    sent++;
}

// the reference's function under another name; the one the cuts call records what it was handed first
#define specAF_FFT specAF_FFT_cut
#include "SPEC_CUT_ROW.inc"
#undef specAF_FFT

struct emitted { int instance, chan_null, block; u1_t row[CONV_FFT_SIZE]; };
static std::vector<emitted> rows_out;
static int cur_block = -1;
bool specAF_FFT(int rx_chan, int instance, int flags, int ratio, int ns_out, TYPECPX *samps)
{
    if (flags != POST_FILTERED || ratio != CONV_FFT_TO_OUTBUF_RATIO) { fprintf(stderr, "unexpected specAF_FFT arguments\n"); exit(7); }
    clock_ms += 1000;                                                   // every call fires
    sent = 0;
    const bool r = specAF_FFT_cut(rx_chan, instance, flags, ratio, ns_out, samps);
    if (!r || sent != 1) { fprintf(stderr, "the limiter held a row back\n"); exit(7); }
    emitted e;
    e.instance = instance; e.chan_null = snd_inst[rx_chan].isChanNull ? 1 : 0; e.block = cur_block;
    memcpy(e.row, sent_row, sizeof e.row);
    rows_out.push_back(e);
    return r;
}

// ---- CFastFIR from the cuts, without its transforms
static std::vector<TYPECPX> blocks;                                     // what the fills are handed, in turn
static size_t next_block;

CFastFIR::CFastFIR()
{
    memset(m_pFFTBuf, 0, sizeof m_pFFTBuf);
#include "SPEC_CUT_POS0.inc"
}
CFastFIR::~CFastFIR() {}

void CFastFIR::SetupParameters(int instance, TYPEREAL FLoCut, TYPEREAL FHiCut, TYPEREAL Offset, TYPEREAL SampleRate)
{
#include "SPEC_CUT_SETUP.inc"
}

int CFastFIR::ProcessData(int rx_chan, int InLength, TYPECPX *InBuf, TYPECPX *OutBuf)
{
#include "SPEC_CUT_INST.inc"
#include "SPEC_CUT_POST.inc"
#include "SPEC_CUT_LOOP.inc"
            (void) j;
            if (next_block >= blocks.size() / CONV_FFT_SIZE) { fprintf(stderr, "blocks.bin is too short\n"); exit(4); }
            cur_block = (int) next_block;
            memcpy(m_pFFTBuf, &blocks[next_block++ * CONV_FFT_SIZE], sizeof m_pFFTBuf);        // :274-297: the filtered spectrum
#include "SPEC_CUT_CALL.inc"
#include "SPEC_CUT_OUT.inc"
#include "SPEC_CUT_TAIL.inc"
}

CFastFIR m_PassbandFIR[MAX_RX_CHANS];
CFastFIR m_chan_null_FIR[MAX_RX_CHANS];

static int demod_calls;
bool wdsp_SAM_demod(int rx_chan, int mode, u4_t SAM_mparam, int ns_out, TYPECPX *in, TYPEMONO16 *out)
{
    demod_calls++;
    return mode == MODE_SAM && (SAM_mparam & CHAN_NULL_WHICH) != CHAN_NULL_NONE;     // SAM_demod.cpp:176, :355
}

static void spc_cmd(snd_t *s, const char *cmd)
{
    bool did_cmd = false;
    int n;
#include "SPEC_CUT_CMD.inc"
        }
    if (!did_cmd) { fprintf(stderr, "command not taken: %s\n", cmd); exit(5); }
}

// the passband command designs both filters (rx_sound_cmd.cpp:274-275): what matters here is the instance each is given
static void passband_cmd(int rx_chan, snd_t *s, float frate)
{
#define CW_OFFSET 0
#include "SPEC_CUT_DESIGN.inc"
}

static void mode_cmd(snd_t *s, int _mode, int mparam, int n)
{
    s->mparam = mparam;
    if (s->mode != _mode || n == 5) {                                   // rx_sound_cmd.cpp:202
        s->isSAM = mode_flags[_mode] & IS_SAM;                          // :214
        if (s->isSAM && n == 5) s->SAM_mparam = s->mparam & MODE_FLAGS_SAM;     // :215-216
#include "SPEC_CUT_CLEAR.inc"
        s->mode = _mode;                                                // :230
    }
}

static std::vector<unsigned char> slurp(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<unsigned char> v;
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s rows|limiter|emit ...\n", argv[0]); return 2; }
    const int rx_chan = 0;
    snd_t *s = &snd_inst[rx_chan];
    memset(s, 0, sizeof(snd_t));                                        // rx_sound.cpp:236
    if (!strcmp(argv[1], "rows")) {
        const std::vector<unsigned char> in = slurp(argv[2]);
        FILE *of = fopen(argv[3], "wb");
        if (!of || in.size() % (CONV_FFT_SIZE * sizeof(TYPECPX))) return 2;
        for (size_t r = 0; r < in.size() / (CONV_FFT_SIZE * sizeof(TYPECPX)); r++)
            for (int null = 0; null < 2; null++) {
                s->isChanNull = null != 0;
                rows_out.clear();
                specAF_FFT(rx_chan, null, POST_FILTERED, CONV_FFT_TO_OUTBUF_RATIO, CONV_FFT_SIZE, (TYPECPX *) in.data() + r * CONV_FFT_SIZE);
                fwrite(rows_out[0].row, 1, CONV_FFT_SIZE, of);
            }
        fclose(of);
        return 0;
    }
    if (!strcmp(argv[1], "limiter")) {
        const std::vector<unsigned char> in = slurp(argv[2]);
        FILE *of = fopen(argv[3], "wb");
        if (!of || in.size() % 4) return 2;
        static TYPECPX zero[CONV_FFT_SIZE];
        for (size_t k = 0; k < in.size() / 4; k++) {
            memcpy(&clock_ms, in.data() + 4 * k, 4);
            sent = 0;
            const int fired = specAF_FFT_cut(rx_chan, 0, POST_FILTERED, CONV_FFT_TO_OUTBUF_RATIO, CONV_FFT_SIZE, zero) ? 1 : 0;
            if (fired != sent) return 7;
            fwrite(&fired, 4, 1, of);
            fwrite(&s->specAF_last_ms, 4, 1, of);
        }
        fclose(of);
        return 0;
    }
    if (!strcmp(argv[1], "emit") && argc == 5) {
        FILE *sf = fopen(argv[2], "r"), *of = fopen(argv[4], "wb");
        if (!sf || !of) return 2;
        const std::vector<unsigned char> in = slurp(argv[3]);
        blocks.resize(in.size() / sizeof(TYPECPX));
        memcpy(blocks.data(), in.data(), blocks.size() * sizeof(TYPECPX));
        s->mode = -1;                                                   // rx_sound.cpp:237
        s->locut = 300; s->hicut = 2700;
        passband_cmd(rx_chan, s, 12000.f);
        static TYPECPX samps[FASTFIR_OUTBUF_SIZE], fir_out[2 * FASTFIR_OUTBUF_SIZE], agc_buf[FASTFIR_OUTBUF_SIZE];
        static TYPEMONO16 out_samps_s2[FASTFIR_OUTBUF_SIZE];
        char line[256], cmd[256];
        while (fgets(line, sizeof line, sf)) {
            const char op = line[0];
            if (op == 'P') {
                int n;
                if (sscanf(line + 1, "%d", &n) != 1) return 3;
                snprintf(cmd, sizeof cmd, "SET spc_=%d", n);
                spc_cmd(s, cmd);
            } else if (op == 'M') {
                int m, mp, n5;
                if (sscanf(line + 1, "%d %d %d", &m, &mp, &n5) != 3) return 3;
                mode_cmd(s, m, mp, n5 ? 5 : 4);
            } else if (op == 'B') {
                rows_out.clear();
                const int ns_out = m_PassbandFIR[rx_chan].ProcessData(rx_chan, FASTFIR_OUTBUF_SIZE, samps, fir_out);
                if (ns_out != FASTFIR_OUTBUF_SIZE) return 8;
                if (mode_flags[s->mode] & IS_SAM) {                     // rx_sound.cpp:791-797
                    TYPECPX *agc_samps_c = agc_buf;
#include "SPEC_CUT_SAM.inc"
                }
                const int nr = (int) rows_out.size();
                fwrite(&nr, 4, 1, of);
                for (const emitted &e : rows_out) {
                    const int iv[3] = {e.instance, e.chan_null, e.block};
                    fwrite(iv, sizeof iv, 1, of);
                    fwrite(e.row, 1, sizeof e.row, of);
                }
            } else if (op != '\n' && op != '#') return 3;
        }
        fclose(of);
        return 0;
    }
    return 2;
}
