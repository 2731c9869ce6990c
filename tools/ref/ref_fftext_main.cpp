// Developer tool (CPU machine only; tools/make_ref_fftext_golden.py builds and runs it): the FFT extension as the reference runs it --
// fft_data (extensions/FFT/FFT.cpp:69-191) and fft_msgs (:193-261) with the declarations they need (:17-67), as the reference's own
// statements, cut at build time into a temporary directory.  Nothing of the reference's text enters the repository; only the data
// (tests/golden/fftext_ref.npz) does.  No FFT runs: the blocks handed to fft_data are the caller's.
//
// What this harness adds:
//   * timer_ms() answering a scripted clock; ext_send_msg_data() capturing the 1025-byte message; ext_send_msg() dropping its text;
//   * ext_register_receive_FFT_samps / ext_unregister_receive_FFT_samps keeping the callback, as the extension interface does: a
//     block reaches fft_data only while one is registered;
//   * ext_update_get_sample_rateHz() answering the script's rate; snd_inst[] with the isSAM / mode the script's S line sets;
//   * the command's printf (:238) compiled away.
//
//   fftext_ref script script.txt pool.bin out.bin
//       script lines:  R rate              the sample rate ext_update_get_sample_rateHz answers from here on (%lf)
//                      S run isSAM mode    snd->isSAM and snd->mode (mode.h's number) set, then `SET run=%d`
//                      I itime             `SET itime=%s` with the text as written
//                      C                   `SET clear`
//                      B inst k            fft_data with instance inst and spectrum k of pool.bin (1024 complex floats each), at a clock
//                                          far enough on for the limiter to pass
//       out.bin: per B int32 sent; when sent, int32 bin and 1024 u8.  Then the state: int32 run, instance, bins, reset; float fft_scale,
//       spectrum_scale; double fi, fft_sec, time; int32 ncma[200]; float pwr[200][1024]
//   fftext_ref limiter clocks.bin out.bin
//       `SET run=1`, then one fft_data per u32 clock: int32 sent, u32 last_ms
#include "ext.h"             // FFT.cpp:3-9 in its own order (rx_waterfall.h, which has an fft_t of its own, stays out)
#include "kiwi.h"
#include "mode.h"
#include "misc.h"
#include "cuteSDR.h"
#include "rx_sound.h"
#undef printf
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <vector>

snd_t snd_inst[MAX_RX_CHANS];

static u4_t clock_ms;
u4_t timer_ms() { return clock_ms; }

static double rate_hz;
double ext_update_get_sample_rateHz(int rx_chan) { return rate_hz; }

static ext_receive_FFT_samps_t registered;
static int registered_flags;
void ext_register_receive_FFT_samps(ext_receive_FFT_samps_t func, int rx_chan, int flags) { registered = func; registered_flags = flags; }
void ext_unregister_receive_FFT_samps(int rx_chan) { registered = NULL; }

extern "C" int ext_send_msg(int rx_chan, bool debug, const char *msg, ...) { return 0; }

static int sent;
static u1_t sent_msg[1 + CONV_FFT_SIZE];
int ext_send_msg_data(int rx_chan, bool debug, u1_t cmd, u1_t *bytes, int nbytes)
{
    if (rx_chan != 0 || cmd != 0 || nbytes != (int) sizeof sent_msg) { fprintf(stderr, "unexpected ext_send_msg_data\n"); exit(7); }
    memcpy(sent_msg, bytes, nbytes);
    sent++;
    return 0;
}

#define printf(...) ((void) 0)
#include "FFTEXT_CUT_DECLS.inc"
#include "FFTEXT_CUT_DATA.inc"
#include "FFTEXT_CUT_MSGS.inc"
#undef printf

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

static void msg(const char *text)
{
    char m[256];
    snprintf(m, sizeof m, "%s", text);
    if (!fft_msgs(m, 0)) { fprintf(stderr, "command not taken: %s\n", text); exit(5); }
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s script|limiter ...\n", argv[0]); return 2; }
    const int rx_chan = 0;
    snd_t *s = &snd_inst[rx_chan];
    memset(s, 0, sizeof(snd_t));
    msg("SET ext_server_init");
    fft_t *e = &fft[rx_chan];
    static TYPECPX blk[CONV_FFT_SIZE];
    if (!strcmp(argv[1], "script") && argc == 5) {
        FILE *sf = fopen(argv[2], "r"), *of = fopen(argv[4], "wb");
        if (!sf || !of) return 2;
        const std::vector<unsigned char> pool = slurp(argv[3]);
        const size_t npool = pool.size() / sizeof blk;
        char line[256], cmd[300];
        while (fgets(line, sizeof line, sf)) {
            line[strcspn(line, "\n")] = 0;
            const char op = line[0];
            if (op == 'R') {
                if (sscanf(line + 1, "%lf", &rate_hz) != 1) return 3;
            } else if (op == 'S') {
                int run, sam, mode;
                if (sscanf(line + 1, "%d %d %d", &run, &sam, &mode) != 3) return 3;
                s->isSAM = sam != 0; s->mode = mode;
                snprintf(cmd, sizeof cmd, "SET run=%d", run);
                msg(cmd);
            } else if (op == 'I') {
                snprintf(cmd, sizeof cmd, "SET itime=%s", line + 2);
                msg(cmd);
            } else if (op == 'C') {
                msg("SET clear");
            } else if (op == 'B') {
                int inst;
                unsigned long k;
                if (sscanf(line + 1, "%d %lu", &inst, &k) != 2 || k >= npool) return 3;
                memcpy(blk, pool.data() + k * sizeof blk, sizeof blk);
                clock_ms += 1000;                                       // the limiter passes
                sent = 0;
                if (registered) {
                    if (registered_flags != POST_FILTERED) return 7;
                    registered(rx_chan, inst, POST_FILTERED, CONV_FFT_TO_OUTBUF_RATIO, CONV_FFT_SIZE, blk);
                }
                fwrite(&sent, 4, 1, of);
                if (sent) {
                    const int bin = sent_msg[0];
                    fwrite(&bin, 4, 1, of);
                    fwrite(sent_msg + 1, 1, CONV_FFT_SIZE, of);
                }
            } else if (op != 0 && op != '#') return 3;
        }
        const int iv[4] = {e->run, e->instance, e->bins, e->reset ? 1 : 0};
        const float fv[2] = {e->fft_scale, e->spectrum_scale};
        const double dv[3] = {e->fi, e->fft_sec, e->time};
        fwrite(iv, sizeof iv, 1, of);
        fwrite(fv, sizeof fv, 1, of);
        fwrite(dv, sizeof dv, 1, of);
        fwrite(e->ncma, sizeof e->ncma, 1, of);
        fwrite(e->pwr, sizeof e->pwr, 1, of);
        fclose(of);
        return 0;
    }
    if (!strcmp(argv[1], "limiter")) {
        const std::vector<unsigned char> in = slurp(argv[2]);
        FILE *of = fopen(argv[3], "wb");
        if (!of || in.size() % 4) return 2;
        rate_hz = 12000;
        msg("SET run=1");
        for (size_t k = 0; k < in.size() / 4; k++) {
            memcpy(&clock_ms, in.data() + 4 * k, 4);
            sent = 0;
            registered(rx_chan, e->instance, POST_FILTERED, CONV_FFT_TO_OUTBUF_RATIO, CONV_FFT_SIZE, blk);
            fwrite(&sent, 4, 1, of);
            fwrite(&e->last_ms, 4, 1, of);
        }
        fclose(of);
        return 0;
    }
    return 2;
}
