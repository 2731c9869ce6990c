// Developer tool (CPU machine only; tools/make_ref_cw_golden.py builds and runs it): the CW decoder extension as the reference runs it
// -- extensions/CW_decoder/uhsdr_cw_decoder.cpp:50-1296, the defines, the struct, the code table and every function from
// AudioFilter_CalcGoertzel through CW_Decode, as the reference's own statements, cut at build time into a temporary directory.  Nothing
// of the reference's text enters the repository; only the data (tests/golden/cw_ref.npz) does.
//
// What this harness adds (none of the reference's headers is used):
//   * float32_t, u4_t, TYPEMONO16, K_PI, CLAMP, ARRAY_LEN, SPACE_FOR_NULL, TRUE / FALSE, MAX_RX_CHANS and the two block sizes as the
//     pinned lines have them; printf inside the cut is swallowed;
//   * snd_rate and ext_update_get_sample_rateHz() from the script's S line, timer_sec() from its N lines, NextTask() counting which
//     corrective branch of ErrorCorrectionFunc an error took (from where sig_outcount stands behind the first reprocessed state);
//   * ext_send_msg() and ext_send_msg_encoded() recording the events of include/kiwigpu.h (kg_cw_ev);
//   * the commands of cw_decoder_msgs (cw_decoder.cpp:135-211) restated from the pinned lines.  The samples go in ONE at a time
//     (CwDecode_RxProcessor loops over them without state of its own), which tells in which Goertzel block an event arose.
//
//   cw_ref script.txt pool.bin out.bin
//       script lines:  S training_interval nom srate   `SET cw_start=` / `SET cw_train=` (snd_rate and the receiver's rate as given)
//                      W wpm training_interval          `SET cw_wpm=`
//                      P pboff | C wsc | A on | H threshold       `SET cw_pboff=`, `cw_wsc=`, `cw_auto_thresh=`, `cw_threshold=`
//                      T                                `SET cw_stop`
//                      N now_sec                        what timer_sec() answers from here on
//                      B off                            CwDecode_RxProcessor(pool + off, 512) (pool.bin: int16)
//       out.bin: per B int32 events, per event 6 int32 (blk = 0, gblk: the Goertzel block among those the sound block completed, kind,
//       a, b, c).  Then the state (kg_cw_info of include/kiwigpu.h), then 8 int32: errors that took the first corrective branch, those
//       of them that succeeded, the same for the second branch, over-long characters, and three zeros.
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

typedef float float32_t;
typedef unsigned int u4_t;
typedef short TYPEMONO16;
#define K_PI (3.14159265358979323846)
#define CLAMP(a, min, max) (((a) < (min)) ? (min) : (((a) > (max)) ? (max) : (a)))
#define ARRAY_LEN(x) ((int) (sizeof(x) / sizeof((x)[0])))
#define SPACE_FOR_NULL 1
#define TRUE 1
#define FALSE 0
#define MAX_RX_CHANS 1
#define CW_DECODER_BLOCKSIZE_MAX 128
#define CW_DECODER_BLOCKSIZE_DEFAULT 88

enum { EV_CHARS = 0, EV_WPM = 1, EV_TRAIN = 2, EV_PLOT = 3 };
static int snd_rate;
static double cur_srate;
static u4_t now_sec;
static int gblk;
static bool in_block;
static std::vector<int32_t> sent;
static int nev;
static int branch_seen, stats[8];
static long total_exe;                         // `static int slowdown` (:519) is not reachable from outside: it is this count modulo 3
static int slowdown_of() { return (int) (total_exe % 3); }
static const char *const prosigns[12] = {"<aa>", "<ar>", "<as>", "<bk>", "<bt>", "<cl>", "<ct>", "<hh>", "<kn>", "<nj>", "<sk>", "<sn>"};

static double ext_update_get_sample_rateHz(int) { return cur_srate; }
static u4_t timer_sec() { return now_sec; }
static void NextTask(const char *);

static void event(int kind, int32_t a, int32_t b, int32_t c)
{
    if (!in_block) return;                      // the `EXT cw_train=0` of a fixed-WPM CwDecode_Init (:385): implied by the command
    const int32_t r[6] = {0, gblk, kind, a, b, c};
    sent.insert(sent.end(), r, r + 6);
    nev++;
}
static int32_t bits(float f) { int32_t i; memcpy(&i, &f, 4); return i; }
static int ext_send_msg(int, bool, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    if (!strcmp(fmt, "EXT cw_train=%d")) event(EV_TRAIN, va_arg(ap, int), 0, 0);
    else if (!strcmp(fmt, "EXT cw_train=0")) event(EV_TRAIN, 0, 0, 0);
    else if (!strcmp(fmt, "EXT cw_wpm=%d")) event(EV_WPM, va_arg(ap, int), 0, 0);
    else if (!strcmp(fmt, "EXT cw_plot=%.2f,%d,%.2f")) {
        const float dB = (float) va_arg(ap, double);                   // both were floats before the promotion: exact
        const int flag = va_arg(ap, int);
        const float thr = (float) va_arg(ap, double);
        event(EV_PLOT, bits(dB), flag, bits(thr));
    } else { fprintf(stderr, "unexpected ext_send_msg %s\n", fmt); exit(7); }
    va_end(ap);
    return 0;
}
static int ext_send_msg_encoded(int, bool, const char *dst, const char *cmd, const char *s)
{
    if (strcmp(dst, "EXT") || strcmp(cmd, "cw_chars")) { fprintf(stderr, "unexpected ext_send_msg_encoded %s %s\n", dst, cmd); exit(7); }
    int code = -1;
    if (!strcmp(s, "[err]")) code = 0xff;
    else if (s[0] == '<') { for (int i = 0; i < 12; i++) if (!strcmp(s, prosigns[i])) code = i; }
    else if (s[0] && !s[1]) code = (unsigned char) s[0];
    if (code < 0) { fprintf(stderr, "unexpected cw_chars %s\n", s); exit(7); }
    event(EV_CHARS, code, 0, 0);
    return 0;
}

#define printf(...) ((void) 0)
#include "CW_CUT_ALL.inc"
#undef printf

static void NextTask(const char *)
{
    if (branch_seen) return;
    cw_decoder_t *cw = &cw_decoder[0];
    const int d = (cw->sig_outcount - cw->last_outcount) & (CW_SIG_BUFSIZE - 1);
    branch_seen = d == 1 ? 2 : 1;               // :1184 restarts at last_outcount, :1149 two behind it
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
    if (argc != 4) { fprintf(stderr, "usage: %s script.txt pool.bin out.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *of = fopen(argv[3], "wb");
    if (!sf || !of) return 2;
    std::vector<unsigned char> pool = slurp(argv[2]);
    const size_t npool = pool.size() / sizeof(short);
    cw_decoder_t *cw = &cw_decoder[0];
    bool capture = false;
    char line[256];
    while (fgets(line, sizeof line, sf)) {
        line[strcspn(line, "\n")] = 0;
        const char op = line[0];
        int a, b;
        double nom, sr;
        if (op == 0 || op == '#') {
        } else if (op == 'S') {
            if (sscanf(line + 1, "%d %lf %lf", &a, &nom, &sr) != 3) return 3;
            snd_rate = (int) nom; cur_srate = sr;
            CwDecode_Init(0, 0, a);
            capture = true;
        } else if (op == 'W') {
            if (sscanf(line + 1, "%d %d", &a, &b) != 2) return 3;
            CwDecode_wpm(0, a, b);
        } else if (op == 'P') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            CwDecode_pboff(0, (u4_t) a);
        } else if (op == 'C') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            CwDecode_wsc(0, a);
        } else if (op == 'A') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            CwDecode_threshold(0, 0, a);
        } else if (op == 'H') {
            if (sscanf(line + 1, "%d", &a) != 1) return 3;
            CwDecode_threshold(0, 1, a);
        } else if (op == 'T') {
            capture = false;
        } else if (op == 'N') {
            unsigned long n;
            if (sscanf(line + 1, "%lu", &n) != 1) return 3;
            now_sec = (u4_t) n;
        } else if (op == 'B') {
            unsigned long off;
            if (sscanf(line + 1, "%lu", &off) != 1 || off + 512 > npool) return 3;
            sent.clear();
            nev = 0; gblk = 0; in_block = true;
            if (capture) {
                short *p = (short *) pool.data() + off;
                for (int i = 0; i < 512; i++) {
                    const int before = cw->sample_counter;
                    const int long_before = cw->data_len >= CW_DATA_BUFSIZE - 2;
                    const int n0 = nev;
                    branch_seen = 0;
                    CwDecode_RxProcessor(0, 0, 1, p + i);
                    if (cw->process_samples && before + 1 >= cw->blocksize) { gblk++; total_exe++; }
                    if (branch_seen) {
                        bool ok = false;                               // a corrected character: CHARS that is not [err] behind the error
                        for (int e = n0; e < nev; e++) if (sent[6 * e + 2] == EV_CHARS && sent[6 * e + 3] != 0xff) ok = true;
                        stats[2 * (branch_seen - 1)]++;
                        stats[2 * (branch_seen - 1) + 1] += ok;
                    } else if (long_before) {
                        for (int e = n0; e < nev; e++) if (sent[6 * e + 2] == EV_CHARS && sent[6 * e + 3] == 0xff) { stats[4]++; break; }
                    }
                }
            }
            in_block = false;
            fwrite(&nev, 4, 1, of);
            if (!sent.empty()) fwrite(sent.data(), 4, sent.size(), of);
        } else return 3;
    }
    const Goertzel &g = cw->goertzel;
    int32_t w[56];
    int k = 0;
#define I(x) w[k++] = (int32_t) (x)
#define F(x) w[k++] = bits(x)
    I(cw->process_samples); I(cw->wpm_update); I(cw->wsc); I(cw->err_cnt); I(cw->err_timeout); F(cw->sampling_freq); I(cw->speed); I(cw->isAutoThreshold);
    I(cw->weight_linear); I(cw->threshold_linear); I(cw->blocksize);
    I(g.a); F(g.b); F(g.sin); F(g.cos); F(g.r);
    I(cw->sig_lastrx); I(cw->sig_incount); I(cw->sig_outcount); I(cw->sig_timer);
    I(cw->data_len); I(cw->code); I(cw->state); I(cw->b.initialized); I(cw->b.dash); I(cw->b.wspace); I(cw->b.timeout); I(cw->b.track);
    F(cw->times.pulse_avg); F(cw->times.dot_avg); F(cw->times.dash_avg); F(cw->times.symspace_avg); F(cw->times.cwspace_avg); I(cw->times.w_space);
    I(cw->timer_stepsize); I(cw->cur_time); I(cw->cur_outcount); I(cw->last_outcount);
    F(cw->CW_env); F(cw->CW_mag); F(cw->CW_noise); F(cw->old_siglevel); F(cw->speed_wpm_avg);
    I(cw->prevstate); I(cw->noisecancel_change); I(cw->sample_counter); I(cw->startpos); I(cw->progress); I(cw->initializing); I(cw->processed);
    I(cw->training_interval);
    I(snd_rate); I(slowdown_of()); I(capture ? 1 : 0); I(0); I(0);
    if (k != 56 || g.b0 != 0 || g.b1 != 0 || g.b2 != 0) return 6;
    fwrite(w, sizeof w, 1, of);
    for (int i = 0; i < CW_SIG_BUFSIZE; i++) { const uint32_t v = cw->sig[i].state | ((uint32_t) cw->sig[i].time << 1); fwrite(&v, 4, 1, of); }
    for (int i = 0; i < CW_DATA_BUFSIZE; i++) { const uint32_t v = cw->data[i].state | ((uint32_t) cw->data[i].time << 1); fwrite(&v, 4, 1, of); }
    fwrite(cw->raw_signal_buffer, sizeof(float), CW_DECODER_BLOCKSIZE_DEFAULT, of);
    const int32_t tail[8] = {stats[0], stats[1], stats[2], stats[3], stats[4], 0, 0, 0};
    fwrite(tail, sizeof tail, 1, of);
    fclose(of);
    return 0;
}
