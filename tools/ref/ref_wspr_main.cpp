// Developer tool (CPU machine only; tools/make_ref_wspr_golden.py builds and runs it): stage 1 of the WSPR extension as the reference
// runs it -- the reference's own statements, cut at build time into a temporary directory:
//   wspr.h:110-332            the defines, wspr_pk_t, wspr_buf_t, wspr_t (WSPR_CUT_H)
//   wspr_main.cpp:94-114      status_str, wspr_status (WSPR_CUT_STATUS)
//   wspr_main.cpp:140-240     the body of WSPR_FFT's loop: the transforms of a group and its row (WSPR_CUT_FFT)
//   wspr_main.cpp:592-788     int_decimate, wspr_data (WSPR_CUT_DATA);  :790-800 wspr_reset (WSPR_CUT_RESET)
//   wspr_main.cpp:1154-1156   nffts, nbins_411, hbins_205 (WSPR_CUT_CONST);  :1186-1188 the window (WSPR_CUT_WINDOW)
//   wspr.cpp:31-40 pr3 (WSPR_CUT_PR3);  :214-253 renormalize (WSPR_CUT_RENORM);  :555-714 pass 0: peak list and coarse search (WSPR_CUT_PASS0)
//   wspr_util.cpp:394-406     snr_comp, freq_comp (WSPR_CUT_COMP)
// Nothing of the reference's text enters the repository; only the data (tests/golden/wspr_ref.npz) does.
//
// What this harness adds (none of the reference's headers is used):
//   * the integer types, TYPECPX, K_PI, TRUE / FALSE, the status numbers of wspr_main.cpp:49-53 and the empty printf macros;
//   * fftwf_complex, a plan that holds its two arrays, and fftwf_execute as wspr_dft512 of wspr_harness.h (FFTW is not here);
//   * the two tasks run where they are woken (TaskWakeupFP): WSPR_FFT's loop body, then `if (last < nffts) continue;` (:275) and the
//     wake-up of WSPR_Deco (:277-281), restated; WSPR_Deco as abort_decode = false, status DECODING, pass 0, status_resume (:468-472, :568);
//   * utc_hour_min_sec from the script's B lines; ext_send_msg / ext_send_msg_data recording the status changes and the rows;
//   * the commands of wspr_msgs (:834-838, :880-900) and wspr_close (:802-824) restated from the pinned lines; what wspr_main does to a
//     wspr_t (:1163-1176) restated too;
//   * at a cycle end, two conditions of the golden: no two kept peaks tie in snr0 (nor the last kept with the first dropped), and every
//     10*log10 of a kept peak is at least 4 double ulps from a float rounding tie (log10l as the judge).
#include <assert.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef unsigned char u1_t;
typedef unsigned int u4_t;
typedef short s2_t;
typedef int s4_t;
typedef struct { double lat, lon; } latLon_t;
typedef struct conn_st conn_t;
typedef struct { float re, im; } TYPECPX;
#define SPACE_FOR_NULL 1
#define MAX_RX_CHANS 1
#define TRUE 1
#define FALSE 0
#define K_PI (3.14159265358979323846)
#define NONE 0
#define IDLE 1
#define SYNC 2
#define RUNNING 3
#define DECODING 4
#define WSPR_DATA 0
#define WSPR_DEBUG_MSG false
#define assert_array_dim(d, l) assert((d) >= 0 && (d) < (l))
#define wspr_printf(...)
#define wspr_aprintf(...)
#define wspr_dprintf(...)
#define wspr_d1printf(...)
#define lprintf(...) ((void) 0)
#define WSPR_YIELD
#define WSPR_SHMEM_YIELD
#define TWF_CHECK_WAKING 0
#define TO_VOID_PARAM(x) ((void *) (intptr_t) (x))
#define FLIP16(x) (x)
#define kiwi_snprintf_buf(buf, ...) snprintf(buf, sizeof(buf), __VA_ARGS__)
#define send_peaks_all(w, n) (w)->npk = (n)
#define MORE_EFFORT

typedef float fftwf_complex[2];
struct plan_st { fftwf_complex *in, *out; };
typedef plan_st *fftwf_plan;

static int h_cycles;
#include "wspr_harness.h"
static void fftwf_execute(fftwf_plan p) { wspr_dft512(p->in, p->out); }

#include "WSPR_CUT_H.inc"

static wspr_shmem_t shm;
#define WSPR_SHMEM (&shm)
wspr_conf_t wspr_c;
int nffts, nbins_411, hbins_205;
static float window[NFFT];
static int cur_min, cur_sec, was_inited;
enum { FFT_TASK = 1, DECO_TASK = 2 };

static void utc_hour_min_sec(int *, int *min, int *sec) { *min = cur_min; *sec = cur_sec; }
static time_t utc_time() { return 0; }
static void ext_unregister_receive_iq_samps(int) {}
static int qsort_floatcomp(const void *a, const void *b)
{
    const float x = *(const float *) a, y = *(const float *) b;
    return x < y ? -1 : x > y ? 1 : 0;
}
static int ext_send_msg(int, bool, const char *fmt, ...)
{
    if (!strncmp(fmt, "EXT WSPR_STATUS=", 16)) {
        va_list ap;
        va_start(ap, fmt);
        rec_status(va_arg(ap, int));
        va_end(ap);
    }
    return 0;
}
static int ext_send_msg_data(int, bool, u1_t cmd, u1_t *bytes, int n)
{
    wspr_t *w = &WSPR_SHMEM->wspr[0];
    if (cmd != WSPR_DATA || n != 412) { fprintf(stderr, "unexpected ext_send_msg_data %d %d\n", cmd, n); exit(7); }
    rec_row(w->FFTtask_group, w->fft_ping_pong, w->buf->savg, bytes);
    return 0;
}
static void TaskWakeupFP(int id, int, void *);

#include "WSPR_CUT_STATUS.inc"
#include "WSPR_CUT_PR3.inc"
#include "WSPR_CUT_COMP.inc"
#include "WSPR_CUT_RENORM.inc"
#include "WSPR_CUT_DATA.inc"
#include "WSPR_CUT_RESET.inc"

static void pass0(int rx_chan)
{
    wspr_t *w = &WSPR_SHMEM->wspr[rx_chan];
    wspr_buf_t *wb = w->buf;
    int i, j, k;
    int ipass = 0;
    float DF2 = FSRATE / FSPS / 2;
    int pki, npk = 0;
    int maxdrift = 4;
    float sync1;
#include "WSPR_CUT_PASS0.inc"
    (void) i;
    rec_pk pk[MAX_NPK];
    rec_cand cand[MAX_NPK];
    int32_t cond[4] = {1, 1, 0, 0};
    for (pki = 0; pki < npk; pki++) {
        const wspr_pk_t &f = w->pk_freq[pki], &s = wb->pk_snr[pki];
        pk[pki] = rec_pk{f.bin0, f.freq0, f.snr0};
        cand[pki] = rec_cand{s.freq0, s.shift0, s.drift0, s.sync0, s.freq_idx, s.bin0};
        if (pki + 1 < npk && wb->pk_snr[pki + 1].snr0 == s.snr0) cond[0] = 0;
        const long double v = 10 * log10l((long double) wb->smspec[WSPR_RENORM_DECODE][s.bin0]) - (long double) w->snr_scaling_factor;
        const float fl = (float) v;
        const long double up = ((long double) fl + (long double) nextafterf(fl, INFINITY)) / 2, dn = ((long double) fl + (long double) nextafterf(fl, -INFINITY)) / 2;
        const long double dist = fminl(fabsl(v - up), fabsl(v - dn));
        const double vd = (double) v, ulp = nextafter(fabs(vd), INFINITY) - fabs(vd);
        if (dist < 4 * (long double) ulp) cond[1] = 0;
    }
    // the strongest dropped peak still stands behind the kept ones (the first qsort left it there; the memset of :560 left zeros behind the list)
    if (npk == MAX_NPK && wb->pk_snr[MAX_NPK].bin0 != 0 && wb->pk_snr[MAX_NPK].snr0 == wb->pk_snr[MAX_NPK - 1].snr0) cond[0] = 0;
    rec_cycle(w->decode_ping_pong, npk, pk, cand, cond);
}

static void deco(int rx_chan)                  // WSPR_Deco, :468-472 and :568
{
    wspr_t *w = &WSPR_SHMEM->wspr[rx_chan];
    w->abort_decode = false;
    wspr_status(w, DECODING, NONE);
    pass0(rx_chan);
    h_cycles++;
    wspr_status(w, w->status_resume, NONE);
}

static void fft_task(int rx_chan)              // one turn of WSPR_FFT's loop (:126-282)
{
    wspr_t *w = &WSPR_SHMEM->wspr[rx_chan];
    wspr_buf_t *wb = w->buf;
    int i, j, k;
    int pgrp = 0, plast = 0;
#include "WSPR_CUT_FFT.inc"
    (void) pgrp; (void) plast; (void) max_dB;
    if (last < nffts) return;                  // :275
    w->decode_ping_pong = w->fft_ping_pong;    // :277-281
    w->not_launched = 0;
    TaskWakeupFP(w->WSPR_DecodeTask_id, TWF_CHECK_WAKING, TO_VOID_PARAM(w->rx_chan));
}

static void TaskWakeupFP(int id, int, void *)
{
    if (id == FFT_TASK) fft_task(0);
    else if (id == DECO_TASK) deco(0);
    else { fprintf(stderr, "unexpected task %d\n", id); exit(7); }
}

static void main_init()                        // wspr_main, :1154-1156, :1163-1176, :1186-1188, restated around the cuts
{
    int i;
#include "WSPR_CUT_CONST.inc"
    wspr_t *w = &WSPR_SHMEM->wspr[0];
    memset(w, 0, sizeof(wspr_t));
    w->magic1 = 0xcafe; w->magic2 = 0xbabe;
    w->rx_chan = 0;
    w->buf = &WSPR_SHMEM->wspr_buf[0];
    w->medium_effort = 1;
    w->wspr_type = WSPR_TYPE_2MIN;
    w->fftin = (fftwf_complex *) calloc(NFFT, sizeof(fftwf_complex));
    w->fftout = (fftwf_complex *) calloc(NFFT, sizeof(fftwf_complex));
    w->fftplan = new plan_st{w->fftin, w->fftout};
    w->WSPR_FFTtask_id = FFT_TASK; w->WSPR_DecodeTask_id = DECO_TASK;
    w->create_tasks = true;
    wspr_reset(w);
#include "WSPR_CUT_WINDOW.inc"
    if (nffts != 343 || nbins_411 != 411 || hbins_205 != 205) { fprintf(stderr, "constants %d %d %d\n", nffts, nbins_411, hbins_205); exit(7); }
}

static int h_init(double snd_rate)             // `SET ext_server_init`, :834-838; int_decimate of :1193
{
    if (!(snd_rate >= 375.0 && snd_rate <= 1e9)) return 11;
    if (!was_inited) main_init();
    was_inited = 1;
    int_decimate = (int) (snd_rate / FSRATE);
    wspr_status(&WSPR_SHMEM->wspr[0], IDLE, IDLE);
    return 0;
}
static int h_capture(int on)                   // `SET capture=%d`, :880-900
{
    if (!was_inited) return 14;
    wspr_t *w = &WSPR_SHMEM->wspr[0];
    w->capture = on;
    if (w->capture) {
        w->send_error = false;
        w->reset = TRUE;
        wspr_status(w, SYNC, RUNNING);
    } else {
        w->abort_decode = true;
        wspr_reset(w);                         // wspr_close, :802-824
    }
    return 0;
}
static int h_type(int type)
{
    if (!was_inited) return 14;
    if (type != WSPR_TYPE_2MIN && type != WSPR_TYPE_15MIN) return 12;
    WSPR_SHMEM->wspr[0].wspr_type = type;
    return 0;
}
static int h_more(int on)
{
    if (!was_inited) return 14;
    WSPR_SHMEM->wspr[0].more_candidates = on != 0;
    return 0;
}
static int h_block(const float *iq, int n, int min, int sec)
{
    if (!was_inited) return 14;
    if (min < 0 || min > 59 || sec < 0 || sec > 59) return 13;
    cur_min = min; cur_sec = sec;
    wspr_data(0, 0, n, (TYPECPX *) iq);
    return 0;
}
static int h_load(const float *pwr_samp, const float *pwr_sampavg)
{
    if (!was_inited) return 14;
    wspr_t *w = &WSPR_SHMEM->wspr[0];
    memcpy(w->buf->pwr_samp[0], pwr_samp, sizeof w->buf->pwr_samp[0]);
    memcpy(w->buf->pwr_sampavg[0], pwr_sampavg, sizeof w->buf->pwr_sampavg[0]);
    w->decode_ping_pong = 0;
    pass0(0);
    return 0;
}
static void h_dump(int32_t *o, FILE *planes)
{
    if (!was_inited) main_init();
    wspr_t *w = &WSPR_SHMEM->wspr[0];
    const int32_t v[18] = {was_inited, w->capture, w->reset, w->tsync, w->ping_pong, w->fft_ping_pong, w->decode_ping_pong, w->decim, w->didx, w->group,
                           w->status, w->status_resume, w->last_sec, w->abort_decode, w->wspr_type, w->more_candidates, was_inited ? int_decimate : 0, h_cycles};
    memcpy(o, v, sizeof v);
    fwrite(w->buf->pwr_sampavg, sizeof w->buf->pwr_sampavg, 1, planes);
    fwrite(w->buf->pwr_samp, sizeof w->buf->pwr_samp, 1, planes);
    fwrite(w->buf->i_data, sizeof w->buf->i_data, 1, planes);
    fwrite(w->buf->q_data, sizeof w->buf->q_data, 1, planes);
}
