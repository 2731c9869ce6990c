// Developer tool (CPU machine only; tools/make_ref_wspr_dec_golden.py builds and runs it): stage 2 of the WSPR extension as the
// reference runs it -- the reference's own statements, cut at build time into a temporary directory:
//   wspr.h:110-332            the defines, wspr_pk_t, wspr_buf_t, wspr_t (WSPR_DEC_CUT_H)
//   wspr.cpp:31-212           pr3, DT, DF, TWOPIDT, sync_and_demodulate (WSPR_DEC_CUT_SYNC)
//   wspr.cpp:437-441          the metric table's loop of wspr_init (WSPR_DEC_CUT_TABLE);  metric_tables.h whole (WSPR_DEC_CUT_METRIC)
//   wspr.cpp:505-513          the tuning constants (WSPR_DEC_CUT_TUNE)
//   wspr.cpp:733-880          the candidate loop from its head to the result classes (WSPR_DEC_CUT_CHAIN)
//   fano.h:15-37, fano.cpp:21-244, tab.cpp:9-42   the decoder, its macro, the parity table (WSPR_DEC_CUT_FANO_H / _FANO / _TAB)
//   wspr_util.cpp:208-230     deinterleave (WSPR_DEC_CUT_DEINT)
// Nothing of the reference's text enters the repository; only the data (tests/golden/wspr_dec_ref.npz) does.
//
// Two builds: A as the reference is (sin / cos of the host's libm); B, -DWSPR_DEC_OURS, with sin and cos INSIDE the cut of
// sync_and_demodulate defined to kg_libm::sin_f2d / cos_f2d (csrc/kg_libm_dtrig.h).  The maker compares the two.
//
// What this harness adds (none of the reference's headers is used):
//   * the integer types, K_PI, the empty printf / yield / send macros, timer_ms, a jelinek that is never called (stack_decoder is 0);
//   * wspr_mode_e (wspr.h:376) and YIELD_EVERY_N_TIMES (:364), restated from the pinned lines;
//   * fano's malloc hands out CLEARED memory (the data bytes of nodes never reached are then zeros, not the heap's);
//   * the loop's frame: the declarations of wspr_decode (:484-496) restated, ipass = 1 so that an ignored candidate is skipped on
//     every call (:740), maxcycles / iifac / quickmode from the scene's pass list; behind the cut, p->ignore = true for a decode
//     (:883, pinned) and the closing brace;
//   * sync_and_demodulate and fano are called THROUGH hooks inside the cut (macros of their names): the hooks keep what each of the six
//     refinement calls returned, every jiggle's symbol bytes, the gates passed and the last fano run's outputs; timer_ms, which the
//     loop calls at a candidate's start (:737), clears them.
// scene file: int32 ncand, npass; float i_data[45000], q_data[45000]; per candidate float freq0, int32 shift0, float drift0, float
// sync0; per pass int32 maxcycles, iifac, quickmode.  Out: [npass][ncand] records of kg_wspr_dec's layout; every jiggle's 162 bytes in
// the order run; the metric table, int32 [2][256].  `-f symbols n maxcycles out`: fano alone (delta 60, :513) on n deinterleaved sets.
#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../flydog_sdr_gps_amd/csrc/kg_libm_dtrig.h"

typedef unsigned char u1_t;
typedef unsigned short u2_t;
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
#define assert_array_dim(d, l) assert((d) >= 0 && (d) < (l))
#define wspr_printf(...)
#define wspr_aprintf(...)
#define wspr_dprintf(...)
#define wspr_d1printf(...)
#define wspr_d2printf(...)
#define lprintf(...) ((void) 0)
#define WSPR_YIELD
#define WSPR_SHMEM_YIELD
#define YIELD_EVERY_N_TIMES 64
#define send_peak_single(w, pki)
#define MORE_EFFORT
typedef enum { FIND_BEST_TIME_LAG, FIND_BEST_FREQ, CALC_SOFT_SYMS } wspr_mode_e;
typedef float fftwf_complex[2];
struct plan_st { fftwf_complex *in, *out; };
typedef plan_st *fftwf_plan;
struct snode { int unused; };

#include "WSPR_DEC_CUT_H.inc"

static wspr_shmem_t shm;
#define WSPR_SHMEM (&shm)

#ifdef WSPR_DEC_OURS
#define sin(x) kg_libm::sin_f2d(x)
#define cos(x) kg_libm::cos_f2d(x)
#endif
#include "WSPR_DEC_CUT_SYNC.inc"
#ifdef WSPR_DEC_OURS
#undef sin
#undef cos
#endif

#include "WSPR_DEC_CUT_FANO_H.inc"
#include "WSPR_DEC_CUT_TAB.inc"
#define LL 1                                // fano.cpp:15, pinned: the Layland-Lushbaugh code
#define malloc(n) calloc(1, (n))
#include "WSPR_DEC_CUT_FANO.inc"
#undef malloc
#include "WSPR_DEC_CUT_DEINT.inc"

#include "WSPR_DEC_CUT_METRIC.inc"
static int mettab[2][256];
static void init_mettab()
{
    float bias = 0.45;                          // wspr.cpp:435, pinned
#include "WSPR_DEC_CUT_TABLE.inc"
}
static int jelinek(unsigned int *, unsigned int *, unsigned char *, unsigned char *, unsigned int, unsigned int, struct snode *, int[2][256], unsigned int)
{
    fprintf(stderr, "jelinek called\n");
    exit(7);
}

struct rec_t {
    int32_t result, ignore;
    float f1; int32_t shift1; float drift1, sync1;
    float tr_f[6]; int32_t tr_shift[6]; float tr_sync[6];
    int32_t idt, ii, jig_shift, gates; float rms;
    uint32_t metric, cycles, maxnp;
    uint8_t decdata[11], symbols[162], pad[3];
};
static_assert(sizeof(rec_t) == 304, "rec_t");

static struct {
    int ncall, gates, jig_shift;
    float tr_f[6], tr_sync[6];
    int tr_shift[6];
    unsigned int metric, cycles, maxnp;
    unsigned char data[11];
} hk;
static FILE *jig_out;

static u4_t timer_ms() { memset(&hk, 0, sizeof hk); return 0; }

static void hooked_sad(wspr_t *w, WSPR_CPX_t *id, WSPR_CPX_t *qd, long np, unsigned char *symbols, float *f1, int ifmin, int ifmax, float fstep, int *shift1, int lagmin,
                       int lagmax, int lagstep, float drift1, int symfac, float *sync, wspr_mode_e mode)
{
    sync_and_demodulate(w, id, qd, np, symbols, f1, ifmin, ifmax, fstep, shift1, lagmin, lagmax, lagstep, drift1, symfac, sync, mode);
    if (mode == CALC_SOFT_SYMS) {
        hk.jig_shift = *shift1;
        fwrite(symbols, 1, NSYM_162, jig_out);
        return;
    }
    if (hk.ncall >= 6) { fprintf(stderr, "a seventh refinement call\n"); exit(7); }
    hk.tr_f[hk.ncall] = *f1; hk.tr_shift[hk.ncall] = *shift1; hk.tr_sync[hk.ncall] = *sync;
    hk.ncall++;
}
static int hooked_fano(unsigned int *metric, unsigned int *cycles, unsigned int *maxnp, unsigned char *data, unsigned char *symbols, unsigned int nbits, int mt[2][256],
                       int delta, unsigned int maxcycles)
{
    memset(data, 0, 11);
    const int r = fano(metric, cycles, maxnp, data, symbols, nbits, mt, delta, maxcycles);
    hk.gates++;
    hk.metric = *metric; hk.cycles = *cycles; hk.maxnp = *maxnp;
    memcpy(hk.data, data, 10);
    return r;
}

static int h_ncand;
static rec_t recs[MAX_NPK];

static void one_pass(unsigned int maxcycles_arg, int iifac_arg, int quick)
{
    wspr_t *w = &WSPR_SHMEM->wspr[0];
    wspr_buf_t *wb = w->buf;
    int i, j, k;
    int ipass = 1;
    int shift1, lagmin, lagmax, lagstep, ifmin, ifmax;
    unsigned int metric, cycles, maxnp;
    int pki, npk = h_ncand;
    float f1, fstep, sync1, drift1, snr;
    int ndecodes_pass;
#include "WSPR_DEC_CUT_TUNE.inc"
    (void) j; (void) k; (void) maxdrift;
    maxcycles = maxcycles_arg;
    iifac = iifac_arg;
    w->quickmode = quick;
    w->stack_decoder = 0;
    w->abort_decode = false;
    WSPR_CPX_t *idat = wb->i_data[0];
    WSPR_CPX_t *qdat = wb->q_data[0];
    int candidates = 0;
    ndecodes_pass = 0;
    memset(recs, 0, sizeof recs);
    for (pki = 0; pki < npk; pki++) recs[pki].ignore = wb->pk_snr[pki].ignore;          // SKIPPED, unless the loop gets there
#define sync_and_demodulate(...) hooked_sad(__VA_ARGS__)
#define fano(...) hooked_fano(__VA_ARGS__)
#include "WSPR_DEC_CUT_CHAIN.inc"
#undef sync_and_demodulate
#undef fano
        if (r_decoded) p->ignore = true;                                                // :883
        (void) r_valid; (void) f_decoded; (void) f_delete; (void) f_image; (void) f_decoding; (void) decode_start; (void) snr;
        rec_t &r = recs[pki];
        r.result = !r_minsync1 ? 1 : r_decoded ? 4 : (r_timeUp && r_tooWeak) ? 2 : r_timeUp ? 3 : 5;
        r.ignore = p->ignore;
        r.f1 = f1; r.shift1 = shift1; r.drift1 = drift1; r.sync1 = sync1;
        for (int c = 0; c < hk.ncall; c++) { r.tr_f[c] = hk.tr_f[c]; r.tr_shift[c] = hk.tr_shift[c]; r.tr_sync[c] = hk.tr_sync[c]; }
        r.idt = idt;
        r.gates = hk.gates;
        if (idt > 0) { r.ii = ii; r.jig_shift = hk.jig_shift; r.rms = rms; memcpy(r.symbols, w->symbols, NSYM_162); }
        r.metric = hk.metric; r.cycles = hk.cycles; r.maxnp = hk.maxnp;
        memcpy(r.decdata, hk.data, 10);
    }
    (void) candidates; (void) ndecodes_pass;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "-f")) {                                      // fano alone: symbols n maxcycles out
        const int n = atoi(argv[3]);
        FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[5], "wb");
        if (!in || !out) return 3;
        init_mettab();
        for (int s = 0; s < n; s++) {
            unsigned char sy[NSYM_162];
            struct { int32_t ok; uint32_t metric, cycles, maxnp; uint8_t data[12]; } o;
            memset(&o, 0, sizeof o);
            if (fread(sy, 1, NSYM_162, in) != NSYM_162) return 4;
            o.ok = fano(&o.metric, &o.cycles, &o.maxnp, o.data, sy, NBITS, mettab, 60, (unsigned int) atol(argv[4]));
            fwrite(&o, sizeof o, 1, out);
        }
        fclose(out);
        return 0;
    }
    if (argc != 5) { fprintf(stderr, "usage: %s scene out jig mettab | -f symbols n maxcycles out\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb"), *mt = fopen(argv[4], "wb");
    jig_out = fopen(argv[3], "wb");
    if (!in || !out || !jig_out || !mt) return 3;
    wspr_t *w = &WSPR_SHMEM->wspr[0];
    memset(&shm, 0, sizeof shm);
    w->buf = &WSPR_SHMEM->wspr_buf[0];
    init_mettab();
    fwrite(mettab, sizeof mettab, 1, mt);
    fclose(mt);
    int32_t head[2];
    if (fread(head, 4, 2, in) != 2 || head[0] < 0 || head[0] > MAX_NPK) return 4;
    h_ncand = head[0];
    if (fread(w->buf->i_data[0], sizeof(float), TPOINTS, in) != TPOINTS || fread(w->buf->q_data[0], sizeof(float), TPOINTS, in) != TPOINTS) return 4;
    for (int c = 0; c < h_ncand; c++) {
        struct { float freq0; int32_t shift0; float drift0, sync0; } cd;
        if (fread(&cd, sizeof cd, 1, in) != 1) return 4;
        wspr_pk_t *p = &w->buf->pk_snr[c];
        p->freq0 = cd.freq0; p->shift0 = cd.shift0; p->drift0 = cd.drift0; p->sync0 = cd.sync0; p->freq_idx = c; p->ignore = false;
    }
    for (int ps = 0; ps < head[1]; ps++) {
        int32_t a[3];
        if (fread(a, 4, 3, in) != 3) return 4;
        one_pass((unsigned int) a[0], a[1], a[2]);
        fwrite(recs, sizeof(rec_t), h_ncand, out);
    }
    fclose(out);
    fclose(jig_out);
    return 0;
}
