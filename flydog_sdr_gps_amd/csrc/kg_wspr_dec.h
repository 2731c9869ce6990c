// kg_wspr_dec.h -- the WSPR extension (extensions/wspr/), stage 2: from a candidate of stage 1 (kg_wspr.h) to the 50 message bits.  On
// the device AND the host, in the reference's own operand types; library, host driver and golden are built with -ffp-contract=off.
// What lives here:
//   * sync_and_demodulate (wspr.cpp:45-212) in its three modes, as the pieces a kernel can share out: the frequency of a symbol (:93),
//     the phase step of a tone (:96-108), a step of the double recurrence (:117-125), a step of the float accumulators (:143-150), the
//     power of a tone (:155-163), a symbol's part of totp and ss (:165-167), the soft symbol (:168-174), the normalisation and the byte
//     (:194-206) -- and the whole function from those pieces, for the host;
//   * the body of wspr_decode's candidate loop (:745-880): the six refinement calls, the three-way choice of the drift (:781-789), the
//     minsync1 gate (:795), the jiggle loop (:819-867) with the rms / sync gate (:830-838), deinterleave (wspr_util.cpp:208-230) and
//     the Fano decoder (fano.cpp:91-244), the result classes (:869-883);
//   * the tuning constants of :505-513; the convolutional polynomials (fano.cpp:52-53), byte parity (tab.cpp: the parity of a byte, here
//     by counting bits) and the interleaver are the published protocol.
// Kept to the letter: f0 = *f1 + ifreq*fstep in float; fp in double rounded to float; dphi a float product; c[0] = 1, s[0] = 0; each
// accumulator step widens to double, adds its two products left to right and rounds to float; k > 0 && k < np (sample 0 is never
// used); p = sqrt in double of a double that holds a FLOAT sum of float squares; totp double, ss float; ss > syncmax with ifreq the
// outer loop and lag the inner one from -1e30; fsum / f2sum float with the divisions in double; the clamps, + 128, the byte.
// fano: maxcycles *= nbits, the tail from nbits - 31, *cycles = i + 1, i >= maxcycles returns 0 even if the last cycle finished, the
// 10 data bytes from nodes[7 + 8 n].
// The seeds of the recurrences, cos(dphi) and sin(dphi) in double of a float-valued dphi, are kg_libm::cos_f2d / sin_f2d
// (kg_libm_dtrig.h: correctly rounded), NOT the host's libm: DESIGN 6.20, stage 2, decision 1.
// Defined here where the reference leaves it open:
//   * silence: totp == 0 makes ss / totp NaN, which never beats syncmax: the call returns shift 0, frequency 0.0 and sync -1e30, to the
//     letter;
//   * a NaN soft symbol gives byte 0 ((u1_t) NaN is undefined; stage 1 pinned the same); such a set never reaches fano: rms or sync
//     fails the gate;
//   * fano's nodes are malloc'ed and never cleared: after a timeout the data bytes of nodes never reached are whatever the heap held.
//     Here the nodes start as zeros (the golden's build of the reference hands fano cleared memory);
//   * metric, cycles, maxnp are those of the candidate's last fano run, 0 if none ran (the reference leaves them uninitialised and only
//     prints them); decdata[10] is 0 (fano writes 10 of w->decdata's 11 bytes);
//   * quickmode leaves the jiggle loop after idt 0: not decoded and no time-up.  That is R_QUICK_MISS; ignore stays clear;
//   * the metric table is the caller's: entries beyond +-2^20 are refused (81 sums of two stay far inside an int).
// REFUSED by the callers of this header, nothing changed: a decode before the table is set; iifac outside 1 .. 128; maxcycles outside
// 1 .. 2^20; a candidate with |freq0| > 113, |shift0| > TPOINTS or |drift0| > 4 (every dphi stays below 2.5).
#ifndef KG_WSPR_DEC_H
#define KG_WSPR_DEC_H
#include "kg_libm_dtrig.h"
#include "kg_wspr.h"

namespace kg_wspr_df {
using kg_wspr_cf::NSYM;
using kg_wspr_cf::SPS;
using kg_wspr_cf::TPOINTS;

enum { NBITS = 81, NNODES = NBITS + 1, TAIL = NBITS - 31, NDATA = 10, LEN_DECODE = 11 };                     // wspr.h:172-174, fano.cpp:116-117, :233
enum { JIG_RANGE = 128, SYMFAC = 50, DELTA = 60, MAX_IDT = JIG_RANGE + 1, NCALLS = 6 };                       // wspr.cpp:509-513
enum { R_SKIPPED = 0, R_MINSYNC1 = 1, R_NO_CHANGE = 2, R_TIME_UP = 3, R_DECODED = 4, R_QUICK_MISS = 5 };
enum { MAX_MAXCYCLES = 1 << 20, MAX_METRIC = 1 << 20 };
#define KG_WSPR_DEC_MINSYNC1 0.10f                             /* wspr.cpp:506 */
#define KG_WSPR_DEC_MINSYNC2 0.12f                             /* :507 */
#define KG_WSPR_DEC_MINRMS 40.625f                             /* :512: 52.0 * (50 / 64.0), exact */
#define KG_WSPR_POLY1 0xf2d05351u                          /* fano.cpp:52-53: the Layland-Lushbaugh code */
#define KG_WSPR_POLY2 0xe4613c47u
#define KG_WSPR_DF 1.46484375f                             /* FSRATE / FSPS (wspr.cpp:42): exact */

// one candidate of one pass (kg_wspr_dec of include/kiwigpu_wspr_dec.h)
struct rec_t {
    int32_t result, ignore;
    float f1; int32_t shift1; float drift1, sync1;
    float tr_f[NCALLS]; int32_t tr_shift[NCALLS]; float tr_sync[NCALLS];
    int32_t idt, ii, jig_shift, gates; float rms;
    uint32_t metric, cycles, maxnp;
    uint8_t decdata[LEN_DECODE], symbols[NSYM], pad[3];
};
static_assert(sizeof(rec_t) == 304, "rec_t");

// ---- sync_and_demodulate, piece by piece
KG_NR_HD float twopidt() { const float DT = 1.0 / 375.0; return 2 * KG_WSPR_K_PI * DT; }                   // wspr.cpp:42-43
KG_NR_HD float f0_of(float f1, int ifreq, float fstep) { return f1 + ifreq * fstep; }                       // :88
KG_NR_HD float fp_of(float f0, float drift1, int i) { return f0 + (drift1 / 2.0) * ((float) i - (162.0 / 2)) / (162.0 / 2); }       // :93
KG_NR_HD float dphi_of(float fp, int tone)                                                                  // :96, :100, :104, :108 (DF15, DF05 of :59)
{
    const float DF15 = KG_WSPR_DF * 1.5, DF05 = KG_WSPR_DF * 0.5;
    const float TWOPIDT = twopidt();
    return tone == 0 ? TWOPIDT * (fp - DF15) : tone == 1 ? TWOPIDT * (fp - DF05) : tone == 2 ? TWOPIDT * (fp + DF05) : TWOPIDT * (fp + DF15);
}
KG_NR_HD void seed_of(float dphi, double *cd, double *sd) { *cd = kg_libm::cos_f2d((double) dphi); *sd = kg_libm::sin_f2d((double) dphi); }
KG_NR_HD void rot_step(double &c, double &s, double cd, double sd)                                          // :118-119
{
    const double c1 = c * cd - s * sd, s1 = c * sd + s * cd;
    c = c1; s = s1;
}
#ifndef KG_WSPR_DEC_ACC_T
#define KG_WSPR_DEC_ACC_T float                            /* a test builds the twin with double here: the golden must notice */
#endif
typedef KG_WSPR_DEC_ACC_T acc_t;
KG_NR_HD void acc_step(acc_t &ii, acc_t &qq, float idk, float qdk, double c, double s)                      // :143-144
{
    ii = ii + idk * c + qdk * s;
    qq = qq - idk * s + qdk * c;
}
KG_NR_HD bool k_used(int k, int np)                                                                         // :141
{
#ifdef KG_WSPR_DEC_MUT_K0
    return (k >= 0) && (k < np);
#else
    return (k > 0) && (k < np);
#endif
}
KG_NR_HD double p_of(acc_t ii, acc_t qq) { double p = ii * ii + qq * qq; return sqrt(p); }                 // :155, :160
KG_NR_HD void sym_step(double &totp, float &ss, double p0, double p1, double p2, double p3, int pr3)        // :165-167
{
    totp = totp + p0 + p1 + p2 + p3;
    const double cmet = (p1 + p3) - (p0 + p2);
    ss = (pr3 == 1) ? ss + cmet : ss - cmet;
}
KG_NR_HD float fsymb_of(double p0, double p1, double p2, double p3, int pr3) { return pr3 == 1 ? p3 - p1 : p2 - p0; }     // :169-173
KG_NR_HD float ss_of(float ss, double totp) { return ss / totp; }                                           // :176
KG_NR_HD bool ss_wins(float ss, double syncmax)                                                             // :177
{
#ifdef KG_WSPR_DEC_MUT_GE
    return ss >= syncmax;
#else
    return ss > syncmax;
#endif
}
KG_NR_HD void norm_step(float &fsum, float &f2sum, float fs)                                                // :195-196
{
    fsum = fsum + fs / 162.0;
    f2sum = f2sum + fs * fs / 162.0;
}
KG_NR_HD double fac_of(float fsum, float f2sum) { return KG_WSPR_SQRT(f2sum - fsum * fsum); }               // :198: sqrt of a float argument
KG_NR_HD float soft_value(float fs, double fac, int symfac)                                                 // :202-204, before the byte
{
    fs = symfac * fs / fac;
    if (fs > 127) fs = 127.0;
    if (fs < -128) fs = -128.0;
    return fs;
}
KG_NR_HD uint8_t soft_byte(float fs) { const float v = fs + 128; return v == v ? (uint8_t) v : (uint8_t) 0; }            // :205; NaN: 0
KG_NR_HD void rms_step(float &sq, uint8_t sym) { const float y = (float) sym - 128.0; sq += y * y; }       // :832-833
KG_NR_HD float rms_of(float sq) { return sqrt(sq / 162.0); }                                                // :835
KG_NR_HD bool gate_of(float sync1, float rms) { return (sync1 > KG_WSPR_DEC_MINSYNC2) && (rms > KG_WSPR_DEC_MINRMS); }           // :838
// the jiggle of step idt (:820-822): 0, -1, +1, -2, +2 ... times iifac
KG_NR_HD int ii_of(int idt, int iifac)
{
    int ii = (idt + 1) / 2;
#ifdef KG_WSPR_DEC_MUT_JIG
    if ((idt & 1) == 0) ii = -ii;
#else
    if ((idt & 1) == 1) ii = -ii;
#endif
    return iifac * ii;
}
KG_NR_HD int nidt_of(int iifac, int quickmode) { return quickmode ? 1 : JIG_RANGE / iifac + 1; }            // :819, :866

// deinterleave (wspr_util.cpp:208-230): place p of the result holds symbol perm(p), the p-th of the bit-reversed bytes below 162
KG_NR_HD int bitrev8(int i) { return (int) ((((i * 0x80200802ULL) & 0x0884422110ULL) * 0x0101010101ULL >> 32) & 0xff); }
template <typename P> KG_NR_HD void deint_table(P *perm)
{
    int p = 0;
    for (int i = 0; i < 256 && p < NSYM; i++) {
        const int j = bitrev8(i);
        if (j < NSYM) perm[p++] = (P) j;
    }
}

// ---- fano (fano.cpp:91-244)
KG_NR_HD int parity32(uint32_t v) { return __builtin_popcount(v) & 1; }
KG_NR_HD int enc_sym(uint32_t encstate) { return (parity32(encstate & KG_WSPR_POLY1) << 1) | parity32(encstate & KG_WSPR_POLY2); }   // ENCODE, fano.h:28-37
// NS: the node store: enc(n), gamma(n), tm0(n), tm1(n), br(n) as references, n = 0 .. NBITS, all zeros at entry;
// sym(k): deinterleaved symbol k; met(a, v): mettab[a][v].  data: NDATA bytes.  Returns 1 on success, 0 on timeout.
template <typename NS, typename SYM, typename MET>
KG_NR_HD int fano(NS &ns, SYM sym, MET met, int delta, uint32_t maxcycles, uint32_t *metric, uint32_t *cycles, uint32_t *maxnp, uint8_t *data)
{
    auto metrics = [&](int n, int k) { return met(k >> 1, sym(2 * n)) + met(k & 1, sym(2 * n + 1)); };     // :124-127
    auto sort_branches = [&](int n) {                                                                       // :134-152, :187-203
        const int lsym = enc_sym(ns.enc(n));
        const int m0 = metrics(n, lsym), m1 = metrics(n, 3 ^ lsym);
        if (m0 > m1) { ns.tm0(n) = m0; ns.tm1(n) = m1; }
        else { ns.tm0(n) = m1; ns.tm1(n) = m0; ns.enc(n)++; }
    };
    const int lastnode = NBITS - 1;
    int n = 0, t = 0;
    uint32_t mnp = 0, i;
    ns.enc(0) = 0;
    sort_branches(0);
    ns.br(0) = 0;
    maxcycles *= NBITS;                                                                                     // :154
    ns.gamma(0) = 0;
    for (i = 1; i <= maxcycles; i++) {
        if (n > (int) mnp) mnp = (uint32_t) n;
        const int ngamma = ns.gamma(n) + (ns.br(n) ? ns.tm1(n) : ns.tm0(n));
        if (ngamma >= t) {
            if (ns.gamma(n) < t + delta)
                while (ngamma >= t + delta) t += delta;
            ns.gamma(n + 1) = ngamma;
            ns.enc(n + 1) = ns.enc(n) << 1;
            if (++n == lastnode + 1) break;
#ifdef KG_WSPR_DEC_MUT_TAIL
            if (n > TAIL) ns.tm0(n) = metrics(n, enc_sym(ns.enc(n)));
#else
            if (n >= TAIL) ns.tm0(n) = metrics(n, enc_sym(ns.enc(n)));                                      // :188-192: the tail is zeros
#endif
            else sort_branches(n);
            ns.br(n) = 0;
            continue;
        }
        for (;;) {                                                                                          // :209-228
            if (n == 0 || ns.gamma(n - 1) < t) {
                t -= delta;
                if (ns.br(n) != 0) { ns.br(n) = 0; ns.enc(n) ^= 1; }
                break;
            }
            if (--n < TAIL && ns.br(n) != 1) { ns.br(n)++; ns.enc(n) ^= 1; break; }
        }
    }
    *metric = (uint32_t) ns.gamma(n);
    for (int k = 0; k < NDATA; k++) data[k] = (uint8_t) ns.enc(7 + 8 * k);
    *cycles = i + 1;
    *maxnp = mnp;
#ifdef KG_WSPR_DEC_MUT_CYC
    return i > maxcycles ? 0 : 1;
#else
    return i >= maxcycles ? 0 : 1;                                                                          // :242
#endif
}

// ---- the host twin
#if !defined(__HIP_DEVICE_COMPILE__)
enum { MODE_LAG = 0, MODE_FREQ = 1, MODE_SOFT = 2 };
struct margin_t { float least; int32_t strict; };                                                            // over the search calls: (winner - runner-up) / |winner|

// sync_and_demodulate (wspr.cpp:45-212).  fsymb_pre: the soft values before the byte (null: not wanted)
inline void sync_and_demodulate(const float *id, const float *qd, long np, uint8_t *symbols, float *f1, int ifmin, int ifmax, float fstep, int *shift1, int lagmin,
                                int lagmax, int lagstep, float drift1, int symfac, float *sync, int mode, margin_t *mg = nullptr, float *fsymb_pre = nullptr)
{
    static const unsigned char pr3[NSYM] = KG_WSPR_PR3;
    float fsymb[NSYM], f0 = 0.0, ss, fbest = 0.0, fsum = 0.0, f2sum = 0.0;
    double syncmax = -1e30, second = -1e30, totp;
    int best_shift = 0;
    if (mode == MODE_LAG) { ifmin = 0; ifmax = 0; fstep = 0.0; }
    if (mode == MODE_FREQ) { lagmin = *shift1; lagmax = *shift1; }
    if (mode == MODE_SOFT) { lagmin = *shift1; lagmax = *shift1; ifmin = 0; ifmax = 0; }
    for (int ifreq = ifmin; ifreq <= ifmax; ifreq++) {
        f0 = f0_of(*f1, ifreq, fstep);
        for (int lag = lagmin; lag <= lagmax; lag = lag + lagstep) {
            ss = 0.0;
            totp = 0.0;
            for (int i = 0; i < NSYM; i++) {
                const float fp = fp_of(f0, drift1, i);
                double p[4];
                for (int tone = 0; tone < 4; tone++) {
                    double cd, sd, c = 1, s = 0;
                    seed_of(dphi_of(fp, tone), &cd, &sd);
                    acc_t ii = 0.0, qq = 0.0;
                    for (int j = 0; j < SPS; j++) {
                        if (j) rot_step(c, s, cd, sd);
                        const int k = lag + i * SPS + j;
                        if (k_used(k, (int) np)) acc_step(ii, qq, id[k], qd[k], c, s);
                    }
                    p[tone] = p_of(ii, qq);
                }
                sym_step(totp, ss, p[0], p[1], p[2], p[3], pr3[i]);
                if (mode == MODE_SOFT) fsymb[i] = fsymb_of(p[0], p[1], p[2], p[3], pr3[i]);
            }
            ss = ss_of(ss, totp);
            if (ss_wins(ss, syncmax)) { second = syncmax; syncmax = ss; best_shift = lag; fbest = f0; }
            else if (ss > second) second = ss;
        }
    }
    if (mg && mode != MODE_SOFT && second > -1e30) {
        if (!(syncmax > second)) mg->strict = 0;
        const float rel = (float) ((syncmax - second) / fabs(syncmax));
        if (rel < mg->least) mg->least = rel;
    }
    *sync = syncmax;
    if (mode != MODE_SOFT) { *shift1 = best_shift; *f1 = fbest; return; }
    for (int i = 0; i < NSYM; i++) norm_step(fsum, f2sum, fsymb[i]);
    const double fac = fac_of(fsum, f2sum);
    for (int i = 0; i < NSYM; i++) {
        const float v = soft_value(fsymb[i], fac, symfac);
        if (fsymb_pre) fsymb_pre[i] = v;
        symbols[i] = soft_byte(v);
    }
}

inline void deinterleave(uint8_t *sym)
{
    uint8_t perm[NSYM], tmp[NSYM];
    deint_table(perm);
    for (int p = 0; p < NSYM; p++) tmp[p] = sym[perm[p]];
    memcpy(sym, tmp, NSYM);
}

struct host_nodes {
    uint32_t e[NNODES]; int32_t g[NNODES], a[NNODES], b[NNODES], r[NNODES];
    host_nodes() { memset(this, 0, sizeof *this); }
    uint32_t &enc(int n) { return e[n]; }
    int32_t &gamma(int n) { return g[n]; }
    int32_t &tm0(int n) { return a[n]; }
    int32_t &tm1(int n) { return b[n]; }
    int32_t &br(int n) { return r[n]; }
};
inline int fano_host(const uint8_t *symbols, const int32_t *mettab, uint32_t maxcycles, uint32_t *metric, uint32_t *cycles, uint32_t *maxnp, uint8_t *data)
{
    host_nodes ns;
    return fano(ns, [&](int k) { return symbols[k]; }, [&](int a, int v) { return mettab[a * 256 + v]; }, DELTA, maxcycles, metric, cycles, maxnp, data);
}

// what the maker wants to know beside the record
struct watch_t {
    margin_t mg;
    float int_dist;                             // the least distance of a pre-clamp soft value from an integer, over the jiggles run
    int32_t njig;
    uint8_t jig_syms[MAX_IDT][NSYM];            // the bytes of every jiggle run, before deinterleave
};

// one candidate of one pass (wspr.cpp:745-883).  ignore: the flag, in and out.  w_symbols: w->symbols, which outlives the candidate.
inline void decode_candidate(const float *idat, const float *qdat, const int32_t *mettab, float freq0, int shift0, float drift0, float sync0, int32_t *ignore,
                             uint32_t maxcycles, int iifac, int quickmode, uint8_t *w_symbols, rec_t &r, watch_t *watch = nullptr)
{
    memset(&r, 0, sizeof r);
    if (*ignore) { r.result = R_SKIPPED; r.ignore = 1; return; }
    margin_t *mg = watch ? &watch->mg : nullptr;
    float f1 = freq0, drift1 = drift0, sync1 = sync0;
    int shift1 = shift0;
    const int symfac = SYMFAC;
    auto trace = [&](int c, float s) { r.tr_f[c] = f1; r.tr_shift[c] = shift1; r.tr_sync[c] = s; };
    float fstep = 0.0;
    int ifmin = 0, ifmax = 0;
    int lagmin = shift1 - 128, lagmax = shift1 + 128, lagstep = 64;                                         // :759-764
    sync_and_demodulate(idat, qdat, TPOINTS, w_symbols, &f1, ifmin, ifmax, fstep, &shift1, lagmin, lagmax, lagstep, drift1, symfac, &sync1, MODE_LAG, mg);
    trace(0, sync1);
    fstep = 0.25; ifmin = -2; ifmax = 2;                                                                    // :766-768
    sync_and_demodulate(idat, qdat, TPOINTS, w_symbols, &f1, ifmin, ifmax, fstep, &shift1, lagmin, lagmax, lagstep, drift1, symfac, &sync1, MODE_FREQ, mg);
    trace(1, sync1);
    fstep = 0.0; ifmin = 0; ifmax = 0;                                                                      // :771-779
    float syncp, syncm;
    const float driftp = drift1 + 0.5;
    sync_and_demodulate(idat, qdat, TPOINTS, w_symbols, &f1, ifmin, ifmax, fstep, &shift1, lagmin, lagmax, lagstep, driftp, symfac, &syncp, MODE_FREQ);
    trace(2, syncp);
    const float driftm = drift1 - 0.5;
    sync_and_demodulate(idat, qdat, TPOINTS, w_symbols, &f1, ifmin, ifmax, fstep, &shift1, lagmin, lagmax, lagstep, driftm, symfac, &syncm, MODE_FREQ);
    trace(3, syncm);
    if (syncp > sync1) { drift1 = driftp; sync1 = syncp; }                                                  // :781-789
    else if (syncm > sync1) { drift1 = driftm; sync1 = syncm; }
    const bool r_minsync1 = sync1 > KG_WSPR_DEC_MINSYNC1;                                                       // :795
    if (r_minsync1) {
        lagmin = shift1 - 32; lagmax = shift1 + 32; lagstep = 16;                                           // :798-805
        sync_and_demodulate(idat, qdat, TPOINTS, w_symbols, &f1, ifmin, ifmax, fstep, &shift1, lagmin, lagmax, lagstep, drift1, symfac, &sync1, MODE_LAG, mg);
        trace(4, sync1);
        fstep = 0.05; ifmin = -2; ifmax = 2;
        sync_and_demodulate(idat, qdat, TPOINTS, w_symbols, &f1, ifmin, ifmax, fstep, &shift1, lagmin, lagmax, lagstep, drift1, symfac, &sync1, MODE_FREQ, mg);
        trace(5, sync1);
    } else *ignore = 1;                                                                                     // :807
    int idt = 0, ii = 0, jiggered_shift = 0, r_decoded = 0, gates = 0;
    float rms = 0.0;
    bool r_tooWeak = true;
    uint32_t metric = 0, cycles = 0, maxnp = 0;
    uint8_t decdata[LEN_DECODE] = {0};
    while (r_minsync1 && !r_decoded && idt <= (JIG_RANGE / iifac)) {                                        // :819-867
        ii = ii_of(idt, iifac);
        jiggered_shift = shift1 + ii;
        float pre[NSYM];
        sync_and_demodulate(idat, qdat, TPOINTS, w_symbols, &f1, ifmin, ifmax, fstep, &jiggered_shift, lagmin, lagmax, lagstep, drift1, symfac, &sync1, MODE_SOFT,
                            nullptr, pre);
        if (watch) {
            memcpy(watch->jig_syms[watch->njig++], w_symbols, NSYM);
            for (int i = 0; i < NSYM; i++) {
                const float d = fabsf(pre[i] - rintf(pre[i]));
                if (pre[i] > -128 && pre[i] < 127 && pre[i] != 0 && d < watch->int_dist) watch->int_dist = d;        // an exact 0: a symbol without samples
            }
        }
        float sq = 0.0;
        for (int i = 0; i < NSYM; i++) rms_step(sq, w_symbols[i]);
        rms = rms_of(sq);
        if (gate_of(sync1, rms)) {
            deinterleave(w_symbols);
            r_decoded = fano_host(w_symbols, mettab, maxcycles, &metric, &cycles, &maxnp, decdata);
            r_tooWeak = false;
            gates++;
        }
        idt++;
        if (quickmode) break;
    }
    const bool r_timeUp = r_minsync1 && !r_decoded && idt > (JIG_RANGE / iifac);                            // :869
    if (r_timeUp && r_tooWeak) *ignore = 1;                                                                 // :873-875
    if (r_decoded) *ignore = 1;                                                                             // :883
    r.result = !r_minsync1 ? R_MINSYNC1 : r_decoded ? R_DECODED : (r_timeUp && r_tooWeak) ? R_NO_CHANGE : r_timeUp ? R_TIME_UP : R_QUICK_MISS;
    r.ignore = *ignore;
    r.f1 = f1; r.shift1 = shift1; r.drift1 = drift1; r.sync1 = sync1;
    r.idt = idt; r.ii = ii; r.jig_shift = jiggered_shift; r.gates = gates; r.rms = rms;
    r.metric = metric; r.cycles = cycles; r.maxnp = maxnp;
    memcpy(r.decdata, decdata, LEN_DECODE);
    if (idt > 0) memcpy(r.symbols, w_symbols, NSYM);
}
#endif  // host

}  // namespace kg_wspr_df
#endif
