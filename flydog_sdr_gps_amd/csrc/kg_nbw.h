// kg_nbw.h -- NB_WILD, the second algorithm of c2s_sound()'s noise-blanker switch (rx/rx_sound.cpp:922-931 -> rx/Teensy/NB_Wild.cpp,
// Michael Wild's LPC blanker: find impulses in the LPC residual, replace them by forward and backward prediction), on the device AND
// the host, in the reference's own operand types like kg_nrs.h: everything float except the two places where NB_Wild.cpp writes a
// double literal (R[0] * (1.0 + 1.0e-9), :112; the windows 1.0 * i / (impulse_length - 1), :97).  Library and host driver are built
// with -ffp-contract=off.  What lives here:
//   * nb_Wild_init's conversions (:38-46) and the rule for a vector the stage can run on;
//   * the eight CMSIS routines the file calls, as the scalar loops the reference's build compiles (no ARM_MATH_LOOPUNROLL / NEON /
//     MVEF): arm_dot_prod_f32, arm_fir_f32 from a zeroed state, arm_var_f32 (two passes), arm_power_f32, and negate / mult / add as
//     single expressions.  Every sum is one accumulator walked in index order;
//   * Levinson-Durbin (:111-139), the threshold (:160), the scan (:162-176) and one hit's repair (:193-235) as written;
//   * a plain serial restatement of nb_Wild_process with WORKING_BUFFER (the host driver's, and the definition the kernel is split from).
#ifndef KG_NBW_H
#define KG_NBW_H
#include <math.h>
#include <string.h>

#include "kg_nr.h"

namespace kg_nbw {

enum { BLOCK = 512 };                                          // ns_out at the call site (FASTFIR_OUTBUF_SIZE)
enum { MAX_ORDER = 40, MAX_IMPULSE_LEN = 41, MAX_PL = (MAX_IMPULSE_LEN - 1) / 2 };       // NB_Wild.cpp:23-25
enum { DIM_WBUF = BLOCK + MAX_ORDER * 2 + MAX_PL * 2 };        // :29
enum { HIST_MAX = MAX_ORDER * 2 + MAX_PL * 2 };                // what a call carries to the next (:242)
enum { N_IMPULSE_COUNT = 20 };                                 // :75
enum { P_THRESH = 0, P_TAPS = 1, P_SAMPLES = 2 };              // NB_THRESH, NB_TAPS, NB_SAMPLES (noise_blank.h)

// One channel's nb_Wild_t (:18-34) and the stage's switch.  Of working_buffer only the first 2 * order + 2 * PL floats outlive a
// call (the rest is rewritten before it is read), so only they are kept.
struct state_t {
    float thresh;
    int taps, impulse_samples;
    int on;                           // nb_enable[NB_BLANKER] && nb_algo == NB_WILD, held by the caller (kg_post_set_nbw)
    float hist[HIST_MAX];
};

// (s1_t) of a float (:43-44).  Outside signed char the conversion is undefined in C: recorded as 0, which no stage runs on.
inline int to_s1(float v) { return (v > -129.0f && v < 128.0f) ? (int) (signed char) v : 0; }

// nb_Wild_init (:38-46) without the memset, which is the caller's
inline void init_params(state_t &s, const float nb_param[kg_nr::NPARAMS])
{
    s.thresh = nb_param[P_THRESH];
    s.taps = to_s1(nb_param[P_TAPS]);
    s.impulse_samples = to_s1(nb_param[P_SAMPLES]);
}

// The vectors the stage runs on: taps = 0 or impulse_samples < 2 make the windows 0/0 and NaN samples reach the output; beyond 40 /
// 41 the file indexes outside working_buffer.
inline bool usable(const state_t &s)
{
    return s.taps >= 1 && s.taps <= MAX_ORDER && s.impulse_samples >= 2 && s.impulse_samples <= MAX_IMPULSE_LEN &&
           s.thresh - s.thresh == 0.0f;
}

KG_NR_HD int impulse_length(int impulse_samples) { return impulse_samples | 1; }      // :66
KG_NR_HD int half_length(int il) { return (il - 1) / 2; }                             // PL, :67

// ---- the CMSIS routines, scalar form ----
// arm_dot_prod_f32
template <typename A, typename B> KG_NR_HD float dot(const A &a, const B &b, int n)
{
    float sum = 0.0f;
    for (int i = 0; i < n; i++) sum += a[i] * b[i];
    return sum;
}

// Output n of arm_fir_f32 with numTaps coefficients c on a state that arm_fir_init_f32 zeroed: the numTaps - 1 samples before x[0]
// are 0.0f and are multiplied like any other (0 * NaN is NaN).
template <typename X, typename C> KG_NR_HD float fir_sample(const X &x, int n, const C &c, int numTaps)
{
    float acc0 = 0.0f;
    for (int i = 0; i < numTaps; i++) {
        const int k = n - (numTaps - 1) + i;
        const float v = k < 0 ? 0.0f : x[k];
        acc0 += v * c[i];
    }
    return acc0;
}

// arm_var_f32, blockSize > 1
template <typename X> KG_NR_HD float variance(const X &x, int n)
{
    float sum = 0.0f, fSum = 0.0f;
    for (int i = 0; i < n; i++) sum += x[i];
    const float fMean = sum / (float) n;
    for (int i = 0; i < n; i++) {
        const float fValue = x[i] - fMean;
        fSum += fValue * fValue;
    }
    return fSum / (float) ((float) n - 1.0f);
}

// arm_power_f32
template <typename X> KG_NR_HD float power(const X &x, int n)
{
    float sum = 0.0f;
    for (int i = 0; i < n; i++) { const float in = x[i]; sum += in * in; }
    return sum;
}

// ---- the stage's own steps ----
// R[i] of :102-109: x is &working_buffer[order + PL]
template <typename X> KG_NR_HD float autocorr(const X &x, int i, int nsamps) { return dot(x, x + i, nsamps - i); }

// :111-143.  R[0] is scaled in place; lpcs[0..order] and reverse_lpcs[0..order] are written; any[] is scratch.
template <typename F> KG_NR_HD void levinson(F R, int order, F lpcs, F reverse_lpcs, F any)
{
    R[0] = R[0] * (1.0 + 1.0e-9);
    lpcs[0] = 1;
    for (int i = 1; i < order + 1; i++) lpcs[i] = 0;
    float alfa = R[0];
    for (int m = 1; m <= order; m++) {
        float s = 0.0;
        for (int u = 1; u < m; u++) s = s + lpcs[u] * R[m - u];
        const float k = -(R[m] + s) / alfa;
        for (int v = 1; v < m; v++) any[v] = lpcs[v] + k * lpcs[m - v];
        for (int w = 1; w < m; w++) lpcs[w] = any[w];
        lpcs[m] = k;
        alfa = alfa * (1 - k * k);
    }
    for (int o = 0; o < order + 1; o++) reverse_lpcs[order - o] = lpcs[o];
}

KG_NR_HD float threshold(float thresh, float sigma2, float lpc_power) { return thresh * sqrtf(sigma2 * lpc_power); }     // :160

// :167, the test of one filtered sample
KG_NR_HD bool over(float t, float impulse_threshold) { return (t > impulse_threshold) || (t < (-impulse_threshold)); }

// :162-176 over the tests of all the block's samples, 64 to a word (bit i of flags[w] is sample 64 w + i): at most N_IMPULSE_COUNT
// positions, each already corrected by the filter delay.  The walk is the reference's do-while; samples whose flag is clear are
// stepped over a word at a time, which finds the same positions (a test's outcome does not depend on the walk).
template <typename M, typename P> KG_NR_HD int scan_flags(const M &flags, int order, int PL, int nsamps, P positions)
{
    int search_pos = order + PL, impulse_count = 0;
    do {
        const unsigned long long rest = flags[search_pos >> 6] >> (search_pos & 63);
        if (rest == 0) { search_pos = ((search_pos >> 6) + 1) << 6; continue; }
        search_pos += __builtin_ctzll(rest);
        positions[impulse_count] = search_pos - order;
        impulse_count++;
        search_pos += PL;
        search_pos++;
    } while ((search_pos < nsamps) && (impulse_count < N_IMPULSE_COUNT));
    return impulse_count;
}

// host: the flags, then the walk
template <typename X, typename P> inline int scan(const X &tempsamp, float impulse_threshold, int order, int PL, int nsamps, P positions)
{
    unsigned long long flags[BLOCK / 64];
    for (int w = 0; w < nsamps / 64; w++) {
        flags[w] = 0;
        for (int i = 0; i < 64; i++) flags[w] |= (unsigned long long) over(tempsamp[64 * w + i], impulse_threshold) << i;
    }
    return scan_flags(flags, order, PL, nsamps, positions);
}

// Wbw[i] of :96-99 (Wfw[i] is Wbw[il - 1 - i]); impulse_length is a u4_t there
KG_NR_HD float window_bw(int i, int il) { return 1.0 * i / (unsigned) (il - 1); }

// the places one hit reads its two prediction bases from (:196-204) and writes its repair to (:231)
KG_NR_HD int fw_base(int pos, int k) { return pos + k; }
KG_NR_HD int bw_base(int pos, int k, int order, int PL) { return order + PL + pos + PL + k + 1; }
KG_NR_HD int repair_base(int pos, int order) { return order + pos; }

// :221-224, the two chains apart: neg_rev is reverse_lpcs[0 .. order) negated, neg_lpc is lpcs[1 .. order] negated (:187-188)
template <typename F, typename C> KG_NR_HD void predict_fw(F Rfw, const C &neg_rev, int order, int il)
{
    for (int i = 0; i < il; i++) Rfw[i + order] = dot(neg_rev, Rfw + i, order);
}
template <typename F, typename C> KG_NR_HD void predict_bw(F Rbw, const C &neg_lpc, int order, int il)
{
    for (int i = 0; i < il; i++) Rbw[il - i - 1] = dot(neg_lpc, Rbw + (il - i), order);
}
// :226-231 for sample i of the repair: arm_mult_f32 twice, arm_add_f32
KG_NR_HD float blend(float fw, float bw, int i, int il) { const float a = window_bw(il - 1 - i, il) * fw, b = window_bw(i, il) * bw; return a + b; }

// (TYPEMONO16) of the float sample as the reference's x86 build converts it (:260)
KG_NR_HD short out_sample(float v) { return kg_nr::mono16(v); }

// what the host driver records of one call
struct trace_t { int hits; float max_abs; };

// host: nb_Wild_process(ch, 512, in, out) (:60-261), serially; in == out allowed, as the reference is called
inline void process(state_t &s, const short *in, short *out, trace_t *trace = nullptr)
{
    const int nsamps = BLOCK, order = s.taps, il = impulse_length(s.impulse_samples), PL = half_length(il);
    static float wb[DIM_WBUF], tempsamp[BLOCK], temp2[BLOCK];
    float lpcs[MAX_ORDER + 1] = {0}, reverse_lpcs[MAX_ORDER + 1] = {0}, R[MAX_ORDER + 1] = {0}, any[MAX_ORDER + 1] = {0};
    float Rfw[MAX_IMPULSE_LEN + MAX_ORDER], Rbw[MAX_IMPULSE_LEN + MAX_ORDER];
    int positions[N_IMPULSE_COUNT];
    const int hist = 2 * PL + 2 * order;
    memcpy(wb, s.hist, sizeof(float) * hist);
    for (int i = 0; i < nsamps; i++) wb[hist + i] = in[i];                                      // :258, :91
    const float *x = wb + order + PL;
    for (int i = 0; i < order + 1; i++) R[i] = autocorr(x, i, nsamps);
    levinson((float *) R, order, (float *) lpcs, (float *) reverse_lpcs, (float *) any);
    for (int n = 0; n < nsamps; n++) tempsamp[n] = fir_sample(x, n, reverse_lpcs, order + 1);   // :149
    for (int n = 0; n < nsamps; n++) temp2[n] = fir_sample(tempsamp, n, lpcs, order + 1);       // :155 (in place there: the state holds the input)
    const float sigma2 = variance(temp2, nsamps), lpc_power = power(lpcs, order);
    const int count = scan(temp2, threshold(s.thresh, sigma2, lpc_power), order, PL, nsamps, positions);
    for (int k = 0; k < order; k++) { lpcs[1 + k] = -lpcs[1 + k]; reverse_lpcs[k] = -reverse_lpcs[k]; }
    for (int j = 0; j < count; j++) {
        const int pos = positions[j];
        for (int k = 0; k < order; k++) {
            Rfw[k] = wb[fw_base(pos, k)];
            Rbw[il + k] = wb[bw_base(pos, k, order, PL)];
        }
        predict_fw((float *) Rfw, reverse_lpcs, order, il);
        predict_bw((float *) Rbw, lpcs + 1, order, il);
        for (int i = 0; i < il; i++) wb[repair_base(pos, order) + i] = blend(Rfw[order + i], Rbw[i], i, il);
    }
    float max_abs = 0.0f;
    for (int i = 0; i < nsamps; i++) {
        const float v = wb[order + PL + i];
        if (fabsf(v) > max_abs || v != v) max_abs = v != v ? INFINITY : fabsf(v);
        out[i] = out_sample(v);
    }
    memcpy(s.hist, wb + nsamps, sizeof(float) * hist);                                          // :242
    if (trace) { trace->hits = count; trace->max_abs = max_abs; }
}

}  // namespace kg_nbw
#endif
