// kg_nrs.h -- NR_SPECTRAL, the third algorithm of c2s_sound()'s noise-reduction switch (rx/rx_sound.cpp:945-947 ->
// rx/Teensy/NR_spectral.cpp, the UHSDR spectral-weighting denoiser), on the device AND the host, in the reference's own operand
// types, like kg_nr.h: f32_t members mixed with double literals, restated so that C++ promotes as the reference's compiler does
// (library and host driver are built with -ffp-contract=off).  What lives here:
//   * nr_spectral_init's derivation (:103-108), the file-scope rate constants (:89-93), the passband bins VAD_low / VAD_high with
//     their clamps (:214-238) and norm_locut / norm_hicut as rx_sound_cmd.cpp:252-266 forms them;
//   * the per-bin expressions of the start-up phase (:177-178) and of phase 3 (:195-204, :210-211, :257-260), NN (:274-282) and the
//     three smoothing loops (:284-314) as one bin's ordered sums;
//   * the 512-point transform the reference calls (CMSIS arm_cfft_f32 -> arm_radix8_butterfly_f32, fftLen 512): three radix-8
//     passes of 64 butterflies, each butterfly one fixed tree of float adds and multiplies, twiddles from KG_NRS_TW (kg_tables.h:
//     OUR table), the digit reversal, the inverse's conjugate and scale.  The same tree gives the same bits;
//   * a plain serial restatement of nr_spectral_process (the host driver's, and the definition the kernel is split from).
#ifndef KG_NRS_H
#define KG_NRS_H
#include <math.h>
#include <string.h>

#include "kg_nr.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define KG_NRS_EXPF(x) kg_libm::expf_glibc(x)     // the host libm's expf, bit for bit (kg_libm.h)
#else
#define KG_NRS_EXPF(x) expf(x)
#endif

namespace kg_nrs {

enum { FFT_FULL = 512, FFT_HALF = 256 };                  // NR_spectral.cpp:30-31
enum { P_GAIN = 0, P_ALPHA = 1, P_ASNR = 2 };             // NR_S_GAIN, NR_ALPHA, NR_ASNR (noise_filter.h:24-26)
enum { NR_WIDTH = 4, INIT_FRAMES = 20 };                  // :123, :182
// the passbands on which the smoothing loops (:284-314) stay inside NR_G[256] / NR_Nest[256] for every NN <= 9
enum { VAD_HIGH_MIN = 17, VAD_LOW_MAX = 244 };

struct par_t {                    // the scalars nr_spectral_init writes (:103-108)
    float final_gain, alpha, asnr, xih1, xih1r, pfac;
};
struct rate_t {                   // the file-scope tinc .. ap (:75-79, :89-93) and snr_prio_min (:122), one set per kg_post
    float tinc, tax, tap, ax, ap, snr_prio_min;
};
// One channel's nr_spectral_t (:41-67).  first_time and init_counter advance on the device; the host writes them at the first
// init only.  vad_lo / vad_hi are VAD_low / VAD_high (:214-238), derived on the host whenever the passband or the rate changes.
struct state_t {
    int first_time, init_counter;
    int vad_lo, vad_hi;
    par_t par;
    float pad[2];
    float last_sample_buffer[FFT_HALF], last_iFFT_result[FFT_HALF];
    float NR_Nest[FFT_HALF], xt[FFT_HALF], pslp[FFT_HALF], NR_SNR_post[FFT_HALF], NR_SNR_prio[FFT_HALF], NR_Hk_old[FFT_HALF], NR_G[FFT_HALF];
};

// ---- host: the commands ----
// :103-108.  xih1r = 1.0 / (1.0 + xih1) - 1.0 and pfac = (1.0 / pspri - 1.0) * (1.0 + xih1) are double, rounded on assignment;
// pspri is a const f32_t (0.5).
inline void init_params(par_t &s, const float nr_param[kg_nr::NPARAMS])
{
    const float pspri = 0.5;
    s.final_gain = nr_param[P_GAIN];
    s.alpha = nr_param[P_ALPHA];
    s.asnr = nr_param[P_ASNR];
    s.xih1 = s.asnr;
    s.xih1r = 1.0 / (1.0 + s.xih1) - 1.0;
    s.pfac = (1.0 / pspri - 1.0) * (1.0 + s.xih1);
}

// the first init of a channel (:86-100): first_time = 1 and four seeded arrays
inline void init_first(state_t &s)
{
    s.first_time = 1;
    for (int b = 0; b < FFT_HALF; b++) {
        s.last_sample_buffer[b] = 0.1;
        s.NR_Hk_old[b] = 0.1;
        s.NR_SNR_post[b] = 2.0;
        s.NR_SNR_prio[b] = 1.0;
    }
}

// :89-93 and :121-122 with the host's libm; snd_rate is the reference's int global
inline rate_t rate_consts(int snd_rate)
{
    rate_t r;
    r.tinc = 1.0 / ((float) snd_rate / FFT_FULL * 2);
    r.tax = -r.tinc / logf(0.8);
    r.tap = -r.tinc / logf(0.9);
    r.ax = expf(-r.tinc / r.tax);
    r.ap = expf(-r.tinc / r.tap);
    const float snr_prio_min_dB = -30;
    r.snr_prio_min = powf(10, snr_prio_min_dB / 10.0);
    return r;
}

// rx_sound_cmd.cpp:252-266 from the clamped cuts (s->locut, s->hicut: double; norm_*: float)
inline void norm_passband(double locut, double hicut, float &norm_locut, float &norm_hicut)
{
    if (locut <= 0 && hicut >= 0) {
        norm_locut = 0.0;
        norm_hicut = (-locut) > (hicut) ? (-locut) : (hicut);       // MAX(-s->locut, s->hicut)
    } else if (locut > 0) {
        norm_locut = locut;
        norm_hicut = hicut;
    } else {
        norm_hicut = -locut;
        norm_locut = -hicut;
    }
}

// (int) of a float as x86 converts it: INT_MIN outside int and for NaN
inline int to_int(float v) { return (v > -2147483904.0f && v < 2147483648.0f) ? (int) v : (int) 0x80000000u; }

// :214-238
inline void vad_bins(float norm_locut, float norm_hicut, int snd_rate, int &VAD_low, int &VAD_high)
{
    VAD_low = to_int(floorf(norm_locut / ((float) snd_rate / FFT_FULL)));
    VAD_high = to_int(ceilf(norm_hicut / ((float) snd_rate / FFT_FULL)));
    if (VAD_low == VAD_high) VAD_high = (int) ((unsigned) VAD_high + 1u);
    if (VAD_low < 1) VAD_low = 1;
    else if (VAD_low > FFT_HALF - 2) VAD_low = FFT_HALF - 2;
    if (VAD_high < 2) VAD_high = 2;
    else if (VAD_high > FFT_HALF) VAD_high = FFT_HALF;
}
// the reference indexes outside its arrays on some NN unless this holds (m down to VAD_high - 2 NN + 1, up to VAD_low + NN/2 + NN - 2)
inline bool vad_ok(int VAD_low, int VAD_high) { return VAD_high >= VAD_HIGH_MIN && VAD_low <= VAD_LOW_MAX; }

// ---- the per-bin expressions (host and device) ----
KG_NR_HD float mag2(float re, float im) { return re * re + im * im; }                     // :170

// first_time == 2 (:177-178): NR_Nest + 0.05 * NR_X in double; psini is a const f32_t
KG_NR_HD void startup_bin(float X, float &Nest, float &xt)
{
    const float psini = 0.5;
    Nest = Nest + 0.05 * X;
    xt = psini * Nest;
}

// :195-204: speech presence and the noise estimate of one bin
KG_NR_HD void track_bin(const par_t &s, float ap, float ax, float X, float &xt, float &pslp)
{
    const float psthr = 0.99, pnsaf = 0.01;
    float ph1y = 1.0 / (1.0 + s.pfac * KG_NRS_EXPF(s.xih1r * X / xt));
    pslp = ap * pslp + (1.0 - ap) * ph1y;
    if (pslp > psthr)
        ph1y = 1.0 - pnsaf;
    else
        ph1y = fmin((double) ph1y, 1.0);
    const float xtr = (1.0 - ph1y) * X + ph1y * xt;
    xt = ax * xt + (1.0 - ax) * xtr;
}

// :210-211
KG_NR_HD void snr_bin(const par_t &s, float snr_prio_min, float X, float xt, float Hk_old, float &post, float &prio)
{
    post = fmax(fmin((double) (X / xt), 1000.0), (double) snr_prio_min);
    prio = fmax(s.alpha * Hk_old + (1.0 - s.alpha) * fmax(post - 1.0, 0.0), 0.0);
}

// :257-260 (GAIN_LIMIT 0.001)
KG_NR_HD void gain_bin(float post, float prio, float &G, float &Hk_old)
{
    const float v = prio * post / (1.0 + prio);
    G = fmax(1.0 / post * sqrtf((float) (0.7212 * v + v * v)), 0.001);
    Hk_old = post * G * G;
}

// :269-270, one step of the two serial sums
KG_NR_HD void power_step(float X, float G, float &pre_power, float &post_power)
{
    pre_power += X;
    post_power += G * G * X;
}

// :273-282.  On a frame of digital silence power_ratio is 0/0: the comparison is false and (int) of a NaN-valued double is
// undefined; the reference's x86 build converts to INT_MIN, the doubling wraps to 0 and NN = 1.  Same convention as kg_nr::mono16.
KG_NR_HD int smoothing_width(float pre_power, float post_power)
{
    const float power_threshold = 0.4;
    const float power_ratio = post_power / pre_power;
    if (power_ratio > power_threshold) return 1;
    const double d = 0.5 + NR_WIDTH * (1.0 - power_ratio / power_threshold);
    if (!(d > -2147483649.0 && d < 2147483648.0)) return 1;
    return (int) (1u + 2u * (unsigned) (int) d);
}

// :284-314 for one bin: the three loops read NR_G only and write NR_Nest[bindx] only, in the order middle, lower edge, upper edge;
// a bin inside more than one range keeps the last loop's value.  Returns false when no loop writes the bin.  G is indexed inside
// [0, 256) for every NN <= 9 on a passband that passes vad_ok().
template <typename GP>
KG_NR_HD bool smooth_bin(const GP &G, int bindx, int VAD_low, int VAD_high, int NN, float &Nest)
{
    const int h = NN / 2;
    bool hit = false;
    if (bindx >= VAD_low + h && bindx < VAD_high - h) {
        float a = 0.0;
        for (int m = bindx - h; m <= bindx + h; m++) a += G[m];
        Nest = a / (float) NN;
        hit = true;
    }
    if (bindx >= VAD_low && bindx < VAD_low + h) {
        float a = 0.0;
        for (int m = bindx; m < bindx + NN; m++) a += G[m];
        Nest = a / (float) NN;
        hit = true;
    }
    if (bindx >= VAD_high - NN && bindx < VAD_high) {
        float a = 0.0;
        for (int m = bindx; m > bindx - NN; m--) a += G[m];
        Nest = a / (float) NN;
        hit = true;
    }
    return hit;
}

// :351: roundf((re + last) * final_gain) into TYPEMONO16
KG_NR_HD short out_sample(float re, float last, float final_gain) { return kg_nr::mono16(roundf((re + last) * final_gain)); }

// ---- the transform ----
// One radix-8 butterfly of arm_radix8_butterfly_f32 on the eight points i1 + k * n2, in place, before its twiddles: sums and
// differences of the pairs (k, k + 4), the even outputs from the sums, the odd ones from the differences through C81.
KG_NR_HD void bfly8(float *xr, float *xi)
{
    const float C81 = 0.70710678118f;
    const float a0 = xr[0] + xr[4], b0 = xr[0] - xr[4], a1 = xr[1] + xr[5], b1 = xr[1] - xr[5];
    const float a2 = xr[2] + xr[6], b2 = xr[2] - xr[6], a3 = xr[3] + xr[7], b3 = xr[3] - xr[7];
    const float c0 = xi[0] + xi[4], d0 = xi[0] - xi[4], c1 = xi[1] + xi[5], d1 = xi[1] - xi[5];
    const float c2 = xi[2] + xi[6], d2 = xi[2] - xi[6], c3 = xi[3] + xi[7], d3 = xi[3] - xi[7];
    const float e0 = a0 + a2, e1 = a0 - a2, e2 = a1 + a3, e3 = a1 - a3;
    const float f0 = c0 + c2, f1 = c0 - c2, f2 = c1 + c3, f3 = c1 - c3;
    xr[0] = e0 + e2; xi[0] = f0 + f2;
    xr[4] = e0 - e2; xi[4] = f0 - f2;
    xr[2] = e1 + f3; xi[2] = f1 - e3;
    xr[6] = e1 - f3; xi[6] = f1 + e3;
    const float g0 = (b1 - b3) * C81, g1 = (b1 + b3) * C81, h0 = (d1 - d3) * C81, h1 = (d1 + d3) * C81;
    const float p0 = b0 - g0, p1 = b0 + g0, p2 = b2 - g1, p3 = b2 + g1;
    const float q0 = d0 - h0, q1 = d0 + h0, q2 = d2 - h1, q3 = d2 + h1;
    xr[1] = p1 + q3; xi[1] = q1 - p3;
    xr[7] = p1 - q3; xi[7] = q1 + p3;
    xr[5] = p0 + q2; xi[5] = q0 - p2;
    xr[3] = p0 - q2; xi[3] = q0 + p2;
}

// the twiddle of output k of the butterfly with offset j in a pass with modifier m: table entry k * j * m, applied as
// (co * re + si * im, co * im - si * re).  Butterflies with j == 0 and the whole last pass carry none (not a multiply by one).
KG_NR_HD void twiddle(float &re, float &im, float co, float si)
{
    const float r = co * re + si * im, i = co * im - si * re;
    re = r; im = i;
}

// Butterfly `bf` (0..63) of pass `pass` (0..2: n2 = 64, 8, 1): its first point i1 and the stride n2 of its eight points
KG_NR_HD void bfly_index(int pass, int bf, int &i1, int &n2, int &j, int &mod)
{
    n2 = pass == 0 ? 64 : pass == 1 ? 8 : 1;
    mod = pass == 0 ? 1 : 8;
    j = bf & (n2 - 1);
    i1 = j + (bf / n2) * n2 * 8;
}

// reversal of the three base-8 digits (the bit-reversal table's pairs, applied as out[rev(i)] = in[i])
KG_NR_HD int rev3(int i) { return ((i & 7) << 6) | (i & 0x38) | (i >> 6); }

// one butterfly with its twiddles, on the eight points the caller loaded from i1 + k * n2 (bfly_index) and stores back there
KG_NR_HD void bfly_compute(int pass, int j, int mod, const float (*tw)[2], float *xr, float *xi)
{
    bfly8(xr, xi);
    if (pass < 2 && j != 0)
        for (int k = 1; k < 8; k++) twiddle(xr[k], xi[k], tw[k * j * mod][0], tw[k * j * mod][1]);
}

// host: arm_cfft_f32(S_len512, buf, ifftFlag, 1) on buf[512][2], serially
inline void cfft512(float (*buf)[2], const float (*tw)[2], bool inverse)
{
    if (inverse) for (int i = 0; i < FFT_FULL; i++) buf[i][1] = -buf[i][1];
    for (int pass = 0; pass < 3; pass++)
        for (int bf = 0; bf < 64; bf++) {
            int i1, n2, j, mod;
            float xr[8], xi[8];
            bfly_index(pass, bf, i1, n2, j, mod);
            for (int k = 0; k < 8; k++) { xr[k] = buf[i1 + k * n2][0]; xi[k] = buf[i1 + k * n2][1]; }
            bfly_compute(pass, j, mod, tw, xr, xi);
            for (int k = 0; k < 8; k++) { buf[i1 + k * n2][0] = xr[k]; buf[i1 + k * n2][1] = xi[k]; }
        }
    for (int i = 0; i < FFT_FULL; i++) {
        const int r = rev3(i);
        if (i < r) {
            const float t0 = buf[i][0], t1 = buf[i][1];
            buf[i][0] = buf[r][0]; buf[i][1] = buf[r][1];
            buf[r][0] = t0; buf[r][1] = t1;
        }
    }
    if (inverse) {
        const float invL = 1.0f / (float) FFT_FULL;
        for (int i = 0; i < FFT_FULL; i++) { buf[i][0] *= invL; buf[i][1] = -(buf[i][1]) * invL; }
    }
}

// what the host driver records of one call: NN of its phase-3 frames in order, and how many of them had a NaN power_ratio
struct trace_t { int nn[2], frames, nan_ratio; };

// host: nr_spectral_process(ch, 512, in, out) (:112-359), serially; in == out allowed, as the reference is called
inline void process(state_t &s, const rate_t &rt, const float (*tw)[2], const float *win, const short *in, short *out, trace_t *trace = nullptr)
{
    if (trace) memset(trace, 0, sizeof *trace);
    static float buf[FFT_FULL][2];
    float X[FFT_HALF];
    if (s.first_time == 1) {                                            // :126-135
        for (int b = 0; b < FFT_HALF; b++) {
            s.last_sample_buffer[b] = 0.0;
            s.NR_G[b] = 1.0;
            s.NR_Hk_old[b] = 1.0;
            s.NR_Nest[b] = 0.0;
            s.pslp[b] = 0.5;
        }
        s.first_time = 2;
    }
    for (int k = 0; k < 2; k++) {
        int VAD_low = 0, VAD_high = 0;
        for (int i = 0; i < FFT_HALF; i++) {                            // :140-156
            buf[i][0] = s.last_sample_buffer[i]; buf[i][1] = 0.0;
        }
        for (int i = 0; i < FFT_HALF; i++) {
            const float f_samp = (float) in[i + k * FFT_HALF];
            s.last_sample_buffer[i] = f_samp;
            buf[FFT_HALF + i][0] = f_samp; buf[FFT_HALF + i][1] = 0.0;
        }
        for (int i = 0; i < FFT_FULL; i++) buf[i][0] *= win[i / 2];     // :159-161
        cfft512(buf, tw, false);
        for (int b = 0; b < FFT_HALF; b++) X[b] = mag2(buf[b][0], buf[b][1]);
        if (s.first_time == 2) {                                        // :173-186
            for (int b = 0; b < FFT_HALF; b++) startup_bin(X[b], s.NR_Nest[b], s.xt[b]);
            s.init_counter = (s.init_counter + 1) & 255;
            if (s.init_counter > INIT_FRAMES - 1) { s.init_counter = 0; s.first_time = 3; }
        }
        if (s.first_time == 3) {
            for (int b = 0; b < FFT_HALF; b++) track_bin(s.par, rt.ap, rt.ax, X[b], s.xt[b], s.pslp[b]);
            for (int b = 0; b < FFT_HALF; b++) snr_bin(s.par, rt.snr_prio_min, X[b], s.xt[b], s.NR_Hk_old[b], s.NR_SNR_post[b], s.NR_SNR_prio[b]);
            VAD_low = s.vad_lo; VAD_high = s.vad_hi;                    // :214-238, derived when the passband was set
            for (int b = VAD_low; b < VAD_high; b++) gain_bin(s.NR_SNR_post[b], s.NR_SNR_prio[b], s.NR_G[b], s.NR_Hk_old[b]);
            float pre_power = 0.0, post_power = 0.0;
            for (int b = VAD_low; b < VAD_high; b++) power_step(X[b], s.NR_G[b], pre_power, post_power);
            const int NN = smoothing_width(pre_power, post_power);
            if (trace) { trace->nn[trace->frames++] = NN; trace->nan_ratio += !(post_power / pre_power == post_power / pre_power); }
            for (int b = 0; b < FFT_HALF; b++) smooth_bin(s.NR_G, b, VAD_low, VAD_high, NN, s.NR_Nest[b]);
            for (int b = VAD_low + NN / 2; b < VAD_high - NN / 2; b++) s.NR_G[b] = s.NR_Nest[b];        // :317-320
        }
        for (int b = VAD_low; b < VAD_high; b++) {                      // :329-338 (bin 511 - b, as written)
            buf[b][0] *= s.NR_G[b]; buf[b][1] *= s.NR_G[b];
            const int ai = FFT_FULL - b - 1;
            buf[ai][0] *= s.NR_G[b]; buf[ai][1] *= s.NR_G[b];
        }
        cfft512(buf, tw, true);
        for (int i = 0; i < FFT_FULL; i++) buf[i][0] *= win[i / 2];
        for (int i = 0; i < FFT_HALF; i++) out[i + k * FFT_HALF] = out_sample(buf[i][0], s.last_iFFT_result[i], s.par.final_gain);
        for (int i = 0; i < FFT_HALF; i++) s.last_iFFT_result[i] = buf[FFT_HALF + i][0];
    }
}

}  // namespace kg_nrs
#endif
