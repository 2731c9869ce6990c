// kg_iqd.h -- the IQ display extension (extensions/IQ_display/iq_display.cpp with rx/kiwi/pll.h), the most used consumer of
// receive_iq_samps(PRE_AGC): CFastFIR's output of every sound block.  On the device AND the host, in the reference's own operand
// types, mixed float / double expressions kept as written; library and host driver are built with -ffp-contract=off.  What lives here:
//   * pll (pll.h:8-54): init() -- host arithmetic in mixed float / double with std::tan on a float -- and update(): the phase taken
//     fmod 16 pi, std::arg(sample * std::exp(complex(0, -phase))), the two-tap loop filter into df;
//   * process_sample (:43-69): the PLL(s) on sample * sample (MSK) or std::pow(sample, exponent) -- in this image's <complex> that is
//     __complex_pow_unsigned: repeated squaring with float complex multiplies, no logarithm --, the recovered carrier, multiply
//     (display_mode 0) or replace, then cma, ama and maN;
//   * to_u1 (:37-42): the scale a DOUBLE expression stored to float -- 255 * (gain * (ch ? 20 : 1) / 32767) or, with gain 0,
//     255 * (1.0f / (4.0 * ama)) with the ama of THAT sample --, std::min / std::max semantics (a NaN becomes 255: silence under
//     auto gain is 0 * inf), then u1_t(float);
//   * display_data (:71-112): the ring, plot / map / iq, the rows, nsamp and the text message's four numbers;
//   * the commands (:114-192, :256-273).
// A complex multiply is the compiler's naive (ac - bd, ad + bc); std::abs is (float) sqrt((double) x * x + (double) y * y);
// std::exp(complex(0, t)) is (cosf t, sinf t).  OUTSIDE the contract: NaN or infinite samples, and overflow to infinity inside the
// power (|s|^8 needs |s| < 6e4) -- there the compiler's multiply falls back to libgcc's recovery routine, which is not restated.
// Refused (nothing changed): a negative exponent (`pll_mode <= 1`, arg < 0: the division is libgcc's; not ported) and points
// outside 1 .. 16384 (the reference then leaves its arrays or sends a negative length).
#ifndef KG_IQD_H
#define KG_IQD_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "kg_nr.h"
#if defined(__HIPCC__)
#include "kg_libm_trig.h"
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KG_IQD_SINF(x) kg_libm::sinf_glibc(x)          // the host libm's, bit for bit (kg_libm_trig.h)
#define KG_IQD_COSF(x) kg_libm::cosf_glibc(x)
#define KG_IQD_ATAN2F(y, x) kg_libm::atan2f_glibc(y, x)
#define KG_IQD_FMODF(x, y) kg_iqd_cf::fmodf_exact(x, y)
#else
#define KG_IQD_SINF(x) sinf(x)
#define KG_IQD_COSF(x) cosf(x)
#define KG_IQD_ATAN2F(y, x) atan2f(y, x)
#define KG_IQD_FMODF(x, y) fmodf(x, y)
#endif

namespace kg_iqd_cf {

enum { RING = 16384, NCH = 2, MAX_NS = 512 };          // N_IQ_RING, N_CH (:25-26); a sound block is at most 512 samples
enum { POINTS = 0, DENSITY = 1 };                      // IQ_POINTS, IQ_DENSITY (:21-22)
enum { REFUSED_EXPONENT = -1, REFUSED_POINTS = -2, REFUSED_RATE = -3 };

struct cf { float re, im; };

// x fmod y, exact like the host's fmodf: shift and subtract on the significands.  NaN for x infinite, y zero or either NaN.
KG_NR_HD float fmodf_exact(float x, float y)
{
    uint32_t hx = __builtin_bit_cast(uint32_t, x), hy = __builtin_bit_cast(uint32_t, y) & 0x7fffffffu;
    const uint32_t sx = hx & 0x80000000u;
    hx ^= sx;
    if (hy == 0 || hx >= 0x7f800000u || hy > 0x7f800000u) return (x * y) / (x * y);
    if (hx < hy) return x;
    if (hx == hy) return __builtin_bit_cast(float, sx);
    int ix, iy;
    if (hx < 0x00800000u) { ix = -126; while (hx < 0x00800000u) { hx <<= 1; ix--; } }
    else { ix = (int) (hx >> 23) - 127; hx = 0x00800000u | (hx & 0x007fffffu); }
    if (hy < 0x00800000u) { iy = -126; while (hy < 0x00800000u) { hy <<= 1; iy--; } }
    else { iy = (int) (hy >> 23) - 127; hy = 0x00800000u | (hy & 0x007fffffu); }
    for (int n = ix - iy; n > 0; n--) {
        if (hx >= hy) hx -= hy;
        if (hx == 0) return __builtin_bit_cast(float, sx);
        hx <<= 1;
    }
    if (hx >= hy) hx -= hy;
    if (hx == 0) return __builtin_bit_cast(float, sx);
    while (hx < 0x00800000u) { hx <<= 1; iy--; }
    if (iy >= -126) hx = (hx - 0x00800000u) | ((uint32_t) (iy + 127) << 23);
    else hx >>= (-126 - iy);
    return __builtin_bit_cast(float, hx | sx);
}

// std::abs(complex<float>): the host's hypotf
KG_NR_HD float hypotf_dbl(float x, float y)
{
    const uint32_t ax = __builtin_bit_cast(uint32_t, x) & 0x7fffffffu, ay = __builtin_bit_cast(uint32_t, y) & 0x7fffffffu;
    if (ax >= 0x7f800000u || ay >= 0x7f800000u) {                      // an infinity wins over a quiet NaN, a signalling NaN over both
        const bool sx = ax > 0x7f800000u && !(ax & 0x00400000u), sy = ay > 0x7f800000u && !(ay & 0x00400000u);
        if ((ax == 0x7f800000u || ay == 0x7f800000u) && !sx && !sy) return __builtin_huge_valf();
        return x + y;
    }
    return (float) sqrt((double) x * (double) x + (double) y * (double) y);
}

KG_NR_HD cf cmul(cf a, cf b)
{
    cf r;
    r.re = a.re * b.re - a.im * b.im;
    r.im = a.re * b.im + a.im * b.re;
    return r;
}

// std::pow(complex<float>, int) for a non-negative int
KG_NR_HD cf cpow_u(cf x, unsigned n)
{
    cf one; one.re = 1.0f; one.im = 0.0f;
    cf y = (n & 1u) ? x : one;
    while (n >>= 1) {
        x = cmul(x, x);
        if (n & 1u) y = cmul(y, x);
    }
    return y;
}

struct pll_t { float fs, fc, df, phase, b0, b1, ud; };

// pll::init (pll.h:23-36) with the default damping 1.0f / sqrt(2.0f)
inline void pll_init(pll_t &p, float dwl, float fc, float fs)
{
    const float xi = 1.0f / sqrtf(2.0f);
    const float wn = M_PI * dwl / xi;
    const float tau[2] = {1 / (wn * wn), 2 * xi / wn};
    p.fs = fs;
    const float ts2 = 0.5 / p.fs;
    p.b0 = ts2 / tau[0] * (1 + 1 / tanf(ts2 / tau[1]));
    p.b1 = ts2 / tau[0] * (1 - 1 / tanf(ts2 / tau[1]));
    p.phase = p.ud = p.df = 0;
    p.fc = fc;
}

// pll::update (pll.h:38-44)
KG_NR_HD float pll_update(pll_t &p, cf sample)
{
    p.phase = KG_IQD_FMODF(p.phase + (float) (2 * M_PI * p.fc + p.df) / p.fs, (float) (8 * 2 * M_PI));
    const float ud_old = p.ud;
    const float t = -p.phase;
    cf e; e.re = KG_IQD_COSF(t); e.im = KG_IQD_SINF(t);
    const cf z = cmul(sample, e);
    p.ud = KG_IQD_ATAN2F(z.im, z.re);
    p.df += p.b0 * p.ud + p.b1 * ud_old;
    return p.phase;
}

// the recovered carrier (:50, :54)
KG_NR_HD cf carrier_msk(float phase_plus, float phase_minus)
{
    const float t = -0.25 * (phase_plus + phase_minus);
    cf e; e.re = KG_IQD_COSF(t); e.im = KG_IQD_SINF(t);
    return e;
}
KG_NR_HD cf carrier_single(float phase, int exponent)
{
    const float t = -phase / exponent;
    cf e; e.re = KG_IQD_COSF(t); e.im = KG_IQD_SINF(t);
    return e;
}

// one step of the running means (:65-66): acc is cma.re, cma.im or ama
KG_NR_HD float ma_step(float acc, float v, int maN) { return ((float) maN * acc + v) / (float) (maN + 1); }

// to_u1 (:37-42)
KG_NR_HD float scale_fixed(float gain, int ch) { return 255 * (double) (gain * (ch ? 20 : 1) / (float) ((1 << 15) - 1)); }
KG_NR_HD float scale_auto(float ama) { return 255 * (1.0f / (4.0 * ama)); }
KG_NR_HD unsigned char u1(float v, float scale)
{
    v *= scale;
    const float x = 127 + v;
    const float lo = x < 255.0f ? x : 255.0f;          // std::min(255.0f, x): a NaN gives 255
    const float hi = 0.0f < lo ? lo : 0.0f;            // std::max(0.0f, lo)
    return (unsigned char) hi;
}

// what the text message carries (:99-109); df is a double expression stored to float, printed as a double
struct status_t { float cmaI, cmaQ; double df; float phase; int32_t reserved; };
KG_NR_HD status_t status_of(float cma_re, float cma_im, int exponent, int msk_mode, float df0, float phase0, float df_minus, float phase_minus,
                            float df_plus, float phase_plus)
{
    float df, phase;
    if (msk_mode) {
        df = (df_plus + df_minus) / (8 * M_PI);
        phase = KG_IQD_FMODF(0.25f * (phase_plus + phase_minus), (float) (2 * M_PI));
    } else {
        df = exponent ? df0 / (2 * M_PI * exponent) : 0;
        phase = phase0;
    }
    status_t s;
    s.cmaI = cma_re; s.cmaQ = cma_im; s.df = df; s.phase = phase; s.reserved = 0;
    return s;
}

// the class without its arrays.  pll[0]: _pll, pll[1]: _pllMinus, pll[2]: _pllPlus
struct state_t {
    int inited, run, rate_set;
    int points, nsamp, exponent, msk_mode, msk_baud, draw, display_mode;
    float gain, fs;
    int ring[NCH], maN;
    float cma_re, cma_im, ama;
    int maNsend;
    float pll_bandwidth;
    pll_t pll[3];
};

inline void pll_init_all(state_t &s)                                   // pll_init (:120-124)
{
    pll_init(s.pll[0], s.pll_bandwidth, 0.0, s.fs);
    pll_init(s.pll[1], s.pll_bandwidth, -0.5 * s.msk_baud, s.fs);
    pll_init(s.pll[2], s.pll_bandwidth, 0.5 * s.msk_baud, s.fs);
}

// `SET ext_server_init`: the constructor (:195-216)
inline void fresh(state_t &s)
{
    memset(&s, 0, sizeof s);
    s.inited = 1;
    s.points = 1024; s.exponent = 1; s.msk_baud = 200; s.fs = 12000.0f; s.pll_bandwidth = 10;
    pll_init_all(s);
}

// `SET run=%d` (:264-273); rate: what ext_update_get_sample_rateHz answers
inline int cmd_run(state_t &s, int run, double rate)
{
    if (run) {
        if (!(rate >= 1 && rate <= 1e9)) return REFUSED_RATE;
        s.fs = (float) rate;                                           // set_sample_rate (:114-118)
        s.maNsend = s.fs / 4;
        pll_init_all(s);
        s.rate_set = 1;
    }
    s.run = run != 0;
    return 0;
}
inline void cmd_gain(state_t &s, int gain) { s.gain = gain ? pow(10.0, ((float) gain - 50) / 10.0) : 0; }      // :127-129
inline int cmd_points(state_t &s, int points)
{
    if (points < 1 || points > RING) return REFUSED_POINTS;
    s.points = points;
    return 0;
}
inline int cmd_pll_mode(state_t &s, int pll_mode, int arg)             // :165-176
{
    if (pll_mode <= 1 && arg < 0) return REFUSED_EXPONENT;
    if (pll_mode <= 1) { s.exponent = arg; s.msk_mode = 0; }
    if (pll_mode == 2) { s.exponent = 2; s.msk_mode = 1; s.msk_baud = arg; }
    pll_init_all(s);
    return 0;
}
inline void cmd_pll_bandwidth(state_t &s, float bw) { s.pll_bandwidth = bw; pll_init_all(s); }
inline void cmd_draw(state_t &s, int draw) { s.draw = draw; }
inline void cmd_display_mode(state_t &s, int mode) { s.display_mode = mode; }
inline void cmd_clear(state_t &s)                                      // :184-192
{
    s.ama = 0; s.cma_re = s.cma_im = 0; s.maN = 0; s.nsamp = 0;
    pll_init_all(s);
}

inline int ma_cap(const state_t &s) { return (int) (0.5 * s.fs); }
KG_NR_HD int ma_count(int maN0, int i, int cap) { return maN0 >= cap ? maN0 : (maN0 + i < cap ? maN0 + i : cap); }      // maN ahead of sample i
inline int row_cmd(const state_t &s, int ch) { return (s.draw << 1) + (ch & 1); }
inline int row_len(const state_t &s) { return s.draw == POINTS ? s.points * NCH * 2 : s.points * 2; }

// The schedule of one display_data call of ns samples (:71-111): no sample enters it.  samp[0 .. rows): the sample behind which a
// row goes out; *sent: whether the text message does.  Advances ring, maN and nsamp.
inline int block_sched(state_t &s, int ch, int ns, int32_t *samp, int *sent)
{
    int rows = 0;
    if (s.draw == POINTS || s.draw == DENSITY) {
        const int first = s.points - s.ring[ch] > 1 ? s.points - s.ring[ch] : 1;      // samples up to the first row
        if (ns < first) s.ring[ch] += ns;
        else {
            for (int i = first - 1; i < ns; i += s.points) samp[rows++] = i;
            s.ring[ch] = (ns - first) % s.points;
        }
        s.maN = ma_count(s.maN, ns, ma_cap(s));
    }
    s.nsamp += ns;
    *sent = 0;
    if (s.nsamp > s.maNsend) { *sent = 1; s.nsamp -= s.maNsend; }
    return rows;
}

// process_sample (:43-69)
inline cf process_sample(state_t &s, cf sample)
{
    cf carrier; carrier.re = 1; carrier.im = 0;
    if (s.msk_mode) {
        const cf s2 = cmul(sample, sample);
        const float pm = pll_update(s.pll[1], s2);
        const float pp = pll_update(s.pll[2], s2);
        carrier = carrier_msk(pp, pm);
    } else if (s.exponent) {
        const float ph = pll_update(s.pll[0], cpow_u(sample, (unsigned) s.exponent));
        carrier = carrier_single(ph, s.exponent);
    }
    if (s.exponent) sample = s.display_mode == 0 ? cmul(sample, carrier) : carrier;
    s.cma_re = ma_step(s.cma_re, sample.re, s.maN);
    s.cma_im = ma_step(s.cma_im, sample.im, s.maN);
    s.ama = ma_step(s.ama, hypotf_dbl(sample.re, sample.im), s.maN);
    s.maN += s.maN < ma_cap(s);
    return sample;
}

// the whole object on the host, sample by sample as the reference walks it
struct full_t {
    state_t s;
    float iq[NCH][RING][2];
    unsigned char plot[NCH][RING][2][2];
    unsigned char map[RING][2];
};
typedef void (*emit_t)(void *user, int samp, int cmd, const unsigned char *bytes, int nbytes);

inline float scale_now(const state_t &s, int ch) { return s.gain ? scale_fixed(s.gain, ch) : scale_auto(s.ama); }

inline void display_data(full_t &q, int ch, int ns, const float *samps, emit_t emit, void *user, int *sent, status_t *st)
{
    state_t &s = q.s;
    const int cmd = row_cmd(s, ch);
    if (s.draw == POINTS || s.draw == DENSITY)
        for (int i = 0; i < ns; i++) {
            const int r = s.ring[ch];
            cf in; in.re = samps[2 * i]; in.im = samps[2 * i + 1];
            const cf v = process_sample(s, in);
            const float sc = scale_now(s, ch);
            if (s.draw == POINTS) {
                q.plot[ch][r][0][0] = u1(q.iq[ch][r][0], sc); q.plot[ch][r][0][1] = u1(q.iq[ch][r][1], sc);
                q.plot[ch][r][1][0] = u1(v.re, sc); q.plot[ch][r][1][1] = u1(v.im, sc);
                q.iq[ch][r][0] = v.re; q.iq[ch][r][1] = v.im;
            } else {
                q.map[r][0] = u1(v.re, sc); q.map[r][1] = u1(v.im, sc);
            }
            if (++s.ring[ch] >= s.points) {
                emit(user, i, cmd, s.draw == POINTS ? &q.plot[ch][0][0][0] : &q.map[0][0], row_len(s));
                s.ring[ch] = 0;
            }
        }
    s.nsamp += ns;
    *sent = 0;
    if (s.nsamp > s.maNsend) { *sent = 1; s.nsamp -= s.maNsend; }
    *st = status_of(s.cma_re, s.cma_im, s.exponent, s.msk_mode, s.pll[0].df, s.pll[0].phase, s.pll[1].df, s.pll[1].phase, s.pll[2].df, s.pll[2].phase);
}

}  // namespace kg_iqd_cf
#endif
