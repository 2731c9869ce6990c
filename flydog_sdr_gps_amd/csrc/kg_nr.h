// kg_nr.h -- the two LMS noise processors of c2s_sound()'s noise-reduction switch (rx/rx_sound.cpp:933-949), on the device AND the
// host, in the reference's own operand types:
//   NR_WDSP  wdsp_ANR_init / wdsp_ANR_filter (rx/wdsp/ANR.cpp:43-116): the variable-leak LMS, one wdsp_ANR_t per channel and type;
//   NR_ORIG  CLMS::Initialize / ProcessFilter (rx/kiwi/lms.cpp:21-123): the 121-tap LMS over one ring of m_dlen + 121 floats.
// TYPEREAL is float there and K_AMPMAX (32767.0) and the other literals are double, so every expression below is written with the
// reference's operand types and in its order: C++ then promotes exactly as the reference's compiler does (the library and
// tools/ref/ref_nr_main.cpp are both built with -ffp-contract=off, so no multiply-add is fused).  What lives here is the per-sample
// scalar arithmetic that kg_post.hip's kernel and tests/test_nr_cpu.py's host driver share as one text, plus the host-side
// inits and a plain serial restatement of both filters (the host driver's, and the definition the kernel is split from).
#ifndef KG_NR_H
#define KG_NR_H
#include <math.h>
#include <string.h>

#if defined(__HIPCC__)
#define KG_NR_HD __host__ __device__ __forceinline__
#else
#define KG_NR_HD inline
#endif

namespace kg_nr {

enum { ANR_DLINE = 512, ANR_MASK = ANR_DLINE - 1 };       // ANR.cpp:19-20
enum { LMSLEN = 121, LMS_RING = 512 };                    // lms.h:7-9: MAX_DLEN + LMSLEN
enum { DENOISE = 0, AUTONOTCH = 1 };                      // nr_type_e, rx/rx_noise.h:10
enum { NPARAMS = 8 };                                     // NOISE_PARAMS, rx/rx_noise.h:4

struct anr_t {                    // wdsp_ANR_t's scalars (ANR.cpp:22-38); d[] and w[] live beside it
    int in_idx, taps, delay, position;
    float two_mu, gamma, lidx, lidx_min, lidx_max, ngamma, den_mult, lincr, ldecr;
};
struct lms_t {                    // CLMS's scalars (lms.h:21-29); m_dline[] and m_lmscoef[] live beside it
    int nr_type, dlen, dlp;
    float beta, decay;
};

// (TYPEMONO16) v: truncation; outside the int range (undefined in C) the low 16 bits of x86's 0x80000000
KG_NR_HD short mono16(float v)
{
    int w;
    if (!(v > -2147483648.0f && v < 2147483648.0f)) w = (int) 0x80000000u;
    else w = (int) v;
    return (short) (unsigned short) (unsigned) w;
}

// ((TYPEREAL) in[i]) / K_AMPMAX (ANR.cpp:72, lms.cpp:90): a double division, rounded to float on assignment
KG_NR_HD float sample_in(short x)
{
    const float v = ((float) x) / 32767.0;
    return v;
}

// (TYPEMONO16) MROUND(v * K_AMPMAX): the double product rounded to float for roundf (ANR.cpp:88, lms.cpp:104 / :110)
KG_NR_HD short sample_out(float v)
{
    return mono16(roundf((float) (v * 32767.0)));
}

// ---- wdsp_ANR_filter's per-sample scalars (ANR.cpp:83-107) ----
// inv_sigp = 1.0 / (sigma + 1e-10): double, rounded on assignment
KG_NR_HD float anr_inv_sigp(float sigma)
{
    const float inv_sigp = 1.0 / (sigma + 1e-10);
    return inv_sigp;
}

// Everything after the two sums of sample i: the output, nel / nev, the lidx update (the reference's dangling else, as written),
// ngamma, and the weight update's factors c0 and c1.  dcur = d[in_idx], y and sigma the serial sums, inv_sigp = anr_inv_sigp(sigma).
KG_NR_HD short anr_step(anr_t &w, int nr_type, float dcur, float y, float sigma, float inv_sigp, float &c0, float &c1)
{
    float error, nel, nev, out_f;
    error = dcur - y;
    if (nr_type == AUTONOTCH)
        out_f = error;
    else
        out_f = y * 4.0;
    const short out = sample_out(out_f);
    if ((nel = error * (1.0 - w.two_mu * sigma * inv_sigp)) < 0.0) nel = -nel;
    if ((nev = dcur - (1.0 - w.two_mu * w.ngamma) * y - w.two_mu * error * sigma * inv_sigp) < 0.0)
        nev = -nev;
    if (nev < nel) {
        if ((w.lidx += w.lincr) > w.lidx_max) w.lidx = w.lidx_max;
        else
        if ((w.lidx -= w.ldecr) < w.lidx_min) w.lidx = w.lidx_min;
    }
    w.ngamma = w.gamma * (w.lidx * w.lidx) * (w.lidx * w.lidx) * w.den_mult;
    c0 = 1.0 - w.two_mu * w.ngamma;
    c1 = w.two_mu * error * inv_sigp;
    return out;
}

// w[j] = c0 * w[j] + c1 * d[idx] (ANR.cpp:109-112): two float products and a float add
KG_NR_HD float anr_weight(float wj, float dj, float c0, float c1) { return c0 * wj + c1 * dj; }

// ---- CLMS::ProcessFilter's per-sample scalars (lms.cpp:100-116) ----
// the denoiser's output, formed from fir before err: fir * 2 (float x int) * K_AMPMAX (double)
KG_NR_HD short lms_out_denoise(float fir) { return mono16(roundf((float) (fir * 2 * 32767.0))); }
KG_NR_HD float lms_err(float samp, float fir) { return samp - fir; }
KG_NR_HD float lms_err2(float err, float beta) { return err * beta; }
// m_lmscoef[i] = m_dline[m_dlp] * err2 + m_lmscoef[i] * m_decay
KG_NR_HD float lms_coef(float dline, float err2, float coef, float decay) { return dline * err2 + coef * decay; }

// ---- host: the inits and the argument checks ----
// wdsp_ANR_init (ANR.cpp:43-62): memset, then the params; (int) truncates taps and delay
inline void anr_init(anr_t &w, float *d, float *wt, const float nr_param[NPARAMS])
{
    memset(&w, 0, sizeof w);
    memset(d, 0, sizeof(float) * ANR_DLINE);
    memset(wt, 0, sizeof(float) * ANR_DLINE);
    w.taps = (int) nr_param[0];           // NR_TAPS
    w.delay = (int) nr_param[1];          // NR_DLY
    w.position = 0;
    w.two_mu = nr_param[2];               // NR_GAIN
    w.gamma = nr_param[3];                // NR_LEAKAGE
    w.lidx = 120.0;
    w.lidx_min = 120.0;
    w.lidx_max = 200.0;
    w.ngamma = 0.001;
    w.den_mult = 6.25e-10;
    w.lincr = 1.0;
    w.ldecr = 3.0;
}

// CLMS::Initialize (lms.cpp:21-50) for nr_type DENOISE or AUTONOTCH: per-type defaults for values <= 0, the delay line cut at 300
inline void lms_init(lms_t &m, float *dline, float *coef, int nr_type, const float nr_param[NPARAMS])
{
    float delayLineLen = nr_param[0], beta = nr_param[1], decay = nr_param[2];       // NR_DELAY, NR_BETA, NR_DECAY
    m.nr_type = nr_type;
    if (m.nr_type == AUTONOTCH) {
        if (delayLineLen <= 0) delayLineLen = 48;
        if (beta <= 0) beta = 0.125;
        m.beta = beta;
        if (decay <= 0) decay = 0.99915;
        m.decay = decay;
    } else {
        if (delayLineLen <= 0) delayLineLen = 1;
        if (beta <= 0) beta = 0.0058;
        m.beta = beta;
        if (decay <= 0) decay = 0.98;
        m.decay = decay;
    }
    if (delayLineLen > 300) delayLineLen = 300;
    m.dlen = delayLineLen;
    m.dlp = 0;
    memset(dline, 0, sizeof(float) * LMS_RING);
    memset(coef, 0, sizeof(float) * LMSLEN);
}

inline bool int_convertible(float v) { return v > -2147483649.0 && v < 2147483648.0; }    // (int) v defined (NaN: false)

// The parameter vectors on which an init is defined.  wdsp_ANR_init converts taps and delay with (int) (undefined for NaN, Inf and
// values outside int); taps > 512 overruns w[]; a delay above INT_MAX - 1022 overflows in_idx + j + delay (ANR.cpp:79).
// CLMS::Initialize converts the clamped delay-line length: only NaN gets through its comparisons to the conversion.
inline bool anr_params_ok(const float p[NPARAMS])
{
    if (!int_convertible(p[0]) || !int_convertible(p[1])) return false;
    return (int) p[0] <= ANR_DLINE && (int) p[1] <= 2147483647 - 1022;
}
inline bool lms_params_ok(const float p[NPARAMS]) { return p[0] == p[0]; }

// ---- host: both filters, serially, as the reference walks them (the CPU test's driver; the kernel's definition) ----
inline void anr_filter(anr_t &w, float *d, float *wt, int nr_type, int ns_out, const short *in, short *out)
{
    for (int i = 0; i < ns_out; i++) {
        d[w.in_idx] = sample_in(in[i]);
        float y = 0, sigma = 0;
        for (int j = 0; j < w.taps; j++) {
            const int idx = (int) ((unsigned) (w.in_idx + j) + (unsigned) w.delay) & ANR_MASK;
            y += wt[j] * d[idx];
            sigma += d[idx] * d[idx];
        }
        const float isp = anr_inv_sigp(sigma);
        float c0, c1;
        out[i] = anr_step(w, nr_type, d[w.in_idx], y, sigma, isp, c0, c1);
        for (int j = 0; j < w.taps; j++) {
            const int idx = (int) ((unsigned) (w.in_idx + j) + (unsigned) w.delay) & ANR_MASK;
            wt[j] = anr_weight(wt[j], d[idx], c0, c1);
        }
        w.in_idx = (w.in_idx + ANR_MASK) & ANR_MASK;
    }
}

inline void lms_filter(lms_t &m, float *dline, float *coef, int ilen, const short *ibuf, short *obuf)
{
    const int L1 = m.dlen + LMSLEN - 1;                   // INC / DEC wrap at m_dlen + LMSLEN_M1 (lms.h:11-12)
    for (int bp = 0; bp < ilen; bp++) {
        const float samp = sample_in(ibuf[bp]);
        dline[m.dlp] = samp; m.dlp = m.dlp == L1 ? 0 : m.dlp + 1;
        float fir = 0;
        for (int i = 0; i < LMSLEN; i++) {
            fir += dline[m.dlp] * coef[i];
            m.dlp = m.dlp == L1 ? 0 : m.dlp + 1;
        }
        m.dlp = m.dlp == 0 ? L1 : m.dlp - 1;
        if (m.nr_type == DENOISE) obuf[bp] = lms_out_denoise(fir);
        const float err = lms_err(samp, fir);
        if (m.nr_type == AUTONOTCH) obuf[bp] = sample_out(err);
        const float err2 = lms_err2(err, m.beta);
        for (int i = LMSLEN - 1; i >= 0; i--) {
            coef[i] = lms_coef(dline[m.dlp], err2, coef[i], m.decay);
            m.dlp = m.dlp == 0 ? L1 : m.dlp - 1;
        }
        m.dlp = m.dlp == L1 ? 0 : m.dlp + 1;
    }
}

}  // namespace kg_nr
#endif
