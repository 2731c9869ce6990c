// kg_nb.h -- the standard noise blanker (NB_STD) of CuteSDR's CNoiseProc (rx/CuteSDR/noiseproc.cpp), on the device AND the host,
// in the reference's own operand types: TYPEREAL is float, the literals (1e-6, MAGAVE_TIME = 0.005, .005) are double, so every
// expression below is written with the reference's operand types and in its order (the library and tools/ref/ref_nb_main.cpp are
// both built with -ffp-contract=off: no multiply-add is fused).  What lives here:
//   setup()      SetupBlanker's derivation (:89-145) plus this library's refusals (the reference is undefined there);
//   mag(), sum_step()  the per-sample arithmetic of ProcessBlanker (:147-203) that kg_nb.hip's kernels share with the host driver;
//   process(), one_shot()  a plain serial restatement of ProcessBlanker and ProcessBlankerOneShot (:259-267): the host driver's, and
//   the definition the kernels are split from (kg_nb.hip).
// The state is CNoiseProc's: a magnitude ring of M + 1 floats (m_Mptr wraps when it passes m_MagSamples), a delay ring of D + 1
// complex samples (m_Dptr likewise), the blank counter and the float running sum.
#ifndef KG_NB_H
#define KG_NB_H
#include <math.h>
#include <limits.h>

#if defined(__HIPCC__)
#define KG_NB_HD __host__ __device__ __forceinline__
#else
#define KG_NB_HD inline
#endif

namespace kg_nbk {

enum { MAX_GATE = 4096 };                 // noiseproc.cpp:48
enum { MAG_CAP = 1024 };                  // this library's cap on m_MagSamples (the reference's MAX_AVE, 32768, overruns its ring by one):
                                          // sample rates below 205000 (12000 -> 60, 20250 -> 101, 8192 -> 40)
enum { DLY_CAP = MAX_GATE / 2 };          // the largest m_DelaySamples
enum { MAG_RING = MAG_CAP + 1, DLY_RING = DLY_CAP + 1 };
enum { WF_NSAMPS = 8192 };                // WF_C_NSAMPS: the waterfall's frame and its "sample rate" (rx_waterfall.cpp:1090)
enum { GATE = 0, THRESHOLD = 1, NPARAMS = 8 };   // extensions/noise_blank/noise_blank.h, NOISE_PARAMS

struct st {                               // CNoiseProc's scalars (noiseproc.h)
    int mptr, dptr, cnt, M, D, G;         // m_Mptr, m_Dptr, m_BlankCounter, m_MagSamples, m_DelaySamples, m_GateSamples
    float ratio, sum;                     // m_Ratio, m_MagAveSum
};

enum { SETUP_OK = 0, SETUP_BAD_GATE = 1, SETUP_BAD_RATE = 2, SETUP_NEVER = 3 };

// SetupBlanker(id, SampleRate, nb_param) (:89-145) on `s` (whose M, D, G, ratio are a previous setup's, or `was_setup` is false):
// the derivation, then every pointer, counter and sum reset (the caller zeroes both rings).  Refused, with `s` unchanged:
//   SETUP_BAD_GATE  GateUsec * 1e-6 * SampleRate (double) NaN or outside int: its (int) conversion is undefined;
//   SETUP_BAD_RATE  SampleRate NaN or infinite, or 0.005 * SampleRate outside int or at or above MAG_CAP + 1 (the device ring);
//   SETUP_NEVER     SampleRate == 0 (only the reset) on a blanker that was never set up: M, D, G and the ratio are uninitialised.
inline int setup(st &s, bool was_setup, float SampleRate, const float *nb_param)
{
    float GateUsec = nb_param[GATE], Threshold = nb_param[THRESHOLD];
    st n = s;
    if (SampleRate != 0) {
        if (!(SampleRate == SampleRate) || isinf(SampleRate)) return SETUP_BAD_RATE;
        const double g = GateUsec * 1e-6 * SampleRate;
        if (!(g > (double) INT_MIN - 1.0 && g < (double) INT_MAX + 1.0)) return SETUP_BAD_GATE;
        const double m = 0.005 * SampleRate;                   // MAGAVE_TIME * SampleRate
        if (!(m > (double) INT_MIN - 1.0 && m < (double) MAG_CAP + 1.0)) return SETUP_BAD_RATE;
        n.G = (int) g;
        if (n.G < 3)
            n.G = 3;
        else if (n.G > MAX_GATE)
            n.G = MAX_GATE;
        n.M = (int) m;
        if (n.M < 1)
            n.M = 1;
        if (Threshold < 0)
            Threshold = 0;
        else if (Threshold > 100)
            Threshold = 100;
        n.ratio = .005 * (Threshold) * (float) n.M;
        n.D = n.G / 2;
        if (n.D < 1)
            n.D = 1;
    } else if (!was_setup) {
        return SETUP_NEVER;
    }
    n.dptr = 0;
    n.mptr = 0;
    n.cnt = 0;
    n.sum = 0.0;
    s = n;
    return SETUP_OK;
}

// peak magnitude: (mre > mim) ? mre : mim (:160-162; MFABS is fabsf)
KG_NB_HD float mag(float re, float im)
{
    const float mre = fabsf(re), mim = fabsf(im);
    return (mre > mim) ? mre : mim;
}

// the moving sum (:165-166): old = the ring entry the new magnitude replaces -- the only serial arithmetic of the stage
KG_NB_HD void sum_walk(float &sum, float old, float m)
{
    sum -= old;
    sum += m;
}

// the trigger test (:179) against the sum after that sample
KG_NB_HD bool trigger(float m, float ratio, float sum)
{
    return m * ratio > sum;
}

KG_NB_HD bool sum_step(float &sum, float old, float m, float ratio)
{
    sum_walk(sum, old, m);
    return trigger(m, ratio, sum);
}

// ProcessBlanker(n, in, out) (:147-203) on interleaved complex floats; in == out allowed (one sample is read before it is written)
inline void process(st &s, float *magbuf, float *dlybuf /* [2 (D + 1)] */, int n, const float *in, float *out)
{
    for (int i = 0; i < n; i++) {
        const float re = in[2 * i], im = in[2 * i + 1];
        const float m = mag(re, im);
        const bool trig = sum_step(s.sum, magbuf[s.mptr], m, s.ratio);
        magbuf[s.mptr++] = m;
        if (s.mptr > s.M) s.mptr = 0;
        const float ore = dlybuf[2 * s.dptr], oim = dlybuf[2 * s.dptr + 1];
        dlybuf[2 * s.dptr] = re; dlybuf[2 * s.dptr + 1] = im;
        s.dptr++;
        if (s.dptr > s.D) s.dptr = 0;
        if (trig) s.cnt = s.G;
        if (s.cnt) {
            s.cnt--;
            out[2 * i] = 0.0; out[2 * i + 1] = 0.0;
        } else {
            out[2 * i] = ore; out[2 * i + 1] = oim;
        }
    }
}

// ProcessBlankerOneShot(8192, in, out) (:259-267): D inputs into a scratch buffer, the remaining 8192 - D into out[0 ..), then D
// zeros into out's tail.  The delay is D + 1, so out[0] is the previous frame's last sample; the zero flush can trigger by itself.
inline void one_shot(st &s, float *magbuf, float *dlybuf, const float *in, float *out /* [2 * 8192], may be in */)
{
    static thread_local float ignore[2 * DLY_CAP], zero[2 * DLY_CAP];
    const int D = s.D, n = WF_NSAMPS;
    for (int i = 0; i < 2 * D; i++) zero[i] = 0.0f;
    process(s, magbuf, dlybuf, D, in, ignore);
    process(s, magbuf, dlybuf, n - D, in + 2 * D, out);
    process(s, magbuf, dlybuf, D, zero, out + 2 * (n - D));
}

}  // namespace kg_nbk

#endif
