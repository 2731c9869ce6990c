// kg_post.hip -- S-meter, CAgc, the AM / NBFM detectors and what follows them up to out_samps_s2 (m_AM_FIR, the NBFM noise
// squelch, the de-emphasis filters) for many receiver channels.
//
// Reference: rx/rx_sound.cpp:676-696 (S-meter), rx/CuteSDR/agc.cpp (CAgc),
// rx/rx_sound.cpp:766-787 (AM + m_AM_FIR), :845-877 (NBFM + m_Squelch), :898-907 (de-emphasis); rx/CuteSDR/fir.cpp (CFir),
// rx/CuteSDR/squelch.cpp (CSquelch).  TYPEREAL is float there and the
// literals are double, so the expressions below keep the reference's operand types
// (the library is built with -ffp-contract=off), and log10f (which CAgc BRANCHES on) and powf are the
// host libm's algorithms restated on the device (kg_libm.h: bit-identical on every argument, round 6):
// nothing in this file computes differently from the reference built on this image.
//
// One wavefront per channel.  What the reference does with circular buffers is
// restated so that most of it runs in parallel over the samples of the call:
//   * the signal delay line is a pure delay of m_DelaySamples (agc.cpp:175-180);
//   * m_Peak is exactly the maximum of the last m_WindowSamples magnitudes: the
//     reference keeps the running maximum and rescans the window when the value that
//     leaves equals it (agc.cpp:193-210), and every real magnitude is >= -8, the floor of
//     the rescan; the window maximum is computed by log2(W) doubling passes in LDS;
//   * the two averagers with their data-dependent branches, the hang timer, the S-meter
//     recurrence and the AM DC-removal IIR are sequential: lane 0 walks the samples;
//   * gain (powf), scaling, the mono16 cast and the NBFM detector are parallel again;
//   * CFir::ProcessFilter keeps its samples in a circular buffer and sums coefficient x sample over the BUFFER positions 0 ..
//     N-1 (fir.cpp:79-91), so the order of the float additions rotates with the write position: sample number g (since the
//     filter was initialised) starts its sum at the tap of age g mod N, runs up to age N-1 and wraps to age 0.  Restated per
//     output sample, that is a sum every lane can do for its own sample -- in that order, over a linear history in LDS;
//   * the squelch's noise average is one more sequential recursion (lane 0); its verdict applies to the whole block;
//   * the synchronous-AM family (rx/rx_sound.cpp:791-806, rx/wdsp/SAM_demod.cpp) is split by dependence, not by sample: lane 0
//     walks only the PLL (sinf / cosf of the phase error, the correlator, atan2f, omega2, fil_out, phzerror; the libm functions are
//     kg_libm_trig.h's restatements) and leaves sin / cos per sample in LDS; the four Hilbert all-pass chains a, b, c, d, which do not feed
//     the PLL, run on lanes 0..3 at once; the per-mode audio formulas run across all lanes; the fade leveler / DC block recursions of
//     audio, audiou, audion on lanes 0..2; the mono16 cast and the stores across all lanes.  No recurrence is reassociated.
//     The SAM state is a parallel table (post_sam) and the stage lives in its own instance of the kernel (post_kernel<true>,
//     launched only for a batch that holds a SAM-family channel), so the other modes' kernel is the one it was.
//   * the noise-reduction switch (rx/rx_sound.cpp:933-949: wdsp's variable-leak LMS, rx/wdsp/ANR.cpp, and the original 121-tap LMS,
//     rx/kiwi/lms.cpp) is split by dependence too.  What depends only on the stage's input -- the d values, wdsp's sigma of every
//     sample (a serial sum of its own) and its double division -- runs per sample across the lanes ahead of the recursion; the tap
//     products and the weight / coefficient updates run across the lanes (one tap per lane and pass); the ordered sums y / fir and
//     the scalar recurrences (kg_nr.h, shared with the host driver of tests/test_nr_cpu.py) are walked by every lane at once over the
//     products in LDS, so no lane waits for a broadcast.  Nothing is reassociated.  The stage is a kernel of its own (post_nr_kernel)
//     that kg_post_process_dev enqueues behind post_kernel only for a batch that holds a channel with NR on, over that launch's
//     d_s16 rows in place.
//   * NR_SPECTRAL (rx/Teensy/NR_spectral.cpp), the third algorithm of that switch, is transform work: per 512 samples two
//     50 %-overlapped 512-point frames, each a forward transform, per-bin gains and an inverse transform.  One wave per channel
//     (post_nrs_kernel), the channel's nine 256-float arrays and the frame in LDS for the whole call.  Each of the three radix-8 passes
//     of the reference's transform is 64 independent butterflies, one per lane, through LDS; the digit reversal is the last pass's
//     store address, the inverse's conjugate and scale a sign at the first load and a factor at the last store.  The per-bin
//     expressions (kg_nrs.h, shared with the host driver) run four bins per lane; the two ordered sums pre_power / post_power are
//     walked by every lane over LDS; each smoothed gain is its own ordered sum of <= 9 terms.  Nothing is reassociated.
//   * NB_WILD (rx/Teensy/NB_Wild.cpp), the noise blanker of the post-filter chain (rx_sound.cpp:922-931, ahead of the NR switch), is
//     a kernel of its own too (post_nbw_kernel), enqueued between post_kernel and the NR kernels only for a batch that holds a
//     channel with the stage on.  One wave per channel; its split between lanes and serial walks is at the kernel.
#include "kg_common.h"
#include "kg_libm.h"
#include "kg_libm_trig.h"
#include "kg_nr.h"
#include "kg_nrs.h"
#include "kg_nbw.h"
#include "kg_tables.h"

#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>

#define POST_CIRC 4096            // per-channel history ring: >= KG_POST_MAX_SAMPLES + 2047
#define POST_MAXW 2047            // MAX_DELAY_BUF - 1 (agc.h:16, agc.cpp:159-160)
#define AGC_OUTSCALE 0.7          // agc.cpp:64
#define MAX_AMPLITUDE 32767.0     // agc.cpp:66

struct post_chan {
    // CAgc parameters (agc.cpp:134-160)
    int agc_on, use_hang, delay_samples, window_samples, hang_time;
    float manual_agc_gain, knee, gain_slope, fixed_gain;
    float attack_rise_alpha, attack_fall_alpha, decay_rise_alpha, decay_fall_alpha;
    // CAgc state
    float decay_ave, attack_ave;
    int hang_timer;
    unsigned count;               // samples written to the rings so far (mod 2^32)
    // S-meter (rx_sound.cpp:249-250)
    float smeter_alpha, smeter_avg, smeter_tap0, smeter_tap1;
    // detectors
    double z1;                    // rx_sound.cpp:244
    float last_re, last_im;       // conn->last_sample
    int mode;
    // CSquelch (squelch.cpp:106-107, 122-129) and its state (:67-77)
    float sq_alpha, sq_value, sq_threshold, sq_ave;
    int sq_state, sq_set;         // m_SquelchState, m_SetSquelch
    int sq_rc, squelched;         // the last nsq_nc_sq; s->squelched (rx_sound.cpp:877)
    int deemp, deemp_nfm;         // s->deemp, s->deemp_nfm (rx_sound_cmd.cpp:554)
};

// wdsp_SAM_t (SAM_demod.cpp:36-66) of a channel, the globals wdsp_SAM_demod_init() derives from snd_rate (:69-80, :154-163),
// and s->SAM_mparam / s->isChanNull (rx_sound_cmd.cpp:216, rx_sound.cpp:802)
#define SAM_STAGES 7              // SAM_PLL_HILBERT_STAGES
#define SAM_ABCD (3 * SAM_STAGES + 3)
struct post_sam {
    double z1, z1_u, z1_n;        // DC block
    float phzerror, fil_out, omega2, sam_carrier, sam_lowpass, zeta, omegaN, g1, g2;
    float dc, dc_insert, dcu, dc_insertu;                 // fade leveler
    float abcd[4][SAM_ABCD];      // Hilbert filter variables a, b, c, d
    float dsI, dsQ;
    int type;
    // not reset by PLL_RESET
    int is_chan_null, snd_rate, mparam;
    float omega_min, omega_max, mtauR, onem_mtauR, mtauI, onem_mtauI;
};

#define POST_MAXTAPS 97           // MAX_NUMCOEF, fir.h:20
#define POST_HIST (POST_MAXTAPS - 1)
enum { POST_FIR_AM = 0, POST_FIR_SQ_HP = 1, POST_FIR_DEEMP_NFM = 2, POST_FIR_DEEMP_AM_SSB = 3, POST_NFIR = 4 };

struct post_cfir {                // one CFir, real-valued (fir.h:24-52)
    int ntaps, pos;               // m_NumTaps; samples since the filter was initialised, mod ntaps (m_State = (ntaps - pos) % ntaps)
    float taps[POST_MAXTAPS];
    float hist[POST_HIST];        // the last 96 inputs, newest last (m_rZBuf unrolled)
};

// (TYPEMONO16) v
__device__ __forceinline__ short post_mono16(float v)
{
    int w;
    if (!(v > -2147483648.0f && v < 2147483648.0f)) w = (int) 0x80000000u;
    else w = (int) v;
    return (short) (unsigned short) (unsigned) w;
}

// CFir::ProcessFilter for the n samples at src (fir.cpp:74-92 real -> real; :176-194 / :199-217 -> mono16 when `mono`).
// X: LDS, POST_HIST + n floats; T: LDS, POST_MAXTAPS floats; src, dst: LDS, dst may be src, neither may overlap X or T.
__device__ __forceinline__ void post_cfir_block(post_cfir *__restrict__ f, float *X, float *T, const float *src, float *dst, int n,
                                                int lane, bool mono)
{
    const int N = f->ntaps, pos = f->pos;
    for (int k = lane; k < POST_HIST; k += 64) X[k] = f->hist[k];
    for (int k = lane; k < N; k += 64) T[k] = f->taps[k];
    for (int j = lane; j < n; j += 64) X[POST_HIST + j] = src[j];
    __syncthreads();
    for (int j = lane; j < n; j += 64) {
        const float *x = X + POST_HIST + j;
        int a = (pos + j) % N;                                  // the age at buffer position 0
        float acc = T[a] * x[-a];                               // "do the 1st MAC"
        for (int t = 1; t < N; t++) {
            a = a + 1 == N ? 0 : a + 1;
            acc += T[a] * x[-a];
        }
        dst[j] = mono ? (float) post_mono16(acc) : acc;
    }
    __syncthreads();
    for (int k = lane; k < POST_HIST; k += 64) f->hist[k] = X[n + k];
    if (lane == 0) f->pos = (pos + n) % N;
    __syncthreads();
}

// CSquelch::PerformFMSquelch (squelch.cpp:151-231) for the n detector samples at demod (LDS; demod + KG_POST_MAX_SAMPLES .. + n is
// scratch): the mono16 output as floats at out (LDS), state and return value into *pc.  X, T as post_cfir_block.
__device__ __forceinline__ void post_squelch_block(post_chan *__restrict__ pc, const post_chan &c, post_cfir *__restrict__ hp, float *X,
                                                   float *T, float *demod, float *out, int n, int lane, int *s_sq)
{
    float *sqbuf = demod + KG_POST_MAX_SAMPLES;
    post_cfir_block(hp, X, T, demod, sqbuf, n, lane, false);                                     // :161
    if (lane == 0) {
        float ave = c.sq_ave;
        const double om = 1.0 - c.sq_alpha;
        for (int i = 0; i < n; i++) {
            const float mag = fabsf(sqbuf[i]);
            ave = om * ave + c.sq_alpha * mag;                                                   // :166
        }
        int state = c.sq_state, rc = 0;
        if (c.sq_value == 0) {                                                                   // :176-179
            if (state) rc = -1;
            state = 0;
        } else if (c.sq_threshold == 0) {                                                        // :182-185
            if (!state) rc = 1;
            state = 1;
        } else if (state) {                                                                      // :188-193
            if (ave < (c.sq_threshold - 50.0)) { rc = -1; state = 0; }
        } else {                                                                                 // :195-200
            if (ave >= (c.sq_threshold + 50.0)) { rc = 1; state = 1; }
        }
        if (c.sq_set) rc = state ? 1 : -1;                                                       // :218-221
        pc->sq_ave = ave; pc->sq_state = state; pc->sq_set = 0; pc->sq_rc = rc;
        if (rc != 0) pc->squelched = rc == 1;                                                    // rx_sound.cpp:877
        *s_sq = state;
    }
    __syncthreads();
    const int squelched = *s_sq;
    for (int j = lane; j < n; j += 64) out[j] = squelched ? 1.0f : (float) post_mono16(demod[j]);   // :205-207, :214-215
    __syncthreads();
}

// ---- the synchronous-AM family (rx/rx_sound.cpp:791-806 -> wdsp_SAM_demod, rx/wdsp/SAM_demod.cpp:210-346) ----
// SAM_demod.cpp:85-103: the double literals as the reference's f32_t arrays hold them
__device__ __constant__ const float sam_c0[SAM_STAGES] = {(float) -0.328201924180698, (float) -0.744171491539427, (float) -0.923022915444215,
                                                          (float) -0.978490468768238, (float) -0.994128272402075, (float) -0.998458978159551,
                                                          (float) -0.999790306259206};
__device__ __constant__ const float sam_c1[SAM_STAGES] = {(float) -0.0991227952747244, (float) -0.565619728761389, (float) -0.857467122550052,
                                                          (float) -0.959123933111275, (float) -0.988739372718090, (float) -0.996959189310611,
                                                          (float) -0.999282492800792};

// wdsp_SAM_demod(rx_chan, mode, SAM_mparam, n, agc_samps_c, out_samps_s2) over the AGC output in s_agc (LDS).  Mono modes: out_samps_s2
// as mono16-valued floats into aud (LDS); stereo (SAS, QAM) and channel-null SAM: the pair written back into agc_samps_c, here pagc
// (global, the row the gain loop wrote).  es, ec, cI, audu, audn: LDS scratch of n floats each; ps: 4 x KG_POST_MAX_SAMPLES floats.
__device__ __forceinline__ void post_sam_block(post_sam *__restrict__ ws, int mode, const float2 *s_agc, float *es, float *ec, float *cI,
                                               float *ps, float *aud, float *audu, float *audn, float2 *pagc, int n, int lane)
{
    const double K_2PI = 2.0 * 3.14159265358979323846;                 // datatypes.h:103
    const int mparam = ws->mparam, which = mparam & 3;                  // CHAN_NULL_WHICH (wdsp.h:5-10)
    const bool is_null = mode == KG_POST_SAM && which != 0;
    const bool need_ps = (mode != KG_POST_SAM && mode != KG_POST_QAM) || is_null;
    const bool stereo_or_null = mode == KG_POST_SAS || mode == KG_POST_QAM || is_null;
    const bool fade = (mparam & 4) != 0, dcb = (mparam & 8) != 0;     // FADE_LEVELER, DC_BLOCK

    // 1. the PLL: one dependent chain per sample (:218-223, :331-342), lane 0; sin / cos of the phase error stay for the others
    if (lane == 0) {
        float phz = ws->phzerror, fil = ws->fil_out, om2 = ws->omega2;
        const float g1 = ws->g1, g2 = ws->g2, omin = ws->omega_min, omax = ws->omega_max;
        for (int j = 0; j < n; j++) {
            const float sn = kg_libm::sinf_glibc(phz), cs = kg_libm::cosf_glibc(phz);
            es[j] = sn; ec[j] = cs;
            const float2 x = s_agc[j];
            const float ai = cs * x.x, bi = sn * x.x, aq = cs * x.y, bq = sn * x.y;
            const float corrI = +ai + bq, corrQ = -bi + aq;
            const float det = kg_libm::atan2f_glibc(corrQ, corrI);
            const float del_out = fil;
            om2 = om2 + g2 * det;
            om2 = om2 < omin ? omin : (om2 > omax ? omax : om2);          // CLAMP (types.h:115)
            fil = g1 * det + om2;
            phz = phz + del_out;
            // wrap round 2 pi in double (:341-342); one pass suffices for any finite phase the loop can reach, the bound keeps an
            // infinite one (which the reference would loop on forever) from hanging the wave
            for (int it = 0; phz >= K_2PI && it < 64; it++) phz = phz - K_2PI;
            for (int it = 0; phz < 0.0 && it < 64; it++) phz = phz + K_2PI;
        }
        ws->phzerror = phz; ws->fil_out = fil; ws->omega2 = om2;
        float car = 0.08 * (om2 * (float) ws->snd_rate) / K_2PI;         // :346-348
        car = car + 0.92 * ws->sam_lowpass;
        ws->sam_carrier = car; ws->sam_lowpass = car;
        ws->is_chan_null = is_null;                                      // the return value, s->isChanNull (rx_sound.cpp:802)
    }
    __syncthreads();

    // 2. the four Hilbert all-pass chains (:225-256): independent recurrences, lanes 0..3 = a (dsI: ai one sample late), b (bi),
    //    c (dsQ: bq one sample late), d (aq); each keeps its 24-entry shift register in registers
    if (need_ps && lane < 4) {
        float r[SAM_ABCD];
#pragma unroll
        for (int k = 0; k < SAM_ABCD; k++) r[k] = ws->abcd[lane][k];
        float cc[SAM_STAGES];
#pragma unroll
        for (int k = 0; k < SAM_STAGES; k++) cc[k] = (lane & 1) ? sam_c1[k] : sam_c0[k];
        const bool delayed = lane == 0 || lane == 2;
        float ds = lane == 0 ? ws->dsI : ws->dsQ;
        const float *e = (lane == 0 || lane == 3) ? ec : es;
        for (int j = 0; j < n; j++) {
            const float2 x = s_agc[j];
            const float v = e[j] * (lane < 2 ? x.x : x.y);
            r[0] = delayed ? ds : v;
            ds = v;
#pragma unroll
            for (int k = 0; k < 3 * SAM_STAGES; k += 3) r[k + 3] = cc[k / 3] * (r[k] - r[k + 5]) + r[k + 2];
            ps[lane * KG_POST_MAX_SAMPLES + j] = r[3 * SAM_STAGES];
#pragma unroll
            for (int k = SAM_ABCD - 1; k > 0; k--) r[k] = r[k - 1];
        }
#pragma unroll
        for (int k = 0; k < SAM_ABCD; k++) ws->abcd[lane][k] = r[k];
        if (lane == 0) ws->dsI = ds;
        if (lane == 2) ws->dsQ = ds;
    }
    __syncthreads();

    // 3. the mode's audio (:258-300), every sample on its own
    for (int j = lane; j < n; j += 64) {
        const float2 x = s_agc[j];
        const float sn = es[j], cs = ec[j];
        const float ai = cs * x.x, bi = sn * x.x, aq = cs * x.y, bq = sn * x.y;
        const float corrI = +ai + bq, corrQ = -bi + aq;
        float ai_ps = 0, bi_ps = 0, bq_ps = 0, aq_ps = 0;
        if (need_ps) {
            ai_ps = ps[j]; bi_ps = ps[KG_POST_MAX_SAMPLES + j];
            bq_ps = ps[2 * KG_POST_MAX_SAMPLES + j]; aq_ps = ps[3 * KG_POST_MAX_SAMPLES + j];
        }
        const float lsb = (ai_ps + bi_ps) - (aq_ps - bq_ps), usb = (ai_ps - bi_ps) + (aq_ps + bq_ps);
        float audio = 0, audiou = 0, audion = 0;
        if (mode == KG_POST_SAM) {
            if (is_null) { audio = lsb; audiou = usb; audion = which == 1 ? audio - audiou : audiou - audio; }
            else audio = corrI;
        } else if (mode == KG_POST_SAU) audio = usb;
        else if (mode == KG_POST_SAL) audio = lsb;
        else if (mode == KG_POST_SAS) { audio = lsb; audiou = usb; }
        else {                                                          // C-QUAM
            audio = corrI / 2 + corrQ / 2; audio *= 2;
            audiou = corrI / 2 - corrQ / 2; audiou *= 2;
        }
        aud[j] = audio; audu[j] = audiou; audn[j] = audion; cI[j] = corrI;
    }
    __syncthreads();

    // 4. fade leveler + DC block (:305-329): three independent recursions, lanes 0..2
    const bool walk = lane == 0 ? (fade || dcb) : lane == 1 ? stereo_or_null && (fade || dcb) : lane == 2 ? is_null && dcb : false;
    if (walk) {
        float *a = lane == 0 ? aud : lane == 1 ? audu : audn;
        double z1 = lane == 0 ? ws->z1 : lane == 1 ? ws->z1_u : ws->z1_n;
        float dc = lane == 0 ? ws->dc : ws->dcu, dci = lane == 0 ? ws->dc_insert : ws->dc_insertu;
        const bool lev = fade && lane < 2;
        const float mR = ws->mtauR, omR = ws->onem_mtauR, mI = ws->mtauI, omI = ws->onem_mtauI;
        for (int j = 0; j < n; j++) {
            float audio = a[j];
            if (lev) {
                dc = mR * dc + omR * audio;
                dci = mI * dci + omI * cI[j];
                audio = audio + dci - dc;
            }
            if (dcb) {
                const float z0 = audio + (z1 * 0.99f);                  // DC_ALPHA
                audio = z0 - z1;
                z1 = z0;
            }
            a[j] = audio;
        }
        if (lane == 0) { ws->z1 = z1; ws->dc = dc; ws->dc_insert = dci; }
        else if (lane == 1) { ws->z1_u = z1; ws->dcu = dc; ws->dc_insertu = dci; }
        else ws->z1_n = z1;
    }
    __syncthreads();

    // 5. outputs (:307-329): out[i] (TYPEMONO16), the stereo / nulled pair back into agc_samps_c
    for (int j = lane; j < n; j += 64) {
        if (!stereo_or_null) {
            aud[j] = (float) post_mono16(aud[j]);
        } else if (is_null) {
            const float an = audn[j];
            aud[j] = (float) post_mono16(an);
            if (pagc) pagc[j] = which == 1 ? make_float2(an, 0.f) : make_float2(0.f, an);
        } else if (pagc) {
            pagc[j] = make_float2(aud[j], audu[j]);
        }
    }
    __syncthreads();
}

// The two seams called on their own: m_*_FIR[ch].ProcessFilter(n, in, out) (kind 0: real -> real, 1: real -> mono16, 2: mono16 ->
// mono16) and m_Squelch[ch].PerformFMSquelch(n, in, out) -- the same device functions as the fused pass below.
__global__ __launch_bounds__(64) void post_cfir_kernel(post_cfir *__restrict__ cfir_tab, const int *__restrict__ chans, int slot, int kind,
                                                       const void *__restrict__ in, size_t in_stride, int n, void *__restrict__ out,
                                                       size_t out_stride)
{
    __shared__ float X[POST_HIST + KG_POST_MAX_SAMPLES];
    __shared__ float buf[KG_POST_MAX_SAMPLES];
    __shared__ float T[POST_MAXTAPS];
    const int lane = threadIdx.x, row = blockIdx.x, ch = chans[row];
    for (int j = lane; j < n; j += 64)
        buf[j] = kind == 2 ? (float) ((const short *) in)[(size_t) row * in_stride + j] : ((const float *) in)[(size_t) row * in_stride + j];
    __syncthreads();
    post_cfir_block(cfir_tab + (size_t) ch * POST_NFIR + slot, X, T, buf, buf, n, lane, kind != 0);
    for (int j = lane; j < n; j += 64) {
        if (kind == 0) ((float *) out)[(size_t) row * out_stride + j] = buf[j];
        else ((short *) out)[(size_t) row * out_stride + j] = (short) buf[j];
    }
}

__global__ __launch_bounds__(64) void post_squelch_kernel(post_chan *__restrict__ chan_tab, post_cfir *__restrict__ cfir_tab,
                                                          const int *__restrict__ chans, const float *__restrict__ in, size_t in_stride, int n,
                                                          short *__restrict__ out, size_t out_stride)
{
    __shared__ float X[POST_HIST + KG_POST_MAX_SAMPLES];
    __shared__ float demod[2 * KG_POST_MAX_SAMPLES];
    __shared__ float res[KG_POST_MAX_SAMPLES];
    __shared__ float T[POST_MAXTAPS];
    __shared__ int s_sq;
    const int lane = threadIdx.x, row = blockIdx.x, ch = chans[row];
    post_chan *pc = &chan_tab[ch];
    const post_chan c = *pc;
    for (int j = lane; j < n; j += 64) demod[j] = in[(size_t) row * in_stride + j];
    __syncthreads();
    post_squelch_block(pc, c, cfir_tab + (size_t) ch * POST_NFIR + POST_FIR_SQ_HP, X, T, demod, res, n, lane, &s_sq);
    for (int j = lane; j < n; j += 64) out[(size_t) row * out_stride + j] = (short) res[j];
}

template <bool kSam>
__global__ __launch_bounds__(64) void post_kernel(
    post_chan *__restrict__ chan_tab, post_cfir *__restrict__ cfir_tab, post_sam *__restrict__ sam_tab, float2 *__restrict__ ring_in,
    float *__restrict__ ring_mag,
    const int *__restrict__ chans, const float2 *__restrict__ fir, size_t in_stride, int n,
    short *__restrict__ o_s16, float *__restrict__ o_demod, float2 *__restrict__ o_agc, size_t out_stride, int by_chan)
{
    __shared__ float bufA[POST_MAXW + KG_POST_MAX_SAMPLES];
    __shared__ float bufB[POST_MAXW + KG_POST_MAX_SAMPLES];
    __shared__ float s_db[KG_POST_MAX_SAMPLES];
    __shared__ float2 s_agc[KG_POST_MAX_SAMPLES];
    __shared__ float s_taps[POST_MAXTAPS];
    __shared__ int s_sq;
    // one wave per channel walking sequential recursions (S-meter, CAgc): latency, among workgroups that fill the vector
    // units -- it takes the issue priority (beside the DDCs' run passes the kernel stretched from 77 to 450 .. 980 us)
    __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x, ch = chans[blockIdx.x], row = by_chan ? ch : (int) blockIdx.x;      // kg_ctx::rows_by_chan
    post_chan *pc = &chan_tab[ch];
    const post_chan c = *pc;
    const float2 *in = fir + (size_t) row * in_stride;
    float2 *rin = ring_in + (size_t) ch * POST_CIRC;
    float *rmag = ring_mag + (size_t) ch * POST_CIRC;
    const unsigned cnt = c.count;
    const int W = c.window_samples, D = c.delay_samples;

    // ---- S-meter, per-sample part (rx_sound.cpp:683-687) ----
    const float snd_max_val = (float) ((1 << (15 - 2)) - 1);
    const float snd_max_pwr = snd_max_val * snd_max_val;
    for (int j = lane; j < n; j += 64) {
        const float2 x = in[j];
        const float pwr = x.x * x.x + x.y * x.y;
        s_db[j] = 10.0 * kg_libm::log10f_glibc((float) ((pwr / snd_max_pwr) + 1e-30));      // the host libm's log10f, bit for bit (kg_libm.h)
    }

    float *P = bufA;                    // window maxima end up here, index W + j
    if (c.agc_on) {
        // ---- magnitudes (agc.cpp:189-191) into the rings and LDS ----
        for (int k = lane; k < W; k += 64) bufA[k] = rmag[(cnt - W + k) & (POST_CIRC - 1)];
        for (int j = lane; j < n; j += 64) {
            const float2 x = in[j];
            float mag = x.x * x.x + x.y * x.y;
            mag = 0.5 * kg_libm::log10f_glibc((float) (mag / (MAX_AMPLITUDE * MAX_AMPLITUDE) + 1e-16));
            bufA[W + j] = mag;
            rmag[(cnt + j) & (POST_CIRC - 1)] = mag;
            rin[(cnt + j) & (POST_CIRC - 1)] = x;
        }
        __syncthreads();
        // ---- m_Peak = max of the last W magnitudes (agc.cpp:193-210) ----
        const int L = W + n;
        float *a = bufA, *b = bufB;
        int span = 1;                   // a[i] = max of the `span` entries ending at i
        while (2 * span <= W) {
            for (int i = lane; i < L; i += 64) b[i] = i >= span ? fmaxf(a[i], a[i - span]) : a[i];
            __syncthreads();
            float *t = a; a = b; b = t;
            span *= 2;
        }
        for (int j = lane; j < n; j += 64) b[W + j] = fmaxf(a[W + j], a[W + j - (W - span)]);
        __syncthreads();
        P = b;
    }

    // ---- the sequential part: lane 0 ----
    // One active lane: every instruction costs its full latency, so the loop is written
    // without branches.  Selecting alpha first and then evaluating the reference's
    // expression (1.0 - alpha) * ave + alpha * peak once is the same arithmetic as
    // evaluating it inside the taken branch; (1.0 - alpha) is an exact double per alpha.
    float *magsel = (P == bufA) ? bufB : bufA;
    if (lane == 0) {
        float attack = c.attack_ave, decay = c.decay_ave;
        int hang = c.hang_timer;
        float savg = c.smeter_avg, tap0 = c.smeter_tap0, tap1 = c.smeter_tap1;
        const double s1 = 1.0 - c.smeter_alpha;
        const double ar1 = 1.0 - c.attack_rise_alpha, af1 = 1.0 - c.attack_fall_alpha;
        const double dr1 = 1.0 - c.decay_rise_alpha, df1 = 1.0 - c.decay_fall_alpha;
        const int half = n / 2;
        if (!c.agc_on) {
            for (int j = 0; j < n; j++) {
                savg = s1 * savg + c.smeter_alpha * s_db[j];                           // rx_sound.cpp:688
                tap0 = j == 0 ? savg : tap0;
                tap1 = j == half ? savg : tap1;                                        // :693
            }
        } else {
            const bool use_hang = c.use_hang != 0;
            for (int j = 0; j < n; j++) {
                savg = s1 * savg + c.smeter_alpha * s_db[j];
                tap0 = j == 0 ? savg : tap0;
                tap1 = j == half ? savg : tap1;
                const float peak = P[W + j];
                const bool a_up = peak > attack;                                       // agc.cpp:215-218, 232-235
                const float aa = a_up ? c.attack_rise_alpha : c.attack_fall_alpha;
                attack = (a_up ? ar1 : af1) * attack + aa * peak;
                const bool d_up = peak > decay;                                        // :220-229 / :237-240
                const float da = d_up ? c.decay_rise_alpha : c.decay_fall_alpha;
                const float moved = (d_up ? dr1 : df1) * decay + da * peak;
                const bool hold = use_hang & !d_up & (hang < c.hang_time);             // hang timer running: keep
                decay = hold ? decay : moved;
                hang = use_hang ? (d_up ? 0 : (hold ? hang + 1 : hang)) : hang;
                magsel[j] = attack > decay ? attack : decay;                           // :244-247
            }
            pc->attack_ave = attack; pc->decay_ave = decay; pc->hang_timer = hang;
            pc->count = cnt + (unsigned) n;
        }
        pc->smeter_avg = savg; pc->smeter_tap0 = tap0; pc->smeter_tap1 = tap1;
    }
    __syncthreads();

    // ---- gain and output (agc.cpp:250-253, 259-292) ----
    short *ps16 = o_s16 ? o_s16 + (size_t) row * out_stride : nullptr;
    float2 *pagc = o_agc ? o_agc + (size_t) row * out_stride : nullptr;
    float *pdem = o_demod ? o_demod + (size_t) row * out_stride : nullptr;
    for (int j = lane; j < n; j += 64) {
        float2 y;
        float mono;
        if (c.agc_on) {
            const float mag = magsel[j];
            float gain;
            if (mag <= c.knee) gain = c.fixed_gain;
            else gain = AGC_OUTSCALE * kg_libm::powf_glibc_pos(10.0f, (float) (mag * (c.gain_slope - 1.0)));    // the host libm's powf (kg_libm.h)
            // written in this launch for j >= D, by an earlier one otherwise
            const float2 d = j >= D ? in[j - D] : rin[(cnt + j - D) & (POST_CIRC - 1)];
            y.x = d.x * gain; y.y = d.y * gain;
            mono = y.x;
        } else {
            const float2 x = in[j];
            y.x = c.manual_agc_gain * x.x; y.y = c.manual_agc_gain * x.y;
            mono = y.x;
        }
        s_agc[j] = y;
        if (c.mode == KG_POST_AM) {                     // rx_sound.cpp:769-771, off the sequential loop
            const float pwr = y.x * y.x + y.y * y.y;
            s_db[j] = sqrtf(pwr);
        }
        if (c.mode == KG_POST_SSB) {                    // rx_sound.cpp:893
            if (c.deemp) s_db[j] = (float) post_mono16(mono);
            else if (ps16) ps16[j] = post_mono16(mono);
        }
        if (pagc && c.mode != KG_POST_SSB) pagc[j] = y;
    }
    __syncthreads();
    post_cfir *fir4 = cfir_tab + (size_t) ch * POST_NFIR;

    if (c.mode == KG_POST_AM) {
        // rx_sound.cpp:773-779: the DC-removal IIR is a recurrence -> lane 0; the envelope
        // is already in s_db (the S-meter is done with it), the differences go out in parallel
        float *s_dm = bufA;                             // free since the gain loop
        if (lane == 0) {
            double z1 = c.z1;
            for (int j = 0; j < n; j++) {
                const float z0 = s_db[j] + (z1 * 0.99f);
                s_dm[j] = z0 - z1;
                z1 = z0;
            }
            pc->z1 = z1;
        }
        __syncthreads();
        if (pdem)
            for (int j = lane; j < n; j += 64) pdem[j] = s_dm[j];
        // rx_sound.cpp:787: m_AM_FIR.ProcessFilter(ns_out, demod_samps_r, out_samps_s2)
        post_cfir_block(fir4 + POST_FIR_AM, bufB, s_taps, s_dm, s_db, n, lane, true);
    } else if (c.mode == KG_POST_NBFM) {
        // rx_sound.cpp:845-881
        const float max_val = 32767, clipper_val = 8192;
        for (int j = lane; j < n; j += 64) {
            const float2 y = s_agc[j];
            const float i = y.x, q = y.y;
            const float iL = j ? s_agc[j - 1].x : c.last_re, qL = j ? s_agc[j - 1].y : c.last_im;
            const float pwr = i * i + q * q;
            float out = pwr ? (max_val * 0.340447550238101026565118445432744920253753662109375 *
                               (i * (q - qL) - q * (i - iL)) / pwr) : 0;
            out = out < -clipper_val ? -clipper_val : (out > clipper_val ? clipper_val : out);
            if (pdem) pdem[j] = out;
            bufA[j] = out;
        }
        if (lane == 0 && n > 0) { pc->last_re = s_agc[n - 1].x; pc->last_im = s_agc[n - 1].y; }
        __syncthreads();
        // rx_sound.cpp:876: m_Squelch.PerformFMSquelch(ns_out, demod_samps_r, out_samps_s2)
        post_squelch_block(pc, c, fir4 + POST_FIR_SQ_HP, bufB, s_taps, bufA, s_db, n, lane, &s_sq);
    }
    if constexpr (kSam) {
        if (c.mode >= KG_POST_SAM) {                    // rx_sound.cpp:791-806 (the AGC output is in s_agc and pagc)
            __shared__ float s_ps[4 * KG_POST_MAX_SAMPLES];
            __shared__ float s_aux[2 * KG_POST_MAX_SAMPLES];
            post_sam_block(sam_tab + ch, c.mode, s_agc, bufA, bufA + KG_POST_MAX_SAMPLES, bufB, s_ps, s_db, s_aux,
                           s_aux + KG_POST_MAX_SAMPLES, pagc, n, lane);
        }
    }
    if (c.mode == KG_POST_IQ || c.mode == KG_POST_SAS || c.mode == KG_POST_QAM) return;      // stereo: no out_samps_s2 (IS_STEREO)
    // rx_sound.cpp:898-907: de-emphasis, out_samps_s2 in place
    const bool nbfm = c.mode == KG_POST_NBFM;
    const bool de_emp = nbfm ? c.deemp_nfm != 0 : c.deemp != 0;
    if (c.mode == KG_POST_SSB && !de_emp) return;               // written by the gain loop
    if (de_emp)
        post_cfir_block(fir4 + (nbfm ? POST_FIR_DEEMP_NFM : POST_FIR_DEEMP_AM_SSB), bufB, s_taps, s_db, s_db, n, lane, true);
    if (ps16)
        for (int j = lane; j < n; j += 64) ps16[j] = (short) s_db[j];
}

// ---- the noise-reduction switch (rx/rx_sound.cpp:933-949) ----
// A channel's s->nr_algo / s->nr_enable[] and its four filter objects: wdsp_ANR[type][ch] (ANR.cpp:40) and m_LMS[ch][type]
// (lms.cpp:17).  The objects persist across connections, mode changes and algo switches, as the reference's statics do; a fresh
// kg_post holds them zeroed, as the statics start.
struct post_nr {
    int algo, en[2], pad;
    kg_nr::anr_t anr[2];
    kg_nr::lms_t lms[2];
    float anr_d[2][kg_nr::ANR_DLINE], anr_w[2][kg_nr::ANR_DLINE];
    float lms_ring[2][kg_nr::LMS_RING], lms_coef[2][128];
};
#define NR_HIST 512               // history in front of the block in X: every age either filter reads (ANR <= 511, CLMS <= 420)
#define NR_WPL (kg_nr::ANR_DLINE / 64)    // ANR weights per lane at taps = 512

__device__ __forceinline__ bool post_is_stereo(int mode) { return mode == KG_POST_IQ || mode == KG_POST_SAS || mode == KG_POST_QAM; }

// wdsp_ANR_filter(ch, nr_type, n, io, io) (ANR.cpp:64-116) over the int16-valued floats io (LDS, in place).  X: LDS, NR_HIST + n
// floats (the d values by age, linear: X[NR_HIST + i - m] = d[(in_idx_i + m) & 511]); P: LDS, 512 floats, 16-byte aligned;
// S, Q: LDS, n floats.
__device__ __forceinline__ void post_anr_block(post_nr *__restrict__ nr, int t, float *io, float *X, float *P, float *S, float *Q, int n, int lane)
{
    kg_nr::anr_t w = nr->anr[t];
    float *dl = nr->anr_d[t], *wt = nr->anr_w[t];
    const int T = w.taps < 0 ? 0 : w.taps, K = (T + 63) / 64;
    for (int m = lane + 1; m <= NR_HIST; m += 64) X[NR_HIST - m] = dl[(w.in_idx + m) & kg_nr::ANR_MASK];
    for (int i = lane; i < n; i += 64) X[NR_HIST + i] = kg_nr::sample_in((short) io[i]);
    __syncthreads();
    // sigma and inv_sigp of every sample depend on the input alone: one sample per lane, its sum serial in j (:76-81, :83)
    for (int i = lane; i < n; i += 64) {
        const float *x = X + NR_HIST + i;
        float sigma = 0;
        for (int j = 0; j < T; j++) {
            const float v = x[-(int) (((unsigned) j + (unsigned) w.delay) & kg_nr::ANR_MASK)];
            sigma += v * v;
        }
        S[i] = sigma;
        Q[i] = kg_nr::anr_inv_sigp(sigma);
    }
    float wr[NR_WPL];
    int ag[NR_WPL];
#pragma unroll
    for (int k = 0; k < NR_WPL; k++) {
        const int j = lane + 64 * k;
        wr[k] = j < T ? wt[j] : 0.f;
        ag[k] = (int) (((unsigned) j + (unsigned) w.delay) & kg_nr::ANR_MASK);
    }
    __syncthreads();
    for (int i = 0; i < n; i++) {
        const float *x = X + NR_HIST + i;
#pragma unroll
        for (int k = 0; k < NR_WPL; k++)
            if (k < K && lane + 64 * k < T) P[lane + 64 * k] = wr[k] * x[-ag[k]];                // w->w[j] * w->d[idx]
        __syncthreads();
        float y = 0;                                                                            // :77-81, in j order
        int j = 0;
        for (; j + 4 <= T; j += 4) {
            const float4 p = *(const float4 *) (P + j);
            y += p.x; y += p.y; y += p.z; y += p.w;
        }
        for (; j < T; j++) y += P[j];
        float c0, c1;
        const short o = kg_nr::anr_step(w, t, x[0], y, S[i], Q[i], c0, c1);                    // :83-107, every lane
#pragma unroll
        for (int k = 0; k < NR_WPL; k++)
            if (k < K) wr[k] = kg_nr::anr_weight(wr[k], x[-ag[k]], c0, c1);                     // :109-112
        if (lane == 0) io[i] = o;
        __syncthreads();
    }
    const int in_idx = (w.in_idx - n) & kg_nr::ANR_MASK;                                        // :114, n times
#pragma unroll
    for (int k = 0; k < NR_WPL; k++)
        if (lane + 64 * k < T) wt[lane + 64 * k] = wr[k];
    for (int m = lane + 1; m <= NR_HIST; m += 64) dl[(in_idx + m) & kg_nr::ANR_MASK] = X[NR_HIST + n - m];
    if (lane == 0) { w.in_idx = in_idx; nr->anr[t] = w; }
    __syncthreads();
}

// CLMS::ProcessFilter(n, io, io) (lms.cpp:83-123).  The ring of L = m_dlen + 121 floats, linear: X[NR_HIST + i - a] is the sample of
// age a at sample i, and tap c of the Wiener filter reads age m_dlen + 120 - c.  X, P as post_anr_block.
__device__ __forceinline__ void post_lms_block(post_nr *__restrict__ nr, int t, float *io, float *X, float *P, int n, int lane)
{
    kg_nr::lms_t m = nr->lms[t];
    float *ring = nr->lms_ring[t], *coef = nr->lms_coef[t];
    const int L = m.dlen + kg_nr::LMSLEN;
    for (int a = lane + 1; a < L; a += 64) X[NR_HIST - a] = ring[(m.dlp - a + L) % L];
    for (int i = lane; i < n; i += 64) X[NR_HIST + i] = kg_nr::sample_in((short) io[i]);
    const bool two = lane + 64 < kg_nr::LMSLEN;
    float cr0 = coef[lane], cr1 = two ? coef[lane + 64] : 0.f;
    const int off0 = m.dlen + kg_nr::LMSLEN - 1 - lane, off1 = off0 - 64;
    __syncthreads();
    for (int i = 0; i < n; i++) {
        const float *x = X + NR_HIST + i;
        P[lane] = x[-off0] * cr0;                                                               // m_dline[m_dlp] * m_lmscoef[i]
        if (two) P[lane + 64] = x[-off1] * cr1;
        __syncthreads();
        float fir = 0;                                                                          // :95-99, in i order
        int c = 0;
        for (; c + 4 <= kg_nr::LMSLEN; c += 4) {
            const float4 p = *(const float4 *) (P + c);
            fir += p.x; fir += p.y; fir += p.z; fir += p.w;
        }
        for (; c < kg_nr::LMSLEN; c++) fir += P[c];
        short o = 0;
        if (m.nr_type == kg_nr::DENOISE) o = kg_nr::lms_out_denoise(fir);                        // :102-104
        const float err = kg_nr::lms_err(x[0], fir);
        if (m.nr_type == kg_nr::AUTONOTCH) o = kg_nr::sample_out(err);                           // :108-110
        const float err2 = kg_nr::lms_err2(err, m.beta);
        cr0 = kg_nr::lms_coef(x[-off0], err2, cr0, m.decay);                                    // :116-120
        if (two) cr1 = kg_nr::lms_coef(x[-off1], err2, cr1, m.decay);
        if (lane == 0) io[i] = o;
        __syncthreads();
    }
    const int dlp = (m.dlp + n) % L;
    coef[lane] = cr0;
    if (two) coef[lane + 64] = cr1;
    for (int a = lane + 1; a <= L; a += 64) ring[(dlp - a + L) % L] = X[NR_HIST + n - a];
    if (lane == 0) nr->lms[t].dlp = dlp;
    __syncthreads();
}

// kFused: the stage of c2s_sound() behind post_kernel, over its d_s16 rows in place: channels in a stereo mode, with an algo other
// than NR_WDSP / NR_ORIG or with neither type enabled return at once; else auto-notch, then denoise (:933-949).
// !kFused: kg_post_nr_process_dev, the filter of `type` under each listed channel's algo.
template <bool kFused>
__global__ __launch_bounds__(64) void post_nr_kernel(post_nr *__restrict__ nr_tab, const post_chan *__restrict__ chan_tab,
                                                     const int *__restrict__ chans, int type, const short *in, size_t in_stride, int n,
                                                     short *out, size_t out_stride, int by_chan)
{
    __shared__ float X[NR_HIST + KG_POST_MAX_SAMPLES];
    __shared__ __attribute__((aligned(16))) float P[kg_nr::ANR_DLINE];
    __shared__ float S[KG_POST_MAX_SAMPLES], Q[KG_POST_MAX_SAMPLES], io[KG_POST_MAX_SAMPLES];
    const int lane = threadIdx.x, ch = chans[blockIdx.x];
    post_nr *nr = nr_tab + ch;
    const int algo = nr->algo;
    bool an = type == kg_nr::AUTONOTCH, dn = type == kg_nr::DENOISE;
    if (kFused) {
        if (post_is_stereo(chan_tab[ch].mode) || (algo != KG_NR_WDSP && algo != KG_NR_ORIG)) return;
        an = nr->en[kg_nr::AUTONOTCH] != 0; dn = nr->en[kg_nr::DENOISE] != 0;
        if (!an && !dn) return;
    }
    const int row = kFused && by_chan ? ch : (int) blockIdx.x;                     // kg_ctx::rows_by_chan (the fused pass only)
    const short *src = in + (size_t) row * in_stride;
    short *dst = out + (size_t) row * out_stride;
    for (int i = lane; i < n; i += 64) io[i] = (float) src[i];
    __syncthreads();
    if (an) {
        if (algo == KG_NR_WDSP) post_anr_block(nr, kg_nr::AUTONOTCH, io, X, P, S, Q, n, lane);
        else post_lms_block(nr, kg_nr::AUTONOTCH, io, X, P, n, lane);
    }
    if (dn) {
        if (algo == KG_NR_WDSP) post_anr_block(nr, kg_nr::DENOISE, io, X, P, S, Q, n, lane);
        else post_lms_block(nr, kg_nr::DENOISE, io, X, P, n, lane);
    }
    for (int i = lane; i < n; i += 64) dst[i] = (short) io[i];
}

// ---- NR_SPECTRAL (rx/rx_sound.cpp:945-947 -> rx/Teensy/NR_spectral.cpp) ----
// The transform's twiddles and the sqrt-Hann window (kg_tables.h) where a lane can index them.
__device__ const kg_nrs_tw_t NRS_TW = KG_NRS_TW;
__device__ const kg_nrs_win_t NRS_WIN = KG_NRS_WIN;
enum { NRS_LSB, NRS_LIFFT, NRS_NEST, NRS_XT, NRS_PSLP, NRS_POST, NRS_PRIO, NRS_HK, NRS_G, NRS_ARRAYS };   // nr_spectral_t's order

// arm_cfft_f32(len512, F, inverse, 1) on F (LDS), one butterfly per lane and pass.  A lane owns its eight points in passes 0 and
// 1; the last pass stores to the digit-reversed places, so every lane has loaded before any stores.
__device__ __forceinline__ void post_nrs_cfft(float2 *F, int lane, bool inverse)
{
    const float invL = 1.0f / (float) kg_nrs::FFT_FULL;
    for (int pass = 0; pass < 3; pass++) {
        int i1, n2, j, mod;
        float xr[8], xi[8];
        kg_nrs::bfly_index(pass, lane, i1, n2, j, mod);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float2 v = F[i1 + k * n2];
            xr[k] = v.x; xi[k] = (inverse && pass == 0) ? -v.y : v.y;              // "conjugate input data"
        }
        kg_nrs::bfly_compute(pass, j, mod, NRS_TW.v, xr, xi);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int i = i1 + k * n2;
            if (pass < 2) F[i] = make_float2(xr[k], xi[k]);
            else if (!inverse) F[kg_nrs::rev3(i)] = make_float2(xr[k], xi[k]);
            else F[kg_nrs::rev3(i)] = make_float2(xr[k] * invL, -(xi[k]) * invL);    // "conjugate and scale output data"
        }
        __syncthreads();
    }
}

// kFused: the stage of c2s_sound() behind post_kernel over its d_s16 rows in place, for the listed channels whose algo is
// NR_SPECTRAL and whose mode is not a stereo one (the others return at once).  !kFused: kg_post_nrs_process_dev.
// n is a multiple of 512: nr_spectral_process(ch, 512, ...) once per 512 samples.
template <bool kFused>
__global__ __launch_bounds__(64) void post_nrs_kernel(kg_nrs::state_t *__restrict__ tab, const post_nr *__restrict__ nr_tab,
                                                      const post_chan *__restrict__ chan_tab, const int *__restrict__ chans,
                                                      kg_nrs::rate_t rt, const short *in, size_t in_stride, int n, short *out,
                                                      size_t out_stride, int by_chan)
{
    using namespace kg_nrs;
    __shared__ float2 F[FFT_FULL];
    __shared__ float A[NRS_ARRAYS][FFT_HALF];
    __shared__ float X[FFT_HALF];
    const int lane = threadIdx.x, ch = chans[blockIdx.x];
    if (kFused && (nr_tab[ch].algo != KG_NR_SPECTRAL || post_is_stereo(chan_tab[ch].mode))) return;
    const int row = kFused && by_chan ? ch : (int) blockIdx.x;
    const short *src = in + (size_t) row * in_stride;
    short *dst = out + (size_t) row * out_stride;
    state_t *s = tab + ch;
    int first_time = s->first_time, init_counter = s->init_counter;
    const int lo3 = s->vad_lo, hi3 = s->vad_hi;
    const par_t par = s->par;
    float *g_arr = s->last_sample_buffer;                                           // the nine arrays lie one behind the other
    for (int a = 0; a < NRS_ARRAYS; a++)
        for (int q = 0; q < 4; q++) A[a][lane + 64 * q] = g_arr[a * FFT_HALF + lane + 64 * q];
    if (first_time == 1) {                                                          // :126-135
        for (int q = 0; q < 4; q++) {
            const int b = lane + 64 * q;
            A[NRS_LSB][b] = 0.0; A[NRS_G][b] = 1.0; A[NRS_HK][b] = 1.0; A[NRS_NEST][b] = 0.0; A[NRS_PSLP][b] = 0.5;
        }
        first_time = 2;
    }
    __syncthreads();
    for (int f = 0; f < n / FFT_HALF; f++) {                                        // frame f: samples f * 256 .. of the call
        int VAD_low = 0, VAD_high = 0;
        for (int q = 0; q < 4; q++) {                                               // :140-161
            const int i = lane + 64 * q;
            const float f_samp = (float) src[f * FFT_HALF + i];
            F[i] = make_float2(A[NRS_LSB][i] * NRS_WIN.v[i / 2], 0.0f);
            F[FFT_HALF + i] = make_float2(f_samp * NRS_WIN.v[(FFT_HALF + i) / 2], 0.0f);
            A[NRS_LSB][i] = f_samp;
        }
        __syncthreads();
        post_nrs_cfft(F, lane, false);
        for (int q = 0; q < 4; q++) {
            const int b = lane + 64 * q;
            X[b] = mag2(F[b].x, F[b].y);
        }
        if (first_time == 2) {                                                      // :173-186
            for (int q = 0; q < 4; q++) {
                const int b = lane + 64 * q;
                startup_bin(X[b], A[NRS_NEST][b], A[NRS_XT][b]);
            }
            init_counter = (init_counter + 1) & 255;
            if (init_counter > INIT_FRAMES - 1) { init_counter = 0; first_time = 3; }
        }
        if (first_time == 3) {
            VAD_low = lo3; VAD_high = hi3;
            for (int q = 0; q < 4; q++) {
                const int b = lane + 64 * q;
                track_bin(par, rt.ap, rt.ax, X[b], A[NRS_XT][b], A[NRS_PSLP][b]);
                snr_bin(par, rt.snr_prio_min, X[b], A[NRS_XT][b], A[NRS_HK][b], A[NRS_POST][b], A[NRS_PRIO][b]);
                if (b >= VAD_low && b < VAD_high) gain_bin(A[NRS_POST][b], A[NRS_PRIO][b], A[NRS_G][b], A[NRS_HK][b]);
            }
            __syncthreads();
            float pre_power = 0.0, post_power = 0.0;                                // :265-271, every lane walks both sums
            for (int b = VAD_low; b < VAD_high; b++) power_step(X[b], A[NRS_G][b], pre_power, post_power);
            const int NN = smoothing_width(pre_power, post_power);
            for (int q = 0; q < 4; q++) {                                           // :284-314: reads NR_G, writes its own NR_Nest
                const int b = lane + 64 * q;
                float nest;
                if (smooth_bin(A[NRS_G], b, VAD_low, VAD_high, NN, nest)) A[NRS_NEST][b] = nest;
            }
            __syncthreads();
            for (int q = 0; q < 4; q++) {                                           // :317-320
                const int b = lane + 64 * q;
                if (b >= VAD_low + NN / 2 && b < VAD_high - NN / 2) A[NRS_G][b] = A[NRS_NEST][b];
            }
        }
        __syncthreads();
        for (int q = 0; q < 4; q++) {                                               // :329-338: bin b and bin 511 - b, as written
            const int b = lane + 64 * q;
            if (b >= VAD_low && b < VAD_high) {
                const float g = A[NRS_G][b];
                const int ai = FFT_FULL - b - 1;
                F[b] = make_float2(F[b].x * g, F[b].y * g);
                F[ai] = make_float2(F[ai].x * g, F[ai].y * g);
            }
        }
        __syncthreads();
        post_nrs_cfft(F, lane, true);
        for (int q = 0; q < 4; q++) {                                               // :344-357
            const int i = lane + 64 * q;
            const float re = F[i].x * NRS_WIN.v[i / 2];
            dst[f * FFT_HALF + i] = out_sample(re, A[NRS_LIFFT][i], par.final_gain);
            A[NRS_LIFFT][i] = F[FFT_HALF + i].x * NRS_WIN.v[(FFT_HALF + i) / 2];
        }
        __syncthreads();
    }
    for (int a = 0; a < NRS_ARRAYS; a++)
        for (int q = 0; q < 4; q++) g_arr[a * FFT_HALF + lane + 64 * q] = A[a][lane + 64 * q];
    if (lane == 0) { s->first_time = first_time; s->init_counter = init_counter; }
}

__global__ void post_nrs_vad_kernel(kg_nrs::state_t *tab, int nchan, int vad_lo, int vad_hi)     // a fresh object's passband bins
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < nchan) { tab[ch].vad_lo = vad_lo; tab[ch].vad_hi = vad_hi; }
}

// ---- NB_WILD (rx/rx_sound.cpp:922-931 -> rx/Teensy/NB_Wild.cpp) ----
// kFused: the stage of c2s_sound() behind post_kernel (de-emphasis) and ahead of the NR kernels, over d_s16 rows in place, for the
// listed channels whose switch is on and whose mode is not a stereo one (the others return at once).  !kFused:
// kg_post_nbw_process_dev.  n is a multiple of 512: nb_Wild_process(ch, 512, ...) once per 512 samples.
// One wave per channel.  Across lanes: the order + 1 autocorrelation lags (a lane walks its own 512 - i terms in order), the two FIR
// passes (one output per lane and step, its taps in order), the copies and a repair's blend.  Serial, because the arithmetic chains:
// Levinson-Durbin (lane 0), the variance's two 512-term sums (every lane walks them, the reads are broadcasts), the scan (the
// threshold tests run across lanes into eight 64-bit words; the walk over them, which skips PL samples behind a hit and stops at 20,
// is serial and every lane makes it), and per hit, in hit order, the forward prediction on lane 0 beside the backward one on lane 1
// (each step feeds the next).
template <bool kFused>
__global__ __launch_bounds__(64) void post_nbw_kernel(kg_nbw::state_t *__restrict__ tab, const post_chan *__restrict__ chan_tab,
                                                      const int *__restrict__ chans, const short *in, size_t in_stride, int n, short *out,
                                                      size_t out_stride, int by_chan)
{
    using namespace kg_nbw;
    __shared__ float WB[DIM_WBUF], T1[BLOCK], T2[BLOCK];
    __shared__ float R[MAX_ORDER + 1], LP[MAX_ORDER + 1], RL[MAX_ORDER + 1], ANY[MAX_ORDER + 1], NLP[MAX_ORDER], NRL[MAX_ORDER];
    __shared__ float RFW[MAX_IMPULSE_LEN + MAX_ORDER], RBW[MAX_IMPULSE_LEN + MAX_ORDER];
    __shared__ int POS[N_IMPULSE_COUNT];
    __shared__ unsigned long long FL[BLOCK / 64];
    const int lane = threadIdx.x, ch = chans[blockIdx.x];
    state_t *s = tab + ch;
    if (kFused && (!s->on || post_is_stereo(chan_tab[ch].mode))) return;
    const int row = kFused && by_chan ? ch : (int) blockIdx.x;
    const short *src = in + (size_t) row * in_stride;
    short *dst = out + (size_t) row * out_stride;
    const float thresh = s->thresh;
    // the host admits the stage only on a usable vector; the clamps keep every index inside the arrays whatever the table holds
    const int order = min(max(s->taps, 1), (int) MAX_ORDER);
    const int il = impulse_length(min(max(s->impulse_samples, 2), (int) MAX_IMPULSE_LEN)), PL = half_length(il);
    const int hist = 2 * PL + 2 * order;
    const float *x = WB + order + PL;
    for (int i = lane; i < hist; i += 64) WB[i] = s->hist[i];
    for (int b = 0; b < n / BLOCK; b++) {
        for (int i = lane; i < BLOCK; i += 64) WB[hist + i] = (float) src[b * BLOCK + i];                 // :258, :91
        __syncthreads();
        if (lane <= order) R[lane] = autocorr(x, lane, BLOCK);                                              // :102-109
        __syncthreads();
        if (lane == 0) levinson((float *) R, order, (float *) LP, (float *) RL, (float *) ANY);            // :111-143
        __syncthreads();
        for (int i = lane; i < BLOCK; i += 64) T1[i] = fir_sample(x, i, RL, order + 1);                     // :149
        __syncthreads();
        for (int i = lane; i < BLOCK; i += 64) T2[i] = fir_sample(T1, i, LP, order + 1);                    // :155
        if (lane < order) { NLP[lane] = -LP[1 + lane]; NRL[lane] = -RL[lane]; }                             // :187-188
        __syncthreads();
        const float sigma2 = variance(T2, BLOCK), lpc_power = power(LP, order);                             // :157-158
        const float impulse_threshold = threshold(thresh, sigma2, lpc_power);                               // :160
        for (int q = 0; q < BLOCK / 64; q++) {                                                              // :167 for every sample
            const unsigned long long m = __ballot(over(T2[lane + 64 * q], impulse_threshold));
            if (lane == 0) FL[q] = m;
        }
        __syncthreads();
        int count = scan_flags(FL, order, PL, BLOCK, POS);                      // :162-176 (every lane stores the same positions)
        count = __builtin_amdgcn_readfirstlane(count);                                                      // (every lane counted the same)
        __syncthreads();
        for (int j = 0; j < count; j++) {                                                                   // :193-235, in hit order
            const int pos = POS[j];
            if (lane < order) {
                RFW[lane] = WB[fw_base(pos, lane)];
                RBW[il + lane] = WB[bw_base(pos, lane, order, PL)];
            }
            __syncthreads();
            if (lane == 0) predict_fw((float *) RFW, NRL, order, il);
            else if (lane == 1) predict_bw((float *) RBW, NLP, order, il);
            __syncthreads();
            if (lane < il) WB[repair_base(pos, order) + lane] = blend(RFW[order + lane], RBW[lane], lane, il);
            __syncthreads();
        }
        for (int i = lane; i < BLOCK; i += 64) dst[b * BLOCK + i] = out_sample(x[i]);                       // :239, :260
        __syncthreads();
        float carry[2];
        for (int q = 0; q < 2; q++) carry[q] = lane + 64 * q < hist ? WB[BLOCK + lane + 64 * q] : 0.0f;    // :242
        __syncthreads();
        for (int q = 0; q < 2; q++) if (lane + 64 * q < hist) WB[lane + 64 * q] = carry[q];
        __syncthreads();
    }
    for (int i = lane; i < hist; i += 64) s->hist[i] = WB[i];
}

__global__ void post_reset_rings_kernel(float2 *ring_in, float *ring_mag, int ch0)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, ch = ch0 + blockIdx.y;
    if (i < POST_CIRC) {
        ring_in[(size_t) ch * POST_CIRC + i] = make_float2(0.f, 0.f);      // agc.cpp:119-121
        ring_mag[(size_t) ch * POST_CIRC + i] = -16.0f;                    // :122
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
struct post_host {               // the SetParameters() arguments last seen (agc.cpp:101-106)
    int agc_on, use_hang, threshold, manual_gain, decay;
    float slope_factor, sample_rate;
};

struct post_nr_host {             // the snd_t fields of the noise-reduction commands (rx_sound.h:130-132)
    int algo, en[2];
    float param[2][kg_nr::NPARAMS];
};

struct post_nrs_host {            // NR_SPECTRAL's host side: s->norm_locut / norm_hicut (rx_sound.h:91), nr_spectral_t's init flag
    bool init;
    float norm_locut, norm_hicut;
    int vad[2];                   // VAD_low, VAD_high of that passband at the object's rate (what the device state holds)
    kg_nrs::par_t par;
};

struct kg_post {
    kg_ctx *ctx;
    int nchan;
    kg_dbuf<post_chan> d_chan;
    kg_dbuf<float2> d_ring_in;
    kg_dbuf<float> d_ring_mag;
    kg_dbuf<post_cfir> d_cfir;           // [nchan][POST_NFIR]
    kg_dbuf<post_sam> d_sam;             // [nchan]
    std::vector<post_sam> h_sam;         // parameters only (the PLL type, its gains, the snd_rate constants, mparam)
    std::vector<post_chan> h_chan;       // parameters only; the state lives on the device
    std::vector<post_host> h_args;
    std::vector<post_cfir> h_cfir;       // taps as designed / handed over; pos and hist are the device's
    std::vector<char> h_fir_ready;       // [nchan][POST_NFIR]: initialised since create
    std::vector<char> h_sq_ready;        // kg_post_squelch_setup AND kg_post_squelch_set were called
    kg_dbuf<post_nr> d_nr;               // [nchan]
    std::vector<post_nr_host> h_nr;      // s->nr_algo, s->nr_enable[], s->nr_param[][] (the filter states are the device's)
    kg_dbuf<kg_nrs::state_t> d_nrs;      // [nchan]: nr_spectral[] (NR_spectral.cpp:69)
    std::vector<post_nrs_host> h_nrs;
    int nrs_snd_rate;                    // the reference's global snd_rate as NR_SPECTRAL sees it (kg_post_nrs_setup; 12000 at create)
    kg_nrs::rate_t nrs_rate;             // tinc .. ap, snr_prio_min at that rate
    kg_dbuf<kg_nbw::state_t> d_nbw;      // [nchan]: nb_Wild[] (NB_Wild.cpp:36) and the stage's switch
    std::vector<kg_nbw::state_t> h_nbw;  // thresh, taps, impulse_samples and the switch (hist is the device's)
    kg_stage_cache list_cache;           // the channel list of the last process call
    std::vector<uint32_t> mode_cmds;     // per channel: kg_post_set_mode / kg_post_set_sam_mparam calls so far (kg_post_mode_cmds_)
};

static int post_check(kg_post *p, int ch, const char *who)
{
    KG_REQUIRE(p != nullptr, KG_ERR_INVALID, "%s: null object", who);
    KG_REQUIRE(ch >= 0 && ch < p->nchan, KG_ERR_INVALID, "%s: channel %d out of range (0..%d)", who, ch, p->nchan - 1);
    return kg_ctx_use(p->ctx);
}

// Parameter words of post_chan are rewritten from the host copy; the state words are
// patched individually so that a parameter change never rolls the device state back.
template <typename T> static int post_put(kg_post *p, int ch, T post_chan::*field, const T &v)
{
    p->h_chan[ch].*field = v;
    const size_t off = (size_t) ((char *) &(p->h_chan[ch].*field) - (char *) &p->h_chan[ch]);
    KG_HIP(hipMemcpyAsync((char *) (p->d_chan + ch) + off, &(p->h_chan[ch].*field), sizeof(T),
                          hipMemcpyHostToDevice, p->ctx->stream));
    return KG_OK;
}

template <typename T> static int sam_put(kg_post *p, int ch, T post_sam::*field, const T &v)
{
    p->h_sam[ch].*field = v;
    const size_t off = (size_t) ((char *) &(p->h_sam[ch].*field) - (char *) &p->h_sam[ch]);
    KG_HIP(hipMemcpyAsync((char *) (p->d_sam + ch) + off, &(p->h_sam[ch].*field), sizeof(T), hipMemcpyHostToDevice, p->ctx->stream));
    return KG_OK;
}

static bool post_is_sam(int mode) { return mode >= KG_POST_SAM && mode <= KG_POST_QAM; }

// ---- wdsp_SAM_demod_init() and wdsp_SAM_PLL() (SAM_demod.cpp:113-163) on the host: f32_t members, double literals, int snd_rate
static void sam_init_consts(post_sam &w, int snd_rate)
{
    const double K_2PI = 2.0 * 3.14159265358979323846;
    const float pll_fmax = +22000.0, tauR = 0.02, tauI = 1.4;
    w.snd_rate = snd_rate;
    w.omega_min = K_2PI * (-pll_fmax) / snd_rate;
    w.omega_max = K_2PI * pll_fmax / snd_rate;
    w.mtauR = expf(-1 / (snd_rate * tauR));
    w.onem_mtauR = 1.0 - w.mtauR;
    w.mtauI = expf(-1 / (snd_rate * tauI));
    w.onem_mtauI = 1.0 - w.mtauI;
}

static void sam_gains(post_sam &w)
{
    const int snd_rate = w.snd_rate;
    w.g1 = 1.0 - expf(-2.0 * w.omegaN * w.zeta / snd_rate);
    w.g2 = -w.g1 + 2.0 * (1 - expf(-w.omegaN * w.zeta / snd_rate) * cosf(w.omegaN / snd_rate * sqrtf(1.0 - w.zeta * w.zeta)));
}

static void sam_pll_host(post_sam &w, int type)       // PLL_RESET = -1, PLL_DX, PLL_MED, PLL_FAST (wdsp.h:14)
{
    if (type == -1) {
        type = w.type;
        memset(&w, 0, offsetof(post_sam, is_chan_null));
        if (type == -1) type = 1;
        sam_pll_host(w, type);
        return;
    }
    if (type == 0) { w.zeta = 0.2; w.omegaN = 70; }
    else if (type == 1) { w.zeta = 0.65; w.omegaN = 200.0; }
    else { w.zeta = 1.0; w.omegaN = 500; }
    sam_gains(w);
    w.type = type;
}

// the PLL state as PLL_RESET leaves it, on the device
static int sam_upload_reset(kg_post *p, int ch)
{
    KG_HIP(hipMemcpyAsync(p->d_sam + ch, &p->h_sam[ch], offsetof(post_sam, is_chan_null), hipMemcpyHostToDevice, p->ctx->stream));
    return KG_OK;
}

// ---- CFir designs (fir.cpp:282-384 InitLPFilter, :403-486 InitHPFilter, :538-555 Izero): host arithmetic, operand types as there
namespace cfir_design {
static const double K_2PI = 2.0 * 3.14159265358979323846, K_PI = 3.14159265358979323846;      // datatypes.h:103-104

static float izero(float x)
{
    const float x2 = x / 2.0;
    float sum = 1.0, ds = 1.0, di = 1.0, tmp;
    const float errorlimit = 1e-9;
    do {
        tmp = x2 / di;
        tmp *= tmp;
        ds *= tmp;
        sum += ds;
        di += 1.0;
    } while (ds >= errorlimit * sum);
    return sum;
}

static float beta_of(float Astop)                             // :294-301 = :415-422
{
    if (Astop < 20.96) return 0;
    if (Astop >= 50.0) return .1102 * (Astop - 8.71);
    return .5842 * powf((Astop - 20.96), 0.4) + .07886 * (Astop - 20.96);
}

// (int) of the tap estimate; Fstop == Fpass makes it infinite, whose conversion C leaves undefined: as x86 converts it
static int to_int(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int) v : (int) 0x80000000u; }

static float kaiser(int n, int ntaps, float Beta, float izb, float Scale, float c)             // :327-328 = :451-452
{
    const float x = ((float) n - ((float) ntaps - 1.0) / 2.0) / (((float) ntaps - 1.0) / 2.0);
    return Scale * c * izero(Beta * sqrtf(1 - (x * x))) / izb;
}

static int lowpass(int NumTaps, float Scale, float Astop, float Fpass, float Fstop, float Fsamprate, float *coef)
{
    const float normFpass = Fpass / Fsamprate, normFstop = Fstop / Fsamprate;
    const float normFcut = (normFstop + normFpass) / 2.0;
    const float Beta = beta_of(Astop);
    int ntaps = to_int((Astop - 8.0) / (2.285 * K_2PI * (normFstop - normFpass)) + 1);          // :304
    if (ntaps > POST_MAXTAPS) ntaps = POST_MAXTAPS;
    if (ntaps < 9) ntaps = 9;
    if (NumTaps) ntaps = NumTaps;
    const float fCenter = .5 * (float) (ntaps - 1);
    const float izb = izero(Beta);
    for (int n = 0; n < ntaps; n++) {
        const float x = (float) n - fCenter;
        float c;
        if ((float) n == fCenter) c = 2.0 * normFcut;                                           // :322-323
        else c = (float) sinf(K_2PI * x * normFcut) / (K_PI * x);                               // :325
        coef[n] = kaiser(n, ntaps, Beta, izb, Scale, c);
    }
    return ntaps;
}

static int highpass(int NumTaps, float Scale, float Astop, float Fpass, float Fstop, float Fsamprate, float *coef)
{
    const float normFpass = Fpass / Fsamprate, normFstop = Fstop / Fsamprate;
    const float normFcut = (normFstop + normFpass) / 2.0;
    const float Beta = beta_of(Astop);
    int ntaps = to_int((Astop - 8.0) / (2.285 * K_2PI * (normFpass - normFstop)) + 1);          // :425
    if (ntaps > (POST_MAXTAPS - 1)) ntaps = POST_MAXTAPS - 1;
    if (ntaps < 3) ntaps = 3;
    ntaps |= 1;                                                                                 // :433
    if (NumTaps) ntaps = NumTaps;
    const float izb = izero(Beta);
    const float fCenter = .5 * (float) (ntaps - 1);
    for (int n = 0; n < ntaps; n++) {
        const float x = (float) n - (float) (ntaps - 1) / 2.0;                                  // :442
        float c;
        if ((float) n == fCenter) c = 1.0 - 2.0 * normFcut;                                     // :446
        else c = (float) (sinf(K_PI * x) / (K_PI * x) - sinf(K_2PI * x * normFcut) / (K_PI * x));   // :448
        coef[n] = kaiser(n, ntaps, Beta, izb, Scale, c);
    }
    return ntaps;
}
}  // namespace cfir_design

// A freshly initialised CFir on the device: the taps of h_cfir, zeroed buffer, m_State = 0 (fir.cpp:230-236, :344-350)
static int post_cfir_upload(kg_post *p, int ch, int which)
{
    post_cfir &f = p->h_cfir[(size_t) ch * POST_NFIR + which];
    f.pos = 0;
    memset(f.hist, 0, sizeof f.hist);
    KG_HIP(hipMemcpyAsync(p->d_cfir + (size_t) ch * POST_NFIR + which, &f, sizeof f, hipMemcpyHostToDevice, p->ctx->stream));
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    p->h_fir_ready[(size_t) ch * POST_NFIR + which] = 1;
    return KG_OK;
}

static int post_which(int which, bool init, const char *who)
{
    KG_REQUIRE(which == KG_CFIR_AM || which == KG_CFIR_DEEMP_NFM || which == KG_CFIR_DEEMP_AM_SSB || (!init && which == KG_CFIR_SQUELCH_HP),
               KG_ERR_INVALID, "%s: filter %d (KG_CFIR_AM, KG_CFIR_DEEMP_NFM, KG_CFIR_DEEMP_AM_SSB%s)", who, which,
               init ? "; the squelch's high-pass is designed by kg_post_squelch_setup" : ", KG_CFIR_SQUELCH_HP");
    return KG_OK;
}
static const int POST_WHICH_SLOT[4] = {POST_FIR_AM, POST_FIR_DEEMP_NFM, POST_FIR_DEEMP_AM_SSB, POST_FIR_SQ_HP};

static int post_list(kg_post *p, const int32_t *chans, int nch, const char *who, void **d_list)
{
    KG_REQUIRE(nch >= 1 && nch <= p->nchan, KG_ERR_INVALID, "%s: nch %d", who, nch);
    std::vector<char> seen(p->nchan, 0);
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(chans[i] >= 0 && chans[i] < p->nchan && !seen[chans[i]], KG_ERR_INVALID,
                   "%s: chans[%d] = %d out of range or listed twice", who, i, chans[i]);
        seen[chans[i]] = 1;
    }
    return kg_ctx_stage_cached(p->ctx, &p->list_cache, chans, sizeof(int) * nch, d_list);
}

static int post_reset_agc_state(kg_post *p, int ch)         // agc.cpp:117-131
{
    int rc;
    hipLaunchKernelGGL(post_reset_rings_kernel, dim3(POST_CIRC / 256), dim3(256), 0, p->ctx->stream,
                       p->d_ring_in, p->d_ring_mag, ch);
    KG_HIP(hipGetLastError());
    if ((rc = post_put(p, ch, &post_chan::hang_timer, 0))) return rc;
    if ((rc = post_put(p, ch, &post_chan::decay_ave, -5.0f))) return rc;
    if ((rc = post_put(p, ch, &post_chan::attack_ave, -5.0f))) return rc;
    if ((rc = post_put(p, ch, &post_chan::count, 0u))) return rc;
    return KG_OK;
}

// ---- the noise-reduction commands' state (rx/rx_sound_cmd.cpp:464-471, :505-523) ----
static bool nr_active(const post_nr_host &h, int mode)
{
    return (h.algo == KG_NR_WDSP || h.algo == KG_NR_ORIG) && (h.en[0] || h.en[1]) &&
           mode != KG_POST_IQ && mode != KG_POST_SAS && mode != KG_POST_QAM;
}

static bool nrs_active(const post_nr_host &h, int mode)
{
    return h.algo == KG_NR_SPECTRAL && mode != KG_POST_IQ && mode != KG_POST_SAS && mode != KG_POST_QAM;   // the enables are not consulted
}

static int nrs_put_vad(kg_post *p, int ch)         // VAD_low / VAD_high to the device (h_nrs is stable storage; the caller synchronises)
{
    KG_HIP(hipMemcpyAsync(&p->d_nrs[ch].vad_lo, p->h_nrs[ch].vad, sizeof(int) * 2, hipMemcpyHostToDevice, p->ctx->stream));
    return KG_OK;
}

static_assert(KG_NBW_HIST == kg_nbw::HIST_MAX && KG_NB_PARAMS == kg_nr::NPARAMS, "kiwigpu.h and kg_nbw.h disagree");
static bool nbw_active(const kg_nbw::state_t &h, int mode)
{
    return h.on && mode != KG_POST_IQ && mode != KG_POST_SAS && mode != KG_POST_QAM;
}

static int nbw_put_on(kg_post *p, int ch, int on)  // the stage's switch to the device (h_nbw is stable storage; the caller synchronises)
{
    p->h_nbw[ch].on = on;
    KG_HIP(hipMemcpyAsync(&p->d_nbw[ch].on, &p->h_nbw[ch].on, sizeof(int), hipMemcpyHostToDevice, p->ctx->stream));
    return KG_OK;
}

static int nr_put_ctl(kg_post *p, int ch)          // s->nr_algo and s->nr_enable[] to the device
{
    const post_nr_host &h = p->h_nr[ch];
    const int v[3] = {h.algo, h.en[0], h.en[1]};
    KG_HIP(hipMemcpyAsync((char *) (p->d_nr + ch) + offsetof(post_nr, algo), v, sizeof v, hipMemcpyHostToDevice, p->ctx->stream));
    KG_HIP(hipStreamSynchronize(p->ctx->stream));      // (v is on the stack)
    return KG_OK;
}

static int post_init(kg_post *p)
{
    kg_ctx *const ctx = p->ctx;
    const int nchan = p->nchan;
    KG_TRY(p->d_chan.alloc(nchan, "kg_post_create: channels"));
    KG_TRY(p->d_ring_in.alloc(POST_CIRC * (size_t) nchan, "kg_post_create: AGC rings"));
    KG_TRY(p->d_ring_mag.alloc(POST_CIRC * (size_t) nchan, "kg_post_create: AGC rings"));
    KG_TRY(p->d_cfir.alloc(POST_NFIR * (size_t) nchan, "kg_post_create: filters"));
    KG_TRY(p->d_sam.alloc(nchan, "kg_post_create: SAM states"));
    KG_TRY(p->d_nr.alloc(nchan, "kg_post_create: noise reduction"));
    KG_HIP(hipMemsetAsync(p->d_nr, 0, sizeof(post_nr) * (size_t) nchan, ctx->stream));     // the zeroed statics, NR_OFF_
    post_nr_host nh;
    memset(&nh, 0, sizeof nh);
    p->h_nr.assign(nchan, nh);
    KG_TRY(p->d_nrs.alloc(nchan, "kg_post_create: spectral noise reduction"));
    KG_HIP(hipMemsetAsync(p->d_nrs, 0, sizeof(kg_nrs::state_t) * (size_t) nchan, ctx->stream));     // the zeroed static nr_spectral[]
    post_nrs_host sh;
    memset(&sh, 0, sizeof sh);
    p->nrs_snd_rate = 12000;
    p->nrs_rate = kg_nrs::rate_consts(p->nrs_snd_rate);
    kg_nrs::vad_bins(0.f, 0.f, p->nrs_snd_rate, sh.vad[0], sh.vad[1]);
    p->h_nrs.assign(nchan, sh);
    hipLaunchKernelGGL(post_nrs_vad_kernel, dim3((nchan + 255) / 256), dim3(256), 0, ctx->stream, p->d_nrs, nchan, sh.vad[0], sh.vad[1]);
    KG_HIP(hipGetLastError());
    KG_TRY(p->d_nbw.alloc(nchan, "kg_post_create: Wild blanker"));
    KG_HIP(hipMemsetAsync(p->d_nbw, 0, sizeof(kg_nbw::state_t) * (size_t) nchan, ctx->stream));     // the zeroed static nb_Wild[]
    kg_nbw::state_t wh;
    memset(&wh, 0, sizeof wh);
    p->h_nbw.assign(nchan, wh);
    p->mode_cmds.assign(nchan, 0);
    post_sam w;                                     // a new connection at snd_rate 12000: PLL(MED), PLL(RESET) (rx_sound.cpp:302-303)
    memset(&w, 0, sizeof w);
    sam_init_consts(w, 12000);
    sam_pll_host(w, 1);
    sam_pll_host(w, -1);
    p->h_sam.assign(nchan, w);
    KG_HIP(hipMemcpyAsync(p->d_sam, p->h_sam.data(), sizeof(post_sam) * nchan, hipMemcpyHostToDevice, ctx->stream));
    post_cfir f0;
    memset(&f0, 0, sizeof f0);
    f0.ntaps = 1;                                   // CFir::CFir(), fir.cpp:60-64 (its coefficient is indeterminate there: 0 here;
    p->h_cfir.assign((size_t) nchan * POST_NFIR, f0);      // a mode that needs an uninitialised filter is refused, kg_post_process_dev)
    p->h_fir_ready.assign((size_t) nchan * POST_NFIR, 0);
    p->h_sq_ready.assign(nchan, 0);
    KG_HIP(hipMemcpyAsync(p->d_cfir, p->h_cfir.data(), sizeof(post_cfir) * p->h_cfir.size(), hipMemcpyHostToDevice, ctx->stream));
    post_chan z;
    memset(&z, 0, sizeof z);
    z.agc_on = 1;                                   // CAgc::CAgc(), agc.cpp:77-86
    z.delay_samples = 1; z.window_samples = 1;      // (int)(100.0 * .015), (int)(100.0 * .018)
    z.decay_ave = -5.0f; z.attack_ave = -5.0f;
    z.mode = KG_POST_SSB;
    z.sq_state = 1;                                 // CSquelch::Reset(), squelch.cpp:67-77
    p->h_chan.assign(nchan, z);
    post_host a = {1, 0, 0, 0, 0, 0.f, 100.0f};
    p->h_args.assign(nchan, a);
    KG_HIP(hipMemcpyAsync(p->d_chan, p->h_chan.data(), sizeof(post_chan) * nchan, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(post_reset_rings_kernel, dim3(POST_CIRC / 256, nchan), dim3(256), 0, ctx->stream,
                       p->d_ring_in, p->d_ring_mag, 0);
    KG_HIP(hipGetLastError());
    KG_HIP(hipStreamSynchronize(ctx->stream));
    return KG_OK;
}

extern "C" {

int kg_post_create(kg_ctx *ctx, int nchan, kg_post **out)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "kg_post_create: out is null");
    *out = nullptr;
    KG_REQUIRE(nchan >= 1 && nchan <= 65536, KG_ERR_INVALID, "kg_post_create: nchan %d", nchan);
    kg_post *p = new (std::nothrow) kg_post();
    KG_REQUIRE(p != nullptr, KG_ERR_NOMEM, "kg_post_create: alloc");
    p->ctx = ctx; p->nchan = nchan;
    rc = post_init(p);
    if (rc) { kg_post_destroy(p); return rc; }
    *out = p;
    return KG_OK;
}


void kg_post_destroy(kg_post *p) { kg_drain_delete(p); }

int kg_post_set_agc(kg_post *p, int ch, int agc_on, int use_hang, int threshold, int manual_gain,
                    int slope_factor, int decay, float sample_rate)
{
    int rc = post_check(p, ch, "kg_post_set_agc");
    if (rc) return rc;
    KG_REQUIRE(sample_rate >= 100.0f && (int) (sample_rate * .018) <= POST_MAXW, KG_ERR_INVALID,
               "kg_post_set_agc: sample rate %g (supported: 100 .. %d Hz)", (double) sample_rate, (int) (POST_MAXW / .018));
    post_host &a = p->h_args[ch];
    agc_on = agc_on != 0; use_hang = use_hang != 0;
    if (agc_on == a.agc_on && use_hang == a.use_hang && threshold == a.threshold && manual_gain == a.manual_gain &&
        slope_factor == a.slope_factor && decay == a.decay && sample_rate == a.sample_rate)
        return KG_OK;                                                       // agc.cpp:101-106
    a.agc_on = agc_on; a.use_hang = use_hang; a.threshold = threshold; a.manual_gain = manual_gain;
    a.slope_factor = slope_factor; a.decay = decay;
    if (a.sample_rate != sample_rate) {                                     // :115-131
        a.sample_rate = sample_rate;
        if ((rc = post_reset_agc_state(p, ch))) return rc;
    }
    const float rate = a.sample_rate;
    // agc.cpp:134-160, operand types as there (TYPEREAL members, double literals)
    const float manual_agc_gain = 32767.0 * powf(10.0, -(100 - (float) a.manual_gain) / 20.0);
    const float knee = (float) a.threshold / 20.0;
    const float gain_slope = a.slope_factor / 100.0;
    const float fixed_gain = AGC_OUTSCALE * powf(10.0, knee * (gain_slope - 1.0));
    const float ara = (1.0 - expf(-1.0 / (rate * .002)));
    const float afa = (1.0 - expf(-1.0 / (rate * .005)));
    const float dra = (1.0 - expf(-1.0 / (rate * (float) a.decay * .001 * .3)));
    const int hang_time = (int) (rate * (float) a.decay * .001);
    float dfa;
    if (a.use_hang) dfa = (1.0 - expf(-1.0 / (rate * .05)));
    else dfa = (1.0 - expf(-1.0 / (rate * (float) a.decay * .001)));
    int delay = (int) (rate * .015);
    const int window = (int) (rate * .018);
    if (delay >= 2048 - 1) delay = 2048 - 1;
    KG_REQUIRE(delay >= 1 && window >= 1, KG_ERR_INVALID, "kg_post_set_agc: delay %d window %d", delay, window);
    if ((rc = post_put(p, ch, &post_chan::agc_on, a.agc_on))) return rc;
    if ((rc = post_put(p, ch, &post_chan::use_hang, a.use_hang))) return rc;
    if ((rc = post_put(p, ch, &post_chan::delay_samples, delay))) return rc;
    if ((rc = post_put(p, ch, &post_chan::window_samples, window))) return rc;
    if ((rc = post_put(p, ch, &post_chan::hang_time, hang_time))) return rc;
    if ((rc = post_put(p, ch, &post_chan::manual_agc_gain, manual_agc_gain))) return rc;
    if ((rc = post_put(p, ch, &post_chan::knee, knee))) return rc;
    if ((rc = post_put(p, ch, &post_chan::gain_slope, gain_slope))) return rc;
    if ((rc = post_put(p, ch, &post_chan::fixed_gain, fixed_gain))) return rc;
    if ((rc = post_put(p, ch, &post_chan::attack_rise_alpha, ara))) return rc;
    if ((rc = post_put(p, ch, &post_chan::attack_fall_alpha, afa))) return rc;
    if ((rc = post_put(p, ch, &post_chan::decay_rise_alpha, dra))) return rc;
    if ((rc = post_put(p, ch, &post_chan::decay_fall_alpha, dfa))) return rc;
    KG_HIP(hipStreamSynchronize(p->ctx->stream));       // the host words just copied may change again
    return KG_OK;
}

int kg_post_agc_delay(kg_post *p, int ch)
{
    int rc = post_check(p, ch, "kg_post_agc_delay");
    if (rc) return rc;
    return p->h_chan[ch].delay_samples;
}

int kg_post_set_smeter(kg_post *p, int ch, float frate)
{
    int rc = post_check(p, ch, "kg_post_set_smeter");
    if (rc) return rc;
    KG_REQUIRE(frate > 0.f, KG_ERR_INVALID, "kg_post_set_smeter: frate %g", (double) frate);
    const float alpha = 1.0 - expf(-1.0 / ((float) frate * .01));          // rx_sound.cpp:248-249
    if ((rc = post_put(p, ch, &post_chan::smeter_alpha, alpha))) return rc;
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_set_mode(kg_post *p, int ch, int mode)
{
    int rc = post_check(p, ch, "kg_post_set_mode");
    if (rc) return rc;
    KG_REQUIRE(mode >= KG_POST_IQ && mode <= KG_POST_QAM, KG_ERR_INVALID, "kg_post_set_mode: mode %d", mode);
    if (post_is_sam(mode) || post_is_sam(p->h_chan[ch].mode)) {
        // rx_sound_cmd.cpp:214-226: a non-SAM -> SAM transition resets the PLL; every mode change clears s->isChanNull
        if (post_is_sam(mode) && !post_is_sam(p->h_chan[ch].mode)) {
            sam_pll_host(p->h_sam[ch], -1);
            if ((rc = sam_upload_reset(p, ch))) return rc;
        }
        if ((rc = sam_put(p, ch, &post_sam::is_chan_null, 0))) return rc;
    }
    if ((rc = post_put(p, ch, &post_chan::mode, mode))) return rc;
    p->mode_cmds[ch]++;
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

// ---- the three libm functions the device code calls, over an array: what tests/test_libm_gpu.py compares with the image's libm
__global__ void math_kernel(int fn, float base, const float *__restrict__ x, unsigned first, size_t n, float *__restrict__ y)
{
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
        const float v = x ? x[i] : __uint_as_float(first + (unsigned) i);
        y[i] = fn == KG_MATH_LOG10F ? kg_libm::log10f_glibc(v) : fn == KG_MATH_POWF ? kg_libm::powf_glibc_pos(base, v)
             : fn == KG_MATH_SINF ? kg_libm::sinf_glibc(v) : fn == KG_MATH_COSF ? kg_libm::cosf_glibc(v) : kg_libm::expf_glibc(v);
    }
}

__global__ void atan2f_kernel(const float *__restrict__ y, const float *__restrict__ x, size_t n, float *__restrict__ out)
{
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
        out[i] = kg_libm::atan2f_glibc(y[i], x[i]);
}

int kg_math_dev(kg_ctx *ctx, int fn, float base, const void *d_x, uint32_t first_bits, size_t n, void *d_y)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(d_y && n >= 1 && ((uintptr_t) d_y & 3) == 0 && ((uintptr_t) d_x & 3) == 0, KG_ERR_INVALID, "kg_math_dev: bad argument");
    KG_REQUIRE(fn == KG_MATH_LOG10F || fn == KG_MATH_POWF || fn == KG_MATH_EXPF || fn == KG_MATH_SINF || fn == KG_MATH_COSF, KG_ERR_INVALID,
               "kg_math_dev: unknown function");
    KG_REQUIRE(fn != KG_MATH_POWF || (base >= 1.17549435e-38f && base < __builtin_huge_valf()), KG_ERR_INVALID,
               "kg_math_dev: powf's base must be positive, finite and normal (CAgc's is 10)");
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(math_kernel, dim3((unsigned) (blocks < 16384 ? blocks : 16384)), dim3(256), 0, ctx->stream, fn, base,
                       (const float *) d_x, first_bits, n, (float *) d_y);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_math_atan2f_dev(kg_ctx *ctx, const void *d_y, const void *d_x, size_t n, void *d_out)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(d_y && d_x && d_out && n >= 1 && ((uintptr_t) d_y & 3) == 0 && ((uintptr_t) d_x & 3) == 0 && ((uintptr_t) d_out & 3) == 0,
               KG_ERR_INVALID, "kg_math_atan2f_dev: bad argument");
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(atan2f_kernel, dim3((unsigned) (blocks < 16384 ? blocks : 16384)), dim3(256), 0, ctx->stream, (const float *) d_y,
                       (const float *) d_x, n, (float *) d_out);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_post_sam_setup(kg_post *p, int ch, int snd_rate)
{
    int rc = post_check(p, ch, "kg_post_sam_setup");
    if (rc) return rc;
    KG_REQUIRE(snd_rate == 12000 || snd_rate == 20250, KG_ERR_INVALID, "kg_post_sam_setup: snd_rate %d (12000 or 20250)", snd_rate);
    post_sam &w = p->h_sam[ch];
    sam_init_consts(w, snd_rate);
    sam_gains(w);                                   // what wdsp_SAM_PLL() computes from then on
    const size_t a = offsetof(post_sam, snd_rate), b = offsetof(post_sam, onem_mtauI) + sizeof(float);
    KG_HIP(hipMemcpyAsync((char *) (p->d_sam + ch) + a, (char *) &w + a, b - a, hipMemcpyHostToDevice, p->ctx->stream));
    if ((rc = sam_put(p, ch, &post_sam::g1, w.g1))) return rc;
    if ((rc = sam_put(p, ch, &post_sam::g2, w.g2))) return rc;
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_sam_pll(kg_post *p, int ch, int type)
{
    int rc = post_check(p, ch, "kg_post_sam_pll");
    if (rc) return rc;
    KG_REQUIRE(type >= -1 && type <= 2, KG_ERR_INVALID, "kg_post_sam_pll: type %d (-1 reset, 0 DX, 1 MED, 2 FAST)", type);
    post_sam &w = p->h_sam[ch];
    sam_pll_host(w, type);
    if (type == -1) {
        if ((rc = sam_upload_reset(p, ch))) return rc;
    } else {
        if ((rc = sam_put(p, ch, &post_sam::zeta, w.zeta))) return rc;
        if ((rc = sam_put(p, ch, &post_sam::omegaN, w.omegaN))) return rc;
        if ((rc = sam_put(p, ch, &post_sam::g1, w.g1))) return rc;
        if ((rc = sam_put(p, ch, &post_sam::g2, w.g2))) return rc;
        if ((rc = sam_put(p, ch, &post_sam::type, w.type))) return rc;
    }
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_set_sam_mparam(kg_post *p, int ch, int mparam)
{
    int rc = post_check(p, ch, "kg_post_set_sam_mparam");
    if (rc) return rc;
    if ((rc = sam_put(p, ch, &post_sam::mparam, mparam & 0xf))) return rc;         // MODE_FLAGS_SAM (rx_sound.h:39)
    p->mode_cmds[ch]++;                                                            // the n == 5 case of rx_sound_cmd.cpp:202
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_sam_state(kg_post *p, const int32_t *chans, int nch, float *carrier, int32_t *is_chan_null, float *phzerror)
{
    KG_REQUIRE(p && chans, KG_ERR_INVALID, "kg_post_sam_state: null argument");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    std::vector<post_sam> h(p->nchan);
    KG_HIP(hipMemcpyAsync(h.data(), p->d_sam, sizeof(post_sam) * p->nchan, hipMemcpyDeviceToHost, p->ctx->stream));
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(chans[i] >= 0 && chans[i] < p->nchan, KG_ERR_INVALID, "kg_post_sam_state: chans[%d] = %d", i, chans[i]);
        const float c = h[chans[i]].sam_carrier;
        if (carrier) carrier[i] = c != c ? 0.f : c;                                      // wdsp_SAM_carrier() (SAM_demod.cpp:165-170)
        if (is_chan_null) is_chan_null[i] = h[chans[i]].is_chan_null;
        if (phzerror) phzerror[i] = h[chans[i]].phzerror;
    }
    return KG_OK;
}

int kg_post_get_mode(kg_post *p, int ch)
{
    int rc = post_check(p, ch, "kg_post_get_mode");
    if (rc) return rc;
    return p->h_chan[ch].mode;
}

int kg_post_reset(kg_post *p, int ch)
{
    int rc = post_check(p, ch, "kg_post_reset");
    if (rc) return rc;
    if ((rc = post_put(p, ch, &post_chan::smeter_avg, 0.f))) return rc;
    if ((rc = post_put(p, ch, &post_chan::smeter_tap0, 0.f))) return rc;
    if ((rc = post_put(p, ch, &post_chan::smeter_tap1, 0.f))) return rc;
    if ((rc = post_put(p, ch, &post_chan::z1, 0.0))) return rc;
    if ((rc = post_put(p, ch, &post_chan::last_re, 0.f))) return rc;
    if ((rc = post_put(p, ch, &post_chan::last_im, 0.f))) return rc;
    sam_pll_host(p->h_sam[ch], 1);                  // rx_sound.cpp:302-303
    sam_pll_host(p->h_sam[ch], -1);
    if ((rc = sam_upload_reset(p, ch))) return rc;
    memset(&p->h_nr[ch], 0, sizeof(post_nr_host));  // :236-240: memset(s) zeroes nr_enable / nr_param, nr_algo = NR_OFF_; the filters stay
    if ((rc = nr_put_ctl(p, ch))) return rc;
    post_nrs_host &sh = p->h_nrs[ch];               // memset(s) zeroes norm_locut / norm_hicut too; nr_spectral[ch] stays
    sh.norm_locut = sh.norm_hicut = 0.f;
    kg_nrs::vad_bins(0.f, 0.f, p->nrs_snd_rate, sh.vad[0], sh.vad[1]);
    if ((rc = nrs_put_vad(p, ch))) return rc;
    if ((rc = nbw_put_on(p, ch, 0))) return rc;     // memset(s) zeroes nb_enable[]; nb_Wild[ch] stays
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_process_dev(kg_post *p, const int32_t *chans, int nch, const void *d_fir, size_t in_stride,
                        int nsamps, void *d_s16, void *d_demod, void *d_agc, size_t out_stride)
{
    KG_REQUIRE(p && chans && d_fir, KG_ERR_INVALID, "kg_post_process_dev: null argument");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    KG_REQUIRE(nch >= 1 && nch <= p->nchan, KG_ERR_INVALID, "kg_post_process_dev: nch %d", nch);
    KG_REQUIRE(nsamps >= 1 && nsamps <= KG_POST_MAX_SAMPLES, KG_ERR_INVALID,
               "kg_post_process_dev: nsamps %d (1..%d)", nsamps, KG_POST_MAX_SAMPLES);
    KG_REQUIRE(in_stride >= (size_t) nsamps && out_stride >= (size_t) nsamps, KG_ERR_INVALID,
               "kg_post_process_dev: stride smaller than nsamps");
    KG_REQUIRE(KG_ALIGNED(d_fir, 8) && KG_ALIGNED(d_s16, 2) && KG_ALIGNED(d_demod, 4) && KG_ALIGNED(d_agc, 8), KG_ERR_INVALID,
               "kg_post_process_dev: misaligned pointer (d_fir and d_agc 8 bytes, d_demod 4, d_s16 2)");
    std::vector<char> seen(p->nchan, 0);
    bool any_sam = false, any_nr = false, any_nrs = false, any_nbw = false;
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(chans[i] >= 0 && chans[i] < p->nchan && !seen[chans[i]], KG_ERR_INVALID,
                   "kg_post_process_dev: chans[%d] = %d out of range or listed twice", i, chans[i]);
        seen[chans[i]] = 1;
        const int ch = chans[i], mode = p->h_chan[ch].mode;
        const char *fr = &p->h_fir_ready[(size_t) ch * POST_NFIR];
        KG_REQUIRE(mode != KG_POST_AM || fr[POST_FIR_AM], KG_ERR_STATE,
                   "kg_post_process_dev: channel %d is in AM mode and its m_AM_FIR was never designed (kg_post_set_am_passband)", ch);
        KG_REQUIRE(mode != KG_POST_NBFM || p->h_sq_ready[ch], KG_ERR_STATE,
                   "kg_post_process_dev: channel %d is in NBFM mode without kg_post_squelch_setup + kg_post_squelch_set (rx_sound.cpp:261-262)", ch);
        KG_REQUIRE(!(mode == KG_POST_NBFM && p->h_chan[ch].deemp_nfm) || fr[POST_FIR_DEEMP_NFM], KG_ERR_STATE,
                   "kg_post_process_dev: channel %d has NBFM de-emphasis on and no m_nfm_deemp_FIR coefficients", ch);
        const bool mono_am_ssb = mode == KG_POST_AM || mode == KG_POST_SSB || mode == KG_POST_SAM || mode == KG_POST_SAU || mode == KG_POST_SAL;
        KG_REQUIRE(!(mono_am_ssb && p->h_chan[ch].deemp) || fr[POST_FIR_DEEMP_AM_SSB], KG_ERR_STATE,
                   "kg_post_process_dev: channel %d has AM/SSB de-emphasis on and no m_am_ssb_deemp_FIR coefficients", ch);
        any_sam |= post_is_sam(mode);
        any_nr |= nr_active(p->h_nr[ch], mode);
        any_nrs |= nrs_active(p->h_nr[ch], mode);
        any_nbw |= nbw_active(p->h_nbw[ch], mode);
    }
    KG_REQUIRE(!any_nbw || (d_s16 && nsamps % kg_nbw::BLOCK == 0), KG_ERR_INVALID,
               "kg_post_process_dev: a listed channel has the Wild noise blanker on, which runs over d_s16 on blocks of %d samples: "
               "d_s16 %s, nsamps %d", kg_nbw::BLOCK, d_s16 ? "given" : "NULL", nsamps);
    KG_REQUIRE(!(any_nr || any_nrs) || d_s16, KG_ERR_INVALID,
               "kg_post_process_dev: a listed channel has noise reduction on, and it runs over d_s16: d_s16 must not be NULL");
    KG_REQUIRE(!any_nrs || nsamps % kg_nrs::FFT_FULL == 0, KG_ERR_INVALID,
               "kg_post_process_dev: a listed channel has spectral noise reduction on, which runs on blocks of %d samples: nsamps %d",
               kg_nrs::FFT_FULL, nsamps);
    hipStream_t st = p->ctx->stream;
    void *d_list = nullptr;
    if ((rc = kg_ctx_stage_cached(p->ctx, &p->list_cache, chans, sizeof(int) * nch, &d_list))) return rc;
    KG_PLAN_ONLY(p->ctx);
    // a batch with a SAM-family channel takes the kernel instance with the SAM stage (and its LDS); every other batch the one without
    hipLaunchKernelGGL(any_sam ? post_kernel<true> : post_kernel<false>, dim3(nch), dim3(64), 0, st, p->d_chan, p->d_cfir, p->d_sam,
                       p->d_ring_in, p->d_ring_mag, (const int *) d_list, (const float2 *) d_fir, in_stride, nsamps,
                       (short *) d_s16, (float *) d_demod, (float2 *) d_agc, out_stride, p->ctx->rows_by_chan);
    KG_HIP(hipGetLastError());
    if (any_nbw) {                                  // rx_sound.cpp:922-931 over the rows just written, ahead of the NR switch
        hipLaunchKernelGGL(post_nbw_kernel<true>, dim3(nch), dim3(64), 0, st, p->d_nbw, p->d_chan, (const int *) d_list,
                           (const short *) d_s16, out_stride, nsamps, (short *) d_s16, out_stride, p->ctx->rows_by_chan);
        KG_HIP(hipGetLastError());
    }
    // rx_sound.cpp:933-949 over the rows just written, only for a batch that holds a channel with NR on (the others return at once)
    if (any_nr) {
        hipLaunchKernelGGL(post_nr_kernel<true>, dim3(nch), dim3(64), 0, st, p->d_nr, p->d_chan, (const int *) d_list, -1,
                           (const short *) d_s16, out_stride, nsamps, (short *) d_s16, out_stride, p->ctx->rows_by_chan);
        KG_HIP(hipGetLastError());
    }
    if (any_nrs) {                                  // :945-947, likewise
        hipLaunchKernelGGL(post_nrs_kernel<true>, dim3(nch), dim3(64), 0, st, p->d_nrs, p->d_nr, p->d_chan, (const int *) d_list, p->nrs_rate,
                           (const short *) d_s16, out_stride, nsamps, (short *) d_s16, out_stride, p->ctx->rows_by_chan);
        KG_HIP(hipGetLastError());
    }
    return KG_OK;
}

int kg_post_cfir_init_lp(kg_post *p, int ch, int which, int NumTaps, float Scale, float Astop, float Fpass, float Fstop, float Fsamprate)
{
    int rc = post_check(p, ch, "kg_post_cfir_init_lp");
    if (rc || (rc = post_which(which, true, "kg_post_cfir_init_lp"))) return rc;
    KG_REQUIRE(NumTaps >= 0 && NumTaps <= POST_MAXTAPS && Fsamprate > 0.f, KG_ERR_INVALID,
               "kg_post_cfir_init_lp: NumTaps %d (0..%d), sample rate %g", NumTaps, POST_MAXTAPS, (double) Fsamprate);
    post_cfir &f = p->h_cfir[(size_t) ch * POST_NFIR + POST_WHICH_SLOT[which]];
    f.ntaps = cfir_design::lowpass(NumTaps, Scale, Astop, Fpass, Fstop, Fsamprate, f.taps);
    if ((rc = post_cfir_upload(p, ch, POST_WHICH_SLOT[which]))) return rc;
    return f.ntaps;
}

int kg_post_cfir_init_const(kg_post *p, int ch, int which, int NumTaps, const float *coef, float Fsamprate)
{
    int rc = post_check(p, ch, "kg_post_cfir_init_const");
    if (rc || (rc = post_which(which, true, "kg_post_cfir_init_const"))) return rc;
    KG_REQUIRE(coef != nullptr && NumTaps >= 1, KG_ERR_INVALID, "kg_post_cfir_init_const: %d coefficients at %p", NumTaps, (const void *) coef);
    (void) Fsamprate;                                           // m_SampleRate is only used by GenerateHBFilter
    post_cfir &f = p->h_cfir[(size_t) ch * POST_NFIR + POST_WHICH_SLOT[which]];
    f.ntaps = NumTaps > POST_MAXTAPS ? POST_MAXTAPS : NumTaps;  // fir.cpp:223-226
    memcpy(f.taps, coef, sizeof(float) * (size_t) f.ntaps);
    if ((rc = post_cfir_upload(p, ch, POST_WHICH_SLOT[which]))) return rc;
    return f.ntaps;
}

int kg_post_cfir_get_taps(kg_post *p, int ch, int which, float *taps)
{
    int rc = post_check(p, ch, "kg_post_cfir_get_taps");
    if (rc || (rc = post_which(which, false, "kg_post_cfir_get_taps"))) return rc;
    const post_cfir &f = p->h_cfir[(size_t) ch * POST_NFIR + POST_WHICH_SLOT[which]];
    if (taps) memcpy(taps, f.taps, sizeof(float) * (size_t) f.ntaps);
    return f.ntaps;
}

int kg_post_cfir_process_dev(kg_post *p, const int32_t *chans, int nch, int which, int kind, const void *d_in, size_t in_stride, int nsamps,
                             void *d_out, size_t out_stride)
{
    KG_REQUIRE(p && chans && d_in && d_out, KG_ERR_INVALID, "kg_post_cfir_process_dev: null argument");
    int rc = kg_ctx_use(p->ctx);
    if (rc || (rc = post_which(which, false, "kg_post_cfir_process_dev"))) return rc;
    KG_REQUIRE(kind >= KG_CFIR_REAL_REAL && kind <= KG_CFIR_MONO16_MONO16, KG_ERR_INVALID, "kg_post_cfir_process_dev: kind %d", kind);
    KG_REQUIRE(KG_ALIGNED(d_in, kind == KG_CFIR_MONO16_MONO16 ? 2 : 4) && KG_ALIGNED(d_out, kind == KG_CFIR_REAL_REAL ? 4 : 2), KG_ERR_INVALID,
               "kg_post_cfir_process_dev: misaligned pointer (float rows 4 bytes, int16 rows 2)");
    KG_REQUIRE(nsamps >= 1 && nsamps <= KG_POST_MAX_SAMPLES && in_stride >= (size_t) nsamps && out_stride >= (size_t) nsamps, KG_ERR_INVALID,
               "kg_post_cfir_process_dev: nsamps %d (1..%d), strides %zu / %zu", nsamps, KG_POST_MAX_SAMPLES, in_stride, out_stride);
    void *d_list = nullptr;
    if ((rc = post_list(p, chans, nch, "kg_post_cfir_process_dev", &d_list))) return rc;
    for (int i = 0; i < nch; i++)
        KG_REQUIRE(p->h_fir_ready[(size_t) chans[i] * POST_NFIR + POST_WHICH_SLOT[which]], KG_ERR_STATE,
                   "kg_post_cfir_process_dev: filter %d of channel %d was never initialised", which, chans[i]);
    KG_PLAN_ONLY(p->ctx);
    hipLaunchKernelGGL(post_cfir_kernel, dim3(nch), dim3(64), 0, p->ctx->stream, p->d_cfir, (const int *) d_list, POST_WHICH_SLOT[which], kind,
                       d_in, in_stride, nsamps, d_out, out_stride);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_post_squelch_perform_dev(kg_post *p, const int32_t *chans, int nch, const void *d_in, size_t in_stride, int nsamps, void *d_out,
                                size_t out_stride)
{
    KG_REQUIRE(p && chans && d_in && d_out, KG_ERR_INVALID, "kg_post_squelch_perform_dev: null argument");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    KG_REQUIRE(nsamps >= 1 && nsamps <= KG_POST_MAX_SAMPLES && in_stride >= (size_t) nsamps && out_stride >= (size_t) nsamps, KG_ERR_INVALID,
               "kg_post_squelch_perform_dev: nsamps %d (1..%d; squelch.cpp:155 returns at once past 1024), strides %zu / %zu", nsamps,
               KG_POST_MAX_SAMPLES, in_stride, out_stride);
    KG_REQUIRE(KG_ALIGNED(d_in, 4) && KG_ALIGNED(d_out, 2), KG_ERR_INVALID, "kg_post_squelch_perform_dev: misaligned pointer (d_in 4 bytes, d_out 2)");
    void *d_list = nullptr;
    if ((rc = post_list(p, chans, nch, "kg_post_squelch_perform_dev", &d_list))) return rc;
    for (int i = 0; i < nch; i++)
        KG_REQUIRE(p->h_sq_ready[chans[i]], KG_ERR_STATE, "kg_post_squelch_perform_dev: channel %d: kg_post_squelch_setup + kg_post_squelch_set first",
                   chans[i]);
    KG_PLAN_ONLY(p->ctx);
    hipLaunchKernelGGL(post_squelch_kernel, dim3(nch), dim3(64), 0, p->ctx->stream, p->d_chan, p->d_cfir, (const int *) d_list,
                       (const float *) d_in, in_stride, nsamps, (short *) d_out, out_stride);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_post_set_am_passband(kg_post *p, int ch, double locut, double hicut, double frate)
{
    // rx_sound_cmd.cpp:248-250: the handler first clamps the client's cuts to the Nyquist limit less one (idempotent for a caller that
    // passes the clamped s->locut / s->hicut); :268-282: "hbw for post AM det is max of hi/lo filter cuts"
    const int fmax = frate / 2 - 1;
    if (hicut > fmax) hicut = fmax;
    if (locut < -fmax) locut = -fmax;
    float hbw = fmaxf(fabs(hicut), fabs(locut));
    if (hbw > frate / 2) hbw = frate / 2;
    float stop = hbw * 1.8;
    if (stop > frate / 2) stop = frate / 2;
    return kg_post_cfir_init_lp(p, ch, KG_CFIR_AM, 0, 1.0, 50.0, hbw, stop, frate);
}

int kg_post_set_deemp(kg_post *p, int ch, int nfm, int de_emp)
{
    int rc = post_check(p, ch, "kg_post_set_deemp");
    if (rc) return rc;
    if ((rc = post_put(p, ch, nfm ? &post_chan::deemp_nfm : &post_chan::deemp, de_emp))) return rc;     // rx_sound_cmd.cpp:554
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_squelch_setup(kg_post *p, int ch, float samplerate)
{
    int rc = post_check(p, ch, "kg_post_squelch_setup");
    if (rc) return rc;
    KG_REQUIRE(samplerate > 0.f, KG_ERR_INVALID, "kg_post_squelch_setup: sample rate %g", (double) samplerate);
    // squelch.cpp:84-116: the noise average's time constant, the high-pass above the voice band (:135-139), Reset()
    const float squelch_hp_freq = 3000.0;                                                       // VOICE_BANDWIDTH, :46, :106
    const float alpha = (1.0 - expf(-1.0 / (samplerate * .02)));                                // :107
    post_cfir &f = p->h_cfir[(size_t) ch * POST_NFIR + POST_FIR_SQ_HP];
    f.ntaps = cfir_design::highpass(0, 1.0, 50.0, squelch_hp_freq * .8, squelch_hp_freq * .65, samplerate, f.taps);
    if ((rc = post_cfir_upload(p, ch, POST_FIR_SQ_HP))) return rc;
    if ((rc = post_put(p, ch, &post_chan::sq_alpha, alpha))) return rc;
    return kg_post_squelch_reset(p, ch);
}

int kg_post_squelch_reset(kg_post *p, int ch)                   // squelch.cpp:67-77
{
    int rc = post_check(p, ch, "kg_post_squelch_reset");
    if (rc) return rc;
    if ((rc = post_put(p, ch, &post_chan::sq_ave, 0.f))) return rc;
    if ((rc = post_put(p, ch, &post_chan::sq_state, 1))) return rc;
    if ((rc = post_put(p, ch, &post_chan::sq_set, 0))) return rc;
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_squelch_set(kg_post *p, int ch, int Value, int SquelchMax)
{
    int rc = post_check(p, ch, "kg_post_squelch_set");
    if (rc) return rc;
    KG_REQUIRE(p->h_fir_ready[(size_t) ch * POST_NFIR + POST_FIR_SQ_HP], KG_ERR_STATE,
               "kg_post_squelch_set: kg_post_squelch_setup first (rx_sound.cpp:261-262)");
    if (SquelchMax == 0) SquelchMax = 8192;                                                     // SQUELCH_MAX = CLIPPER_NBFM_VAL, squelch.cpp:57
    const float threshold = (float) (SquelchMax - ((SquelchMax * Value) / 99));                 // :126
    if ((rc = post_put(p, ch, &post_chan::sq_value, (float) Value))) return rc;
    if ((rc = post_put(p, ch, &post_chan::sq_threshold, threshold))) return rc;
    if ((rc = post_put(p, ch, &post_chan::sq_set, 1))) return rc;
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    p->h_sq_ready[ch] = 1;
    return KG_OK;
}

int kg_post_squelch_state(kg_post *p, const int32_t *chans, int nch, int32_t *nsq_nc_sq, int32_t *squelched, float *ave)
{
    KG_REQUIRE(p && chans, KG_ERR_INVALID, "kg_post_squelch_state: null argument");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    std::vector<post_chan> h(p->nchan);
    KG_HIP(hipMemcpyAsync(h.data(), p->d_chan, sizeof(post_chan) * p->nchan, hipMemcpyDeviceToHost, p->ctx->stream));
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(chans[i] >= 0 && chans[i] < p->nchan, KG_ERR_INVALID, "kg_post_squelch_state: chans[%d] = %d", i, chans[i]);
        if (nsq_nc_sq) nsq_nc_sq[i] = h[chans[i]].sq_rc;
        if (squelched) squelched[i] = h[chans[i]].squelched;
        if (ave) ave[i] = h[chans[i]].sq_ave;
    }
    return KG_OK;
}

int kg_post_smeter(kg_post *p, const int32_t *chans, int nch, float *avg_dB, float *taps)
{
    KG_REQUIRE(p && chans && avg_dB, KG_ERR_INVALID, "kg_post_smeter: null argument");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    std::vector<post_chan> h(p->nchan);
    KG_HIP(hipMemcpyAsync(h.data(), p->d_chan, sizeof(post_chan) * p->nchan, hipMemcpyDeviceToHost, p->ctx->stream));
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(chans[i] >= 0 && chans[i] < p->nchan, KG_ERR_INVALID, "kg_post_smeter: chans[%d] = %d", i, chans[i]);
        avg_dB[i] = h[chans[i]].smeter_avg;
        if (taps) { taps[2 * i] = h[chans[i]].smeter_tap0; taps[2 * i + 1] = h[chans[i]].smeter_tap1; }
    }
    return KG_OK;
}

int kg_post_set_nr_algo(kg_post *p, int ch, int algo)
{
    int rc = post_check(p, ch, "kg_post_set_nr_algo");
    if (rc) return rc;
    KG_REQUIRE(algo != KG_NR_SPECTRAL, KG_ERR_INVALID, "kg_post_set_nr_algo: NR_SPECTRAL is selected by kg_post_nrs_select");
    post_nr_host &h = p->h_nr[ch];
    h.algo = algo;                                  // rx_sound_cmd.cpp:465-469: any other value is a switch without a case
    h.en[0] = h.en[1] = 0;
    return nr_put_ctl(p, ch);
}

int kg_post_set_nr_enable(kg_post *p, int ch, int type, int en)
{
    int rc = post_check(p, ch, "kg_post_set_nr_enable");
    if (rc) return rc;
    KG_REQUIRE(type == KG_NR_DENOISE || type == KG_NR_AUTONOTCH, KG_ERR_INVALID, "kg_post_set_nr_enable: type %d", type);
    p->h_nr[ch].en[type] = en;                      // :506-509
    return nr_put_ctl(p, ch);
}

int kg_post_set_nr_param(kg_post *p, int ch, int type, int param, float pval)
{
    int rc = post_check(p, ch, "kg_post_set_nr_param");
    if (rc) return rc;
    KG_REQUIRE(type == KG_NR_DENOISE || type == KG_NR_AUTONOTCH, KG_ERR_INVALID, "kg_post_set_nr_param: type %d", type);
    KG_REQUIRE(param >= 0 && param < kg_nr::NPARAMS, KG_ERR_INVALID, "kg_post_set_nr_param: param %d (0..%d)", param, kg_nr::NPARAMS - 1);
    post_nr_host &h = p->h_nr[ch];
    float v[kg_nr::NPARAMS];
    memcpy(v, h.param[type], sizeof v);
    v[param] = pval;                                // :512-521: stored, then type `type` of the current algo re-initialised from v
    KG_REQUIRE(h.algo != KG_NR_WDSP || kg_nr::anr_params_ok(v), KG_ERR_INVALID,
               "kg_post_set_nr_param: wdsp_ANR_init would be undefined on taps %g, delay %g (finite, in int; taps <= 512, "
               "delay <= INT_MAX - 1022)", (double) v[0], (double) v[1]);
    KG_REQUIRE(h.algo != KG_NR_ORIG || kg_nr::lms_params_ok(v), KG_ERR_INVALID,
               "kg_post_set_nr_param: CLMS::Initialize would convert a NaN delay-line length");
    memcpy(h.param[type], v, sizeof v);
    post_nr *d = p->d_nr + ch;
    hipStream_t st = p->ctx->stream;
    if (h.algo == KG_NR_WDSP) {
        post_nr f;                                  // (a staging copy; only the slot of `type` is used)
        kg_nr::anr_init(f.anr[type], f.anr_d[type], f.anr_w[type], v);
        KG_HIP(hipMemcpyAsync(&d->anr[type], &f.anr[type], sizeof f.anr[type], hipMemcpyHostToDevice, st));
        KG_HIP(hipMemcpyAsync(d->anr_d[type], f.anr_d[type], sizeof f.anr_d[type], hipMemcpyHostToDevice, st));
        KG_HIP(hipMemcpyAsync(d->anr_w[type], f.anr_w[type], sizeof f.anr_w[type], hipMemcpyHostToDevice, st));
        KG_HIP(hipStreamSynchronize(st));
    } else if (h.algo == KG_NR_ORIG) {
        post_nr f;
        memset(f.lms_coef[type], 0, sizeof f.lms_coef[type]);
        kg_nr::lms_init(f.lms[type], f.lms_ring[type], f.lms_coef[type], type, v);
        KG_HIP(hipMemcpyAsync(&d->lms[type], &f.lms[type], sizeof f.lms[type], hipMemcpyHostToDevice, st));
        KG_HIP(hipMemcpyAsync(d->lms_ring[type], f.lms_ring[type], sizeof f.lms_ring[type], hipMemcpyHostToDevice, st));
        KG_HIP(hipMemcpyAsync(d->lms_coef[type], f.lms_coef[type], sizeof f.lms_coef[type], hipMemcpyHostToDevice, st));
        KG_HIP(hipStreamSynchronize(st));
    } else if (h.algo == KG_NR_SPECTRAL) {          // :520: nr_spectral_init(rx_chan, s->nr_param[n_type]), one state for either type
        post_nrs_host &sh = p->h_nrs[ch];
        kg_nrs::state_t *ds = p->d_nrs + ch;
        kg_nrs::state_t f;                          // (a staging copy of the first init's seeds)
        if (!sh.init) {                             // NR_spectral.cpp:85-101
            sh.init = true;
            kg_nrs::init_first(f);
            KG_HIP(hipMemcpyAsync(&ds->first_time, &f.first_time, sizeof(int), hipMemcpyHostToDevice, st));
            KG_HIP(hipMemcpyAsync(ds->last_sample_buffer, f.last_sample_buffer, sizeof f.last_sample_buffer, hipMemcpyHostToDevice, st));
            KG_HIP(hipMemcpyAsync(ds->NR_Hk_old, f.NR_Hk_old, sizeof f.NR_Hk_old, hipMemcpyHostToDevice, st));
            KG_HIP(hipMemcpyAsync(ds->NR_SNR_post, f.NR_SNR_post, sizeof f.NR_SNR_post, hipMemcpyHostToDevice, st));
            KG_HIP(hipMemcpyAsync(ds->NR_SNR_prio, f.NR_SNR_prio, sizeof f.NR_SNR_prio, hipMemcpyHostToDevice, st));
        }
        kg_nrs::init_params(sh.par, v);             // :103-108
        KG_HIP(hipMemcpyAsync(&ds->par, &sh.par, sizeof sh.par, hipMemcpyHostToDevice, st));
        KG_HIP(hipStreamSynchronize(st));
    }
    return KG_OK;
}

int kg_post_nrs_select(kg_post *p, int ch)
{
    int rc = post_check(p, ch, "kg_post_nrs_select");
    if (rc) return rc;
    const post_nrs_host &sh = p->h_nrs[ch];
    KG_REQUIRE(kg_nrs::vad_ok(sh.vad[0], sh.vad[1]), KG_ERR_INVALID,
               "kg_post_nrs_select: channel %d: passband %g..%g Hz is bins %d..%d at %d Hz; NR_spectral.cpp indexes outside its arrays "
               "unless VAD_high >= %d and VAD_low <= %d (kg_post_nrs_passband first)", ch, (double) sh.norm_locut, (double) sh.norm_hicut,
               sh.vad[0], sh.vad[1], p->nrs_snd_rate, kg_nrs::VAD_HIGH_MIN, kg_nrs::VAD_LOW_MAX);
    post_nr_host &h = p->h_nr[ch];
    h.algo = KG_NR_SPECTRAL;                        // rx_sound_cmd.cpp:465-469
    h.en[0] = h.en[1] = 0;
    return nr_put_ctl(p, ch);
}

int kg_post_nrs_setup(kg_post *p, int snd_rate)
{
    KG_REQUIRE(p != nullptr, KG_ERR_INVALID, "kg_post_nrs_setup: null object");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    KG_REQUIRE(snd_rate >= 1000 && snd_rate <= 1000000, KG_ERR_INVALID, "kg_post_nrs_setup: snd_rate %d", snd_rate);
    std::vector<int> vad(2 * (size_t) p->nchan);
    for (int ch = 0; ch < p->nchan; ch++) {
        kg_nrs::vad_bins(p->h_nrs[ch].norm_locut, p->h_nrs[ch].norm_hicut, snd_rate, vad[2 * ch], vad[2 * ch + 1]);
        KG_REQUIRE(p->h_nr[ch].algo != KG_NR_SPECTRAL || kg_nrs::vad_ok(vad[2 * ch], vad[2 * ch + 1]), KG_ERR_INVALID,
                   "kg_post_nrs_setup: at %d Hz channel %d's passband is bins %d..%d, outside what NR_SPECTRAL can run on", snd_rate, ch,
                   vad[2 * ch], vad[2 * ch + 1]);
    }
    p->nrs_snd_rate = snd_rate;
    p->nrs_rate = kg_nrs::rate_consts(snd_rate);
    for (int ch = 0; ch < p->nchan; ch++) {
        p->h_nrs[ch].vad[0] = vad[2 * ch]; p->h_nrs[ch].vad[1] = vad[2 * ch + 1];
        if ((rc = nrs_put_vad(p, ch))) return rc;
    }
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_nrs_passband(kg_post *p, int ch, double locut, double hicut)
{
    int rc = post_check(p, ch, "kg_post_nrs_passband");
    if (rc) return rc;
    float nl, nh;
    int vl, vh;
    kg_nrs::norm_passband(locut, hicut, nl, nh);    // rx_sound_cmd.cpp:252-266
    kg_nrs::vad_bins(nl, nh, p->nrs_snd_rate, vl, vh);
    KG_REQUIRE(p->h_nr[ch].algo != KG_NR_SPECTRAL || kg_nrs::vad_ok(vl, vh), KG_ERR_INVALID,
               "kg_post_nrs_passband: channel %d runs NR_SPECTRAL, and %g..%g Hz is bins %d..%d at %d Hz: NR_spectral.cpp indexes outside "
               "its arrays unless VAD_high >= %d and VAD_low <= %d", ch, (double) nl, (double) nh, vl, vh, p->nrs_snd_rate,
               kg_nrs::VAD_HIGH_MIN, kg_nrs::VAD_LOW_MAX);
    post_nrs_host &sh = p->h_nrs[ch];
    sh.norm_locut = nl; sh.norm_hicut = nh;
    sh.vad[0] = vl; sh.vad[1] = vh;
    if ((rc = nrs_put_vad(p, ch))) return rc;
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_nrs_process_dev(kg_post *p, const int32_t *chans, int nch, const void *d_in, size_t in_stride, int nsamps, void *d_out,
                            size_t out_stride)
{
    KG_REQUIRE(p && chans && d_in && d_out, KG_ERR_INVALID, "kg_post_nrs_process_dev: null argument");
    KG_REQUIRE(KG_ALIGNED(d_in, 2) && KG_ALIGNED(d_out, 2), KG_ERR_INVALID, "kg_post_nrs_process_dev: int16 rows must be 2-byte aligned");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    KG_REQUIRE(nsamps >= kg_nrs::FFT_FULL && nsamps <= KG_NRS_MAX_SAMPLES && nsamps % kg_nrs::FFT_FULL == 0 && in_stride >= (size_t) nsamps &&
               out_stride >= (size_t) nsamps, KG_ERR_INVALID,
               "kg_post_nrs_process_dev: nsamps %d (a multiple of %d up to %d), strides %zu / %zu", nsamps, kg_nrs::FFT_FULL,
               KG_NRS_MAX_SAMPLES, in_stride, out_stride);
    void *d_list = nullptr;
    if ((rc = post_list(p, chans, nch, "kg_post_nrs_process_dev", &d_list))) return rc;
    for (int i = 0; i < nch; i++)
        KG_REQUIRE(p->h_nr[chans[i]].algo == KG_NR_SPECTRAL, KG_ERR_STATE,
                   "kg_post_nrs_process_dev: channel %d: its algo is %d (kg_post_nrs_select)", chans[i], p->h_nr[chans[i]].algo);
    KG_PLAN_ONLY(p->ctx);
    hipLaunchKernelGGL(post_nrs_kernel<false>, dim3(nch), dim3(64), 0, p->ctx->stream, p->d_nrs, p->d_nr, p->d_chan, (const int *) d_list,
                       p->nrs_rate, (const short *) d_in, in_stride, nsamps, (short *) d_out, out_stride, 0);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_post_nrs_state(kg_post *p, const int32_t *chans, int nch, int32_t *ints, float *scalars, float *rate, float *arrays)
{
    KG_REQUIRE(p && chans && nch >= 0, KG_ERR_INVALID, "kg_post_nrs_state: null argument");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(chans[i] >= 0 && chans[i] < p->nchan, KG_ERR_INVALID, "kg_post_nrs_state: chans[%d] = %d", i, chans[i]);
        kg_nrs::state_t hs;
        KG_HIP(hipMemcpyAsync(&hs, p->d_nrs + chans[i], sizeof hs, hipMemcpyDeviceToHost, p->ctx->stream));
        KG_HIP(hipStreamSynchronize(p->ctx->stream));
        const post_nrs_host &sh = p->h_nrs[chans[i]];
        if (ints) { ints[4 * i] = hs.first_time; ints[4 * i + 1] = hs.init_counter; ints[4 * i + 2] = hs.vad_lo; ints[4 * i + 3] = hs.vad_hi; }
        if (scalars) {
            const float v[8] = {hs.par.final_gain, hs.par.alpha, hs.par.asnr, hs.par.xih1, hs.par.xih1r, hs.par.pfac, sh.norm_locut, sh.norm_hicut};
            memcpy(scalars + 8 * (size_t) i, v, sizeof v);
        }
        if (arrays) memcpy(arrays + (size_t) i * NRS_ARRAYS * kg_nrs::FFT_HALF, hs.last_sample_buffer, sizeof(float) * NRS_ARRAYS * kg_nrs::FFT_HALF);
    }
    if (rate) memcpy(rate, &p->nrs_rate, sizeof p->nrs_rate);
    return KG_OK;
}

int kg_post_nbw_init(kg_post *p, int ch, const float *nb_param)
{
    int rc = post_check(p, ch, "kg_post_nbw_init");
    if (rc) return rc;
    KG_REQUIRE(nb_param != nullptr, KG_ERR_INVALID, "kg_post_nbw_init: null argument");
    kg_nbw::state_t &h = p->h_nbw[ch];
    kg_nbw::state_t v = h;
    kg_nbw::init_params(v, nb_param);               // NB_Wild.cpp:42-44
    KG_REQUIRE(!h.on || kg_nbw::usable(v), KG_ERR_INVALID,
               "kg_post_nbw_init: channel %d has the stage on, and NB_Wild.cpp cannot run on thresh %g, taps %g, samples %g (thresh "
               "finite, taps 1..%d, samples 2..%d)", ch, (double) nb_param[kg_nbw::P_THRESH], (double) nb_param[kg_nbw::P_TAPS],
               (double) nb_param[kg_nbw::P_SAMPLES], kg_nbw::MAX_ORDER, kg_nbw::MAX_IMPULSE_LEN);
    h.thresh = v.thresh; h.taps = v.taps; h.impulse_samples = v.impulse_samples;
    hipStream_t st = p->ctx->stream;
    KG_HIP(hipMemsetAsync(p->d_nbw[ch].hist, 0, sizeof h.hist, st));                        // :41, the history included
    KG_HIP(hipMemcpyAsync(&p->d_nbw[ch], &h, offsetof(kg_nbw::state_t, hist), hipMemcpyHostToDevice, st));
    KG_HIP(hipStreamSynchronize(st));
    return KG_OK;
}

int kg_post_set_nbw(kg_post *p, int ch, int on)
{
    int rc = post_check(p, ch, "kg_post_set_nbw");
    if (rc) return rc;
    on = on != 0;
    KG_REQUIRE(!on || kg_nbw::usable(p->h_nbw[ch]), KG_ERR_STATE,
               "kg_post_set_nbw: channel %d: NB_Wild.cpp cannot run on thresh %g, taps %d, samples %d (kg_post_nbw_init first: thresh "
               "finite, taps 1..%d, samples 2..%d)", ch, (double) p->h_nbw[ch].thresh, p->h_nbw[ch].taps, p->h_nbw[ch].impulse_samples,
               kg_nbw::MAX_ORDER, kg_nbw::MAX_IMPULSE_LEN);
    if ((rc = nbw_put_on(p, ch, on))) return rc;
    KG_HIP(hipStreamSynchronize(p->ctx->stream));
    return KG_OK;
}

int kg_post_nbw_process_dev(kg_post *p, const int32_t *chans, int nch, const void *d_in, size_t in_stride, int nsamps, void *d_out,
                            size_t out_stride)
{
    KG_REQUIRE(p && chans && d_in && d_out, KG_ERR_INVALID, "kg_post_nbw_process_dev: null argument");
    KG_REQUIRE(KG_ALIGNED(d_in, 2) && KG_ALIGNED(d_out, 2), KG_ERR_INVALID, "kg_post_nbw_process_dev: int16 rows must be 2-byte aligned");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    KG_REQUIRE(nsamps >= kg_nbw::BLOCK && nsamps <= KG_NBW_MAX_SAMPLES && nsamps % kg_nbw::BLOCK == 0 && in_stride >= (size_t) nsamps &&
               out_stride >= (size_t) nsamps, KG_ERR_INVALID,
               "kg_post_nbw_process_dev: nsamps %d (a multiple of %d up to %d), strides %zu / %zu", nsamps, kg_nbw::BLOCK,
               KG_NBW_MAX_SAMPLES, in_stride, out_stride);
    void *d_list = nullptr;
    if ((rc = post_list(p, chans, nch, "kg_post_nbw_process_dev", &d_list))) return rc;
    for (int i = 0; i < nch; i++)
        KG_REQUIRE(kg_nbw::usable(p->h_nbw[chans[i]]), KG_ERR_STATE,
                   "kg_post_nbw_process_dev: channel %d: thresh %g, taps %d, samples %d is not a vector NB_Wild.cpp can run on "
                   "(kg_post_nbw_init)", chans[i], (double) p->h_nbw[chans[i]].thresh, p->h_nbw[chans[i]].taps,
                   p->h_nbw[chans[i]].impulse_samples);
    KG_PLAN_ONLY(p->ctx);
    hipLaunchKernelGGL(post_nbw_kernel<false>, dim3(nch), dim3(64), 0, p->ctx->stream, p->d_nbw, p->d_chan, (const int *) d_list,
                       (const short *) d_in, in_stride, nsamps, (short *) d_out, out_stride, 0);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_post_nbw_state(kg_post *p, const int32_t *chans, int nch, int32_t *ints, float *floats)
{
    KG_REQUIRE(p && chans && nch >= 0, KG_ERR_INVALID, "kg_post_nbw_state: null argument");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(chans[i] >= 0 && chans[i] < p->nchan, KG_ERR_INVALID, "kg_post_nbw_state: chans[%d] = %d", i, chans[i]);
        kg_nbw::state_t hs;
        KG_HIP(hipMemcpyAsync(&hs, p->d_nbw + chans[i], sizeof hs, hipMemcpyDeviceToHost, p->ctx->stream));
        KG_HIP(hipStreamSynchronize(p->ctx->stream));
        if (ints) { ints[3 * i] = hs.taps; ints[3 * i + 1] = hs.impulse_samples; ints[3 * i + 2] = hs.on; }
        if (floats) {
            float *f = floats + (size_t) i * (1 + kg_nbw::HIST_MAX);
            f[0] = hs.thresh;
            memcpy(f + 1, hs.hist, sizeof hs.hist);     // (an init zeroes all of it; a call writes the first 2 * order + 2 * PL)
        }
    }
    return KG_OK;
}

int kg_post_nr_process_dev(kg_post *p, const int32_t *chans, int nch, int type, const void *d_in, size_t in_stride, int nsamps,
                           void *d_out, size_t out_stride)
{
    KG_REQUIRE(p && chans && d_in && d_out, KG_ERR_INVALID, "kg_post_nr_process_dev: null argument");
    KG_REQUIRE(KG_ALIGNED(d_in, 2) && KG_ALIGNED(d_out, 2), KG_ERR_INVALID, "kg_post_nr_process_dev: int16 rows must be 2-byte aligned");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    KG_REQUIRE(type == KG_NR_DENOISE || type == KG_NR_AUTONOTCH, KG_ERR_INVALID, "kg_post_nr_process_dev: type %d", type);
    KG_REQUIRE(nsamps >= 1 && nsamps <= KG_POST_MAX_SAMPLES && in_stride >= (size_t) nsamps && out_stride >= (size_t) nsamps, KG_ERR_INVALID,
               "kg_post_nr_process_dev: nsamps %d (1..%d), strides %zu / %zu", nsamps, KG_POST_MAX_SAMPLES, in_stride, out_stride);
    void *d_list = nullptr;
    if ((rc = post_list(p, chans, nch, "kg_post_nr_process_dev", &d_list))) return rc;
    for (int i = 0; i < nch; i++)
        KG_REQUIRE(p->h_nr[chans[i]].algo == KG_NR_WDSP || p->h_nr[chans[i]].algo == KG_NR_ORIG, KG_ERR_STATE,
                   "kg_post_nr_process_dev: channel %d: its algo is %d (KG_NR_WDSP or KG_NR_ORIG)", chans[i], p->h_nr[chans[i]].algo);
    KG_PLAN_ONLY(p->ctx);
    hipLaunchKernelGGL(post_nr_kernel<false>, dim3(nch), dim3(64), 0, p->ctx->stream, p->d_nr, p->d_chan, (const int *) d_list, type,
                       (const short *) d_in, in_stride, nsamps, (short *) d_out, out_stride, 0);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_post_nr_state(kg_post *p, const int32_t *chans, int nch, int type, int32_t *anr_i, float *anr_f, int32_t *lms_i, float *anr_w,
                     float *lms_coef)
{
    KG_REQUIRE(p && chans && nch >= 0, KG_ERR_INVALID, "kg_post_nr_state: null argument");
    int rc = kg_ctx_use(p->ctx);
    if (rc) return rc;
    KG_REQUIRE(type == KG_NR_DENOISE || type == KG_NR_AUTONOTCH, KG_ERR_INVALID, "kg_post_nr_state: type %d", type);
    post_nr h;
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(chans[i] >= 0 && chans[i] < p->nchan, KG_ERR_INVALID, "kg_post_nr_state: chans[%d] = %d", i, chans[i]);
        KG_HIP(hipMemcpyAsync(&h, p->d_nr + chans[i], sizeof h, hipMemcpyDeviceToHost, p->ctx->stream));
        KG_HIP(hipStreamSynchronize(p->ctx->stream));
        const kg_nr::anr_t &a = h.anr[type];
        const kg_nr::lms_t &m = h.lms[type];
        if (anr_i) { anr_i[3 * i] = a.in_idx; anr_i[3 * i + 1] = a.taps; anr_i[3 * i + 2] = a.delay; }
        if (anr_f) { anr_f[2 * i] = a.lidx; anr_f[2 * i + 1] = a.ngamma; }
        if (lms_i) { lms_i[3 * i] = m.dlp; lms_i[3 * i + 1] = m.dlen; lms_i[3 * i + 2] = m.nr_type; }
        if (anr_w) memcpy(anr_w + (size_t) i * kg_nr::ANR_DLINE, h.anr_w[type], sizeof h.anr_w[type]);
        if (lms_coef) memcpy(lms_coef + (size_t) i * kg_nr::LMSLEN, h.lms_coef[type], sizeof(float) * kg_nr::LMSLEN);
    }
    return KG_OK;
}

}  // extern "C"

// for kg_rxbank.hip (not part of the ABI): what its mirror of s->specAF_instance / s->isChanNull needs without a device sync
uint32_t kg_post_mode_cmds_(const kg_post *p, int ch) { return p->mode_cmds[ch]; }
int kg_post_sam_mparam_(const kg_post *p, int ch) { return p->h_sam[ch].mparam; }
