// kg_fftext.h -- the FFT extension (extensions/FFT/FFT.cpp): fft_msgs (:193-261) and fft_data (:69-191), the one consumer of
// receive_FFT(POST_FILTERED), on the device AND the host, in the reference's own operand types like kg_spec.h.  Library and host
// driver are built with -ffp-contract=off.  What lives here:
//   * `SET run=%d` (:206-244): the instance chosen AT THE COMMAND (CHAN_NULL only for FUNC_SPEC while snd->isSAM), the scale
//     10.0 * 2.0 / (CUTESDR_MAX_VAL^2 * INTEG_WIDTH^2) -- a float denominator under a DOUBLE quotient stored to float, unlike
//     specAF_FFT's all-float one -- times the boost 1e4 (wf, integ), 1e6 (spec), 100 (spec under isSAM; QAM the same), last_ms = 0
//     under FUNC_SPEC.  The command does not latch `reset`;
//   * `SET itime=%lf` and `SET clear` (:246-258): both latch `reset`;
//   * the head of fft_data (:72-101): the other instance's block ignored first; a latched reset (fft_sec, bins, fi = 0, pwr and ncma
//     zeroed); under FUNC_INTEG bin = trunc(fmod(fi, time) / time * bins), fi += fft_sec, a block with bin >= MAX_BINS dropped AFTER fi
//     advanced; otherwise bin 0.  No sample enters it: the schedule runs on the host;
//   * the body (:114-167): pwr[0][i] = re * re outside FUNC_INTEG (the real part only, overwriting), pwr[bin][i] += re * re + im * im
//     and ncma[bin]++ under it; the byte 10.0 * log10f(pwr * scale + (float) 1e-30) clamped to [-200, 0], decremented, (u1_t) (int),
//     stored at i ^ 512;
//   * the 100 ms limiter of FUNC_SPEC (:174-186).
// What the reference leaves undefined is refused (block() answers a negative value and changes nothing): a FUNC_INTEG block while
// `time` is not finite or not above 0 (fmod(fi, 0) is NaN and (int) of it indexes pwr), a reset whose time / fft_sec does not fit an
// int.  NaN samples are OUTSIDE the contract as in kg_spec.h; +-inf and overflow are inside and give byte 255.
#ifndef KG_FFTEXT_H
#define KG_FFTEXT_H
#include <math.h>
#include <stdint.h>

#include "kg_nr.h"
#if defined(__HIPCC__)
#include "kg_libm.h"
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KG_FFTEXT_LOG10F(x) kg_libm::log10f_glibc(x)   // the host libm's log10f, bit for bit (kg_libm.h)
#else
#define KG_FFTEXT_LOG10F(x) log10f(x)
#endif

namespace kg_fftext_cf {

enum { WIDTH = 1024 };                                 // INTEG_WIDTH = CONV_FFT_SIZE (:33)
enum { MAX_BINS = 200 };                               // :38
enum { UPDATE_MS = 100 };                              // :177
enum { RATIO = 2 };                                    // CONV_FFT_TO_OUTBUF_RATIO, what fastfir.cpp:302 hands over
enum { FUNC_OFF = -1, FUNC_WF = 0, FUNC_SPEC = 1, FUNC_INTEG = 2 };      // :66
enum { PASSBAND = 0, CHAN_NULL = 1 };                  // SND_INSTANCE_FFT_PASSBAND, SND_INSTANCE_FFT_CHAN_NULL (rx_sound.h:34-35)
enum { REFUSED_TIME = -1, REFUSED_BINS = -2 };         // block()'s refusals

// e of :40-59 without its buffers.  A connection starts with the function off, nothing latched and time 0.
struct state_t {
    int run, instance;
    float fft_scale, spectrum_scale;
    uint32_t last_ms;
    int reset;
    double time, fft_sec;
    int bins;
    double fi;
};
inline void init(state_t &e)
{
    e.run = FUNC_OFF; e.instance = PASSBAND; e.fft_scale = e.spectrum_scale = 0; e.last_ms = 0; e.reset = 0; e.time = 0; e.fft_sec = 0;
    e.bins = 0; e.fi = 0;
}

// :211 with CUTESDR_MAX_VAL = (float) 32767 (kiwi.h:42-43): the denominator is a float product, the quotient a double one
inline float base_scale()
{
    const float max_val = (float) ((1 << 15) - 1);
    return (float) (10.0 * 2.0 / (max_val * max_val * WIDTH * WIDTH));
}

// `SET run=%d` (:206-244); is_sam / is_qam: snd->isSAM and snd->mode == MODE_QAM at the command.  0, or -1 for a run outside -1 .. 2
// (nothing changed: the reference's switch would leave the scales of the function before).
inline int cmd_run(state_t &e, int run, bool is_sam, bool is_qam)
{
    if (run < FUNC_OFF || run > FUNC_INTEG) return -1;
    e.run = run;
    if (run == FUNC_OFF) return 0;
    const float scale = base_scale();
    float boost = 1;
    if (run == FUNC_SPEC) {
        e.instance = is_sam ? CHAN_NULL : PASSBAND;
        (void) is_qam;                                 // :225 asks, and answers 100 for QAM and for the rest of the SAM family alike
        boost = is_sam ? 100 : 1e6;
        e.last_ms = 0;
    } else {
        e.instance = PASSBAND;
        boost = 1e4;
    }
    e.spectrum_scale = scale * boost;
    e.fft_scale = scale * boost;
    return 0;
}
inline void cmd_itime(state_t &e, double itime) { e.time = itime; e.reset = 1; }   // :246-252
inline void cmd_clear(state_t &e) { e.reset = 1; }                                // :254-258

// The head of fft_data (:72-101) for one block of `instance` at the sample rate srate (ext_update_get_sample_rateHz, a double).
// 1: the block is taken, *bin says where, *did_reset whether pwr / ncma are to be zeroed ahead of it; 0: ignored (the other instance,
// or the function off) or dropped (bin >= MAX_BINS; *did_reset may still be set); negative: refused, e unchanged.
inline int block(state_t &e, int instance, double srate, int *bin, int *did_reset)
{
    *did_reset = 0;
    if (e.run == FUNC_OFF || instance != e.instance) return 0;
    double fft_sec = e.fft_sec, fi = e.fi;
    int bins = e.bins;
    if (e.reset) {
        fft_sec = 1.0 / (srate * RATIO / WIDTH);
        const double q = e.time / fft_sec;
        if (!(q > -2147483649.0 && q < 2147483648.0)) return REFUSED_BINS;
        bins = (int) trunc(q);
        fi = 0;
    }
    if (e.run == FUNC_INTEG && !(e.time > 0 && e.time <= 1.79769313486231570815e308)) return REFUSED_TIME;
    if (e.reset) { *did_reset = 1; e.reset = 0; }
    e.fft_sec = fft_sec; e.bins = bins;
    int b = 0;
    if (e.run == FUNC_INTEG) {
        const double fr = fmod(fi, e.time);
        const double fb = fr / e.time;
        const double fbin = fb * bins;
        b = (int) trunc(fbin);                         // 0 <= fbin < bins: fits
        fi += fft_sec;
    }
    e.fi = fi;
    if (b >= MAX_BINS) return 0;
    *bin = b;
    return 1;
}

// what the block's row is scaled with (:152)
KG_NR_HD float row_scale(int run, float fft_scale, float spectrum_scale) { return run == FUNC_SPEC ? spectrum_scale : fft_scale; }

// the power a block adds to (or, outside FUNC_INTEG, puts in place of) its column's sum (:116, :127-128)
KG_NR_HD float power(float re, float im, bool integ) { return integ ? re * re + im * im : re * re; }

// one column's byte (:158-166).  10.0 * log10f() is a double product rounded to float: a 24-bit times a 4-bit significand is exact in
// double, so it is the float product.
KG_NR_HD unsigned char bin_byte(float pwr, float scale)
{
    float dB = (float) (10.0 * (double) KG_FFTEXT_LOG10F(pwr * scale + (float) 1e-30));
    if (dB > 0) dB = 0;
    if (dB < -200.0) dB = -200.0;
    dB--;
    return (unsigned char) (int) dB;
}

// where column i goes in the row (:165-166)
KG_NR_HD int unwrap(int i) { return i ^ (WIDTH / 2); }

// the body for one taken block on the host: samps = WIDTH complex floats (re, im interleaved), pwr = the sums of the block's bin
inline void body(const state_t &e, const float *samps, float *pwr, int *ncma, unsigned char *fft)
{
    const bool integ = e.run == FUNC_INTEG;
    const float scale = row_scale(e.run, e.fft_scale, e.spectrum_scale);
    for (int i = 0; i < WIDTH; i++) {
        const float p = power(samps[2 * i], samps[2 * i + 1], integ);
        if (integ) pwr[i] += p;
        else pwr[i] = p;
    }
    if (integ) (*ncma)++;
    for (int i = 0; i < WIDTH; i++) fft[unwrap(i)] = bin_byte(pwr[i], scale);
}

// "limit spectrum update rate" (:174-186): 1 when the row of a block handed over at now_ms is sent.  Only FUNC_SPEC is limited.
inline int due(state_t &e, uint32_t now_ms)
{
    if (e.run != FUNC_SPEC) return 1;
    if (now_ms > e.last_ms + UPDATE_MS) {
        if (e.last_ms) e.last_ms += UPDATE_MS;
        else e.last_ms = now_ms;
        return 1;
    }
    return 0;
}

}  // namespace kg_fftext_cf
#endif
