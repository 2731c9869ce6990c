// kg_spec.h -- the audio spectrum row of c2s_sound(), specAF_FFT (rx/rx_sound.cpp:175-220), on the device AND the host, in the
// reference's own operand types like kg_nbw.h and kg_nrs.h.  Library and host driver are built with -ffp-contract=off.  What lives here:
//   * the scale (:201-202) of both instances, evaluated left to right in float as written;
//   * one bin's byte (:198, :209-215): re * re (the real part ONLY, as the reference has it), 10.0 * log10f(pwr * scale + (float) 1e-30)
//     rounded to float, the clamps, the decrement and (u1_t) (int);
//   * a row with its half-swap (:214-215), for the host model;
//   * the 125 ms limiter (:186-195).
// log10f is the host libm's on the host and its bit-for-bit restatement on the device (kg_libm.h), so a row is an exact function of
// the spectrum on both sides.
// NaN is OUTSIDE the contract: (int) NaN is undefined in the reference, no test feeds one.  +-inf, and a power or product that
// overflows to inf, are inside: log10f(inf) = inf, clamped to 0, byte 255.
#ifndef KG_SPEC_H
#define KG_SPEC_H
#include <math.h>
#include <stdint.h>

#include "kg_nr.h"
#if defined(__HIPCC__)
#include "kg_libm.h"
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KG_SPEC_LOG10F(x) kg_libm::log10f_glibc(x)     // the host libm's log10f, bit for bit (kg_libm.h)
#else
#define KG_SPEC_LOG10F(x) log10f(x)
#endif

namespace kg_spec {

enum { WIDTH = 1024 };                                 // FFT_WIDTH = CONV_FFT_SIZE (:180)
enum { UPDATE_MS = 125 };                              // :187
enum { PASSBAND = 0, CHAN_NULL = 1 };                  // SND_INSTANCE_FFT_PASSBAND, SND_INSTANCE_FFT_CHAN_NULL (rx_sound.h:34-35)
enum { SPEC_SND_AF = 2, N_SND_SPEC = 3 };              // rx_sound.h:81-82

// :201-202 with CUTESDR_MAX_VAL = (float) 32767 (kiwi.h:42-43): 0x1.3131c4p-26 (passband), 0x1.0628f6p-57 (channel null)
KG_NR_HD float scale(int inst)
{
    const float max_val = (float) ((1 << 15) - 1);
    float s = 10.0f * 2.0f / (max_val * max_val * WIDTH * WIDTH);
    s *= inst == CHAN_NULL ? 0.0004f : 1e6f;
    return s;
}

// one bin (:198, :209-215).  10.0 * log10f() is a double product rounded to float: a 24-bit times a 4-bit significand is exact in
// double, so it is the float product.
KG_NR_HD unsigned char bin_byte(float re, float scale_)
{
    const float pwr = re * re;
    float dB = (float) (10.0 * (double) KG_SPEC_LOG10F(pwr * scale_ + (float) 1e-30));
    if (dB > 0) dB = 0;
    if (dB < -200.0) dB = -200.0;
    dB--;
    return (unsigned char) (int) dB;
}

// where bin i goes in the row (:214-215)
KG_NR_HD int unwrap(int i) { return i ^ (WIDTH / 2); }

// a row from WIDTH complex floats (re, im interleaved)
inline void row(const float *samps, int inst, unsigned char *fft)
{
    const float s = scale(inst);
    for (int i = 0; i < WIDTH; i++) fft[unwrap(i)] = bin_byte(samps[2 * i], s);
}

// "limit update rate" (:186-195): 1 when a row handed over at now_ms is sent.  The first call fires only when now_ms > 125.
inline int due(uint32_t *last_ms, uint32_t now_ms)
{
    if (now_ms > *last_ms + UPDATE_MS) {
        if (*last_ms) *last_ms += UPDATE_MS;
        else *last_ms = now_ms;
        return 1;
    }
    return 0;
}

// `SET spc_=%d` (rx_sound_cmd.cpp:333-337): what of n switches the rows on
inline int cmd_on(int n)
{
    if (n < 0 || n >= N_SND_SPEC) n = 0;
    return n == SPEC_SND_AF;
}

// The emission rule per receiver, decided on the host (kg_rxbank.hip): `inst` mirrors s->specAF_instance / s->isChanNull, which
// change together (rx_sound_cmd.cpp:227-228, rx_sound.cpp:802-803).
//   cleared  by the mode command (every kg_post_set_mode and kg_post_set_sam_mparam)
//   block    one 512-sample sound block: the passband filter's row goes out while the mirror says PASSBAND at that block
//            (fastfir.cpp:253); then the SAM family's demodulator sets the mirror (the other modes leave it alone), and in
//            channel-null SAM the nulled pair is fed to the second filter (rx_sound.cpp:804), whose instance equals the mirror by
//            then: its fill goes out.  That filter is fed 512 samples a block from FirPos() 0, so every feed completes a fill.
struct emit_t { int inst; };
struct rows_t { int passband, chan_null; };            // rows of this block, in this order
inline void emit_clear(emit_t &e) { e.inst = PASSBAND; }
inline rows_t emit_block(emit_t &e, bool spec_on, bool sam_family, bool sam_null)
{
    rows_t r;
    r.passband = spec_on && e.inst == PASSBAND;
    if (sam_family) e.inst = sam_null ? CHAN_NULL : PASSBAND;
    r.chan_null = spec_on && sam_null;
    return r;
}

}  // namespace kg_spec
#endif
