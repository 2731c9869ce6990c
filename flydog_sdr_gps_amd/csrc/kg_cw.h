// kg_cw.h -- the CW decoder extension (extensions/CW_decoder/uhsdr_cw_decoder.cpp; cw_decoder.cpp for the commands), the second
// consumer of the real-samples task tap: the 16-bit mono audio a sound block ends as.  On the device AND the host, in the reference's
// own operand types (float32_t is float); library, host driver and golden are built with -ffp-contract=off.  What lives here, with the
// lines of uhsdr_cw_decoder.cpp it restates:
//   * CwDecode_Init (:345-392): cmd_init.  A memset with defaults: weight_linear, threshold_linear, isAutoThreshold, process_samples,
//     the Goertzel coefficients and sample_counter fall back to 0 until the client sends them again.  The fixed-WPM branch (:362-385) in
//     its float and double arithmetic as written; its `EXT cw_train=0` (:385) is implied by the command and is no event of a push.
//   * CwDecode_pboff with AudioFilter_CalcGoertzel (:296-305, :394-402): pboff_a, cmd_pboff.  g->a is an int formed from a double
//     expression; sinf / cosf are kg_libm_trig.h's on the device.  It zeroes b0..b2, which are zero between blocks anyway, and leaves
//     sample_counter and raw_signal_buffer alone: the reference runs the Goertzel over the WHOLE buffered block when its 88th sample
//     arrives (:433-436), so a pboff in mid block applies to the block's earlier samples too.  The port keeps the buffer (raw[]), not a
//     running b1 / b2, for that reason.
//   * CwDecode_wsc (:1020-1024), CwDecode_threshold (:1026-1041): cmd_wsc, cmd_auto_threshold, cmd_threshold.
//   * CwDecode_RxProcessor (:609-625): a sample is (float) s16 / 4; a Goertzel block is CW_DECODER_BLOCKSIZE_DEFAULT = 88 samples, so
//     512-sample sound blocks do not align with it; sample_counter and the buffer are carried across pushes.
//   * CW_Decode_exe (:423-607): goertzel_mag (b0 = r * b1 - b2 + in, the energy with sqrtf) and exe -- the automatic-threshold branch
//     (decayavg with the integer weights weight_linear / 1000 / 4, * 16 and * 48, CLAMP, 0.8 * in double, the signed root), the
//     fixed-threshold branch, the two-tap low pass (not recursive: old_siglevel holds the previous RAW value; its products with
//     SIGNAL_TAU are in double), the comparison with the uint32_t threshold as a float, the noise-cancel confirmation, the ring of 256
//     (state, time) entries, ONE_SECOND = snd_rate / blocksize as the integer division it is (136 at 12000) with the clamp at
//     ONE_SECOND * CW_TIMEOUT, the PARIS speed with its 0.3 / 0.7 low pass, and cw->speed.
//   * cw_train (:646-732), cw_DataRecognition (:797-938) with its equations 4.10 to 4.14 (the (uint32_t) time - pulse_avg mix of types
//     as written), CodeGenFunc (:946-957), CwGen_CharacterIdFunc (:278-294) over the 58-entry code table (:189-248, restated as data of
//     ours: twelve prosigns, then the characters; `=` stands behind <bt> with the same elements and is never found), PrintCharFunc
//     (:964-988), WordSpaceFunc (:998-1018), ErrorCorrectionFunc (:1058-1228: both corrective actions, the three reprocessing loops
//     capped at 1024, the writes into sig[]), CW_Decode (:1241-1296) with err_cnt and err_timeout.
//   * spikecancel is always 0 and noisecancel_enable always 1 in the reference and no command sets them: constants here, and the spike
//     branches (:743-780) are not ported.
// TIME IS AN INPUT: the reference reads timer_sec() in PrintCharFunc (:983) and for err_timeout (:1277, :1289); here a push carries
// now_sec, which holds for every block of it.
// DEFINED HERE where the reference leaves it open:
//   1. `static int slowdown` (:519) is shared by all channels there; here it is per connection (what a lone connection sees), survives
//      cmd_init as a static does, and is zero at create.
//   2. cw->speed = speed_wpm_avg (:606) and int16_t x of WordSpaceFunc (:1007) convert floats that can leave the target's range: as
//      x86-64 gcc yields them, cvt_i32 (truncate to int32, 0x80000000 out of range or NaN), then the low byte / the low 16 bits.
//   3. data[data_len - 1] with data_len == 0 (:862, :874) IS reached: a character that ends in a dash and is finalised by the time-out
//      (:915-925) leaves b.dash set with data_len 0, and the next space reads data[-1].  Defined as the struct layout gives on x86-64
//      gcc: the word before data[] is sig_timer, whose upper 31 bits are the time (last_time).
// What the state machine cannot reach, shown from the code: ErrorCorrectionFunc's over-long branch (:1062-1066) -- CW_Decode calls
// CodeGenFunc (:1260), which zeroes data_len, before it -- and a SUCCESS of the second corrective action (:1215): each reprocessing
// loop runs until sig_outcount meets sig_incount (cw_DataRecognition returns true for every state it takes, not per character), so the
// third loop finds nothing, CodeGenFunc gives code 0 and CharacterIdFunc 0xfe.  Both are ported as written.
// EVENTS (ev_t; include/kiwigpu.h kg_cw_ev): CHARS a = the character, the prosign index 0..11, 0xff for [err] or ' '; WPM a = speed;
// TRAIN a = the value (negative: the error count); PLOT a, c = the two floats' bits, b = the flag.
// THE BOUND, 7 events a Goertzel block: exe sends at most one PLOT; CW_Decode at most one TRAIN from cw_train, then EITHER a character
// with its word space (2 CHARS) OR an error correction (at most 2 CHARS: :1217-1218) with the error count's TRAIN, in both cases at most
// one WPM (now_sec is fixed within a push, so wpm_update matches from the second PrintCharFunc on) and the time-out's TRAIN (:1292):
// 1 + 1 + 2 + 1 + 1 + 1 = 7.  A push of nblk sound blocks completes at most (512 nblk + 87) / 88 Goertzel blocks.
// REFUSED, nothing changed: training_interval outside 1 .. 255 (the ring); wpm negative; a pboff for which g->a leaves 0 .. blocksize / 2,
// or before the first start (blocksize is 0: 0 / 0); a sample rate that is not finite, not positive or outside half to twice the
// nominal; a nominal rate below blocksize (ONE_SECOND is then 0) or above 1e6.
// NOT ported: the test-file player (cw_file_data, SET cw_test), cw_task's sequence numbers, the printfs.
#ifndef KG_CW_H
#define KG_CW_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "kg_nr.h"
#if defined(__HIPCC__)
#include "kg_libm.h"
#include "kg_libm_trig.h"
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KG_CW_SINF(x) kg_libm::sinf_glibc(x)            // the host libm's, bit for bit (kg_libm_trig.h, kg_libm.h)
#define KG_CW_COSF(x) kg_libm::cosf_glibc(x)
#define KG_CW_LOG10F(x) kg_libm::log10f_glibc(x)
#else
#define KG_CW_SINF(x) sinf(x)
#define KG_CW_COSF(x) cosf(x)
#define KG_CW_LOG10F(x) log10f(x)
#endif

namespace kg_cw_cf {

enum { BLK = 512, GBLK = 88, SIG_BUFSIZE = 256, DATA_BUFSIZE = 40, TRAINING_STABLE = 32, CW_TIMEOUT = 3, ERROR_TIMEOUT = 8, N_CODE = 58, EVENTS_PER_GBLK = 7 };
enum { AUTO_WEIGHT_LINEAR = 32000, AUTO_THRESHOLD_LINEAR = 15849, DIT = 2, DAH = 3 };
enum { EV_CHARS = 0, EV_WPM = 1, EV_TRAIN = 2, EV_PLOT = 3 };
enum { REFUSED_INTERVAL = -1, REFUSED_WPM = -2, REFUSED_PBOFF = -3, REFUSED_RATE = -4, REFUSED_NOT_STARTED = -5 };
#define KG_CW_PI (3.14159265358979323846)                  /* K_PI, datatypes.h:104 */
#define KG_CW_SIGNAL_TAU 0.1                               /* :51 */

// cw_decoder_t (:106-174) as the port keeps it: a sigbuf_t (:81-84) is one word, bit 0 the state and the upper 31 the time, as the
// bit fields lie on x86-64.  The layout is kg_cw_info's (include/kiwigpu.h).
struct state_t {
    int32_t process_samples; uint32_t wpm_update; int32_t wsc, err_cnt, err_timeout; float sampling_freq; int32_t speed, isAutoThreshold;
    uint32_t weight_linear, threshold_linear; int32_t blocksize;
    int32_t g_a; float g_b, g_sin, g_cos, g_r;
    int32_t sig_lastrx, sig_incount, sig_outcount, sig_timer;
    int32_t data_len; uint32_t code; int32_t state, initialized, dash, wspace, timeout, track;
    float pulse_avg, dot_avg, dash_avg, symspace_avg, cwspace_avg; int32_t w_space;
    int32_t timer_stepsize, cur_time, cur_outcount, last_outcount;
    float CW_env, CW_mag, CW_noise, old_siglevel, speed_wpm_avg;
    int32_t prevstate, noisecancel_change, sample_counter, startpos, progress, initializing, processed, training_interval;
    int32_t snd_rate, slowdown, started, pad0, pad1;       // snd_rate: the global of :59; started: the host's (the task tap)
    uint32_t sig[SIG_BUFSIZE];
    uint32_t data[DATA_BUFSIZE];
    float raw[GBLK];                                        // raw_signal_buffer (:128), the 88 entries that are used
};

struct ev_t { int32_t blk, gblk, kind, a, b, c; };
struct sink_t {
    ev_t *out;
    int32_t n, cap, overflow, blk, gblk;
};

KG_NR_HD void emit(sink_t &k, int kind, int32_t a, int32_t b, int32_t c)
{
    if (k.n >= k.cap) { k.overflow = 1; return; }
    ev_t &e = k.out[k.n++];
    e.blk = k.blk; e.gblk = k.gblk; e.kind = kind; e.a = a; e.b = b; e.c = c;
}
KG_NR_HD int32_t f_bits(float f) { int32_t i; memcpy(&i, &f, 4); return i; }
// float -> int32 as cvttss2si gives it
KG_NR_HD int32_t cvt_i32(float x) { return (x >= -2147483648.0f && x < 2147483648.0f) ? (int32_t) x : (int32_t) 0x80000000u; }
KG_NR_HD uint32_t sig_time(uint32_t v) { return v >> 1; }
KG_NR_HD int32_t sig_state(uint32_t v) { return (int32_t) (v & 1u); }
KG_NR_HD uint32_t sig_make(int32_t state, uint32_t time) { return (uint32_t) (state & 1) | (time << 1); }
KG_NR_HD int32_t ring_inc(int32_t v) { return (v + 1) == SIG_BUFSIZE ? 0 : v + 1; }                // ring_idx_increment (:417)
KG_NR_HD int32_t ring_dec(int32_t v) { return v == 0 ? SIG_BUFSIZE - 1 : v - 1; }                  // ring_idx_decrement (:418)
KG_NR_HD int32_t ring_change(int32_t v, int32_t change)                                            // ring_idx_change (:411-415)
{
    const int32_t w = v + change;
    return change > 0 ? (w >= SIG_BUFSIZE ? w - SIG_BUFSIZE : w) : (w < 0 ? w + SIG_BUFSIZE : w);
}
KG_NR_HD int32_t one_second(const state_t &s) { return s.snd_rate / s.blocksize; }                // :59

// ---- the code table (:189-248): {what CharacterIdFunc returns, the elements as pairs of bits, dit 10 and dah 11, first element highest}
KG_NR_HD uint8_t character_id(uint32_t code)                                                       // :278-294
{
    static constexpr uint16_t tab[N_CODE][2] = {
        {0, 0xbb}, {1, 0x2ee}, {2, 0x2ea}, {3, 0x3abb}, {4, 0x3ab}, {5, 0xeeba}, {6, 0x3bb}, {7, 0xaaaa}, {8, 0x3be}, {9, 0xebf}, {10, 0xabb}, {11, 0x2ae},
        // aa .-.-   ar .-.-.   as .-...   bk -...-.-   bt -...-   cl -.-..-..   ct -.-.-   hh ........   kn -.--.   nj -..---   sk ...-.-   sn ...-.
        {'E', 0x2}, {'T', 0x3}, {'I', 0xa}, {'A', 0xb}, {'N', 0xe}, {'M', 0xf}, {'S', 0x2a}, {'U', 0x2b}, {'R', 0x2e}, {'W', 0x2f}, {'D', 0x3a}, {'K', 0x3b},
        {'G', 0x3e}, {'O', 0x3f}, {'H', 0xaa}, {'V', 0xab}, {'F', 0xae}, {'L', 0xba}, {'P', 0xbe}, {'J', 0xbf}, {'B', 0xea}, {'X', 0xeb}, {'C', 0xee}, {'Y', 0xef},
        {'Z', 0xfa}, {'Q', 0xfb}, {'5', 0x2aa}, {'4', 0x2ab}, {'3', 0x2af}, {'2', 0x2bf}, {'1', 0x2ff}, {'6', 0x3aa}, {'=', 0x3ab}, {'/', 0x3ae}, {'7', 0x3ea},
        {'8', 0x3fa}, {'9', 0x3fe}, {'0', 0x3ff}, {'?', 0xafa}, {'"', 0xbae}, {'.', 0xbbb}, {'@', 0xbee}, {'\'', 0xbfe}, {'-', 0xeab}, {',', 0xfaf}, {':', 0xfea}};
    if (code == 0) return 0xfe;
    for (int i = 0; i < N_CODE; i++)
        if (code == tab[i][1]) return (uint8_t) tab[i][0];
    return 0xff;
}

// ---- the commands
// g->a of :299 for a receiver rate and a pboff
KG_NR_HD int32_t pboff_a(float sampling_freq, uint32_t pboff)
{
    const float freq = (float) pboff;
    const double a = 0.5 + (double) ((freq * 1.0f) * (float) (uint32_t) GBLK / sampling_freq);
    return (a >= -2147483648.0 && a < 2147483648.0) ? (int32_t) a : (int32_t) 0x80000000u;
}
KG_NR_HD int start_check(int training_interval, double nom_rate, double srate)
{
    if (!(training_interval >= 1 && training_interval <= SIG_BUFSIZE - 1)) return REFUSED_INTERVAL;
    if (!(nom_rate >= (double) GBLK && nom_rate <= 1e6)) return REFUSED_RATE;
    if (!(srate > 0 && srate >= nom_rate / 2 && srate <= nom_rate * 2)) return REFUSED_RATE;          // a NaN fails every comparison
    return 0;
}
KG_NR_HD int pboff_check(float sampling_freq, int32_t blocksize, uint32_t pboff)
{
    if (blocksize == 0) return REFUSED_NOT_STARTED;
    const int32_t a = pboff_a(sampling_freq, pboff);
    return (a >= 0 && a <= blocksize / 2) ? 0 : REFUSED_PBOFF;
}
// CwDecode_Init (:345-392); slowdown, snd_rate and started are not the struct's
KG_NR_HD void cmd_init(state_t &s, int wpm, int training_interval, int32_t snd_rate, double srate)
{
    const int32_t slowdown = s.slowdown, started = s.started;
    memset(&s, 0, sizeof s);
    s.slowdown = slowdown; s.started = started; s.snd_rate = snd_rate;
    s.wsc = 1;
    s.old_siglevel = (float) 0.001;
    s.timer_stepsize = 1;
    s.sampling_freq = (float) srate;
    s.blocksize = GBLK;
    if (wpm != 0) {
        s.speed_wpm_avg = (float) wpm;
        const float blk_per_ms = (float) ((double) s.sampling_freq / 1e3 / GBLK);
        const float ms_per_elem = (float) (60000.0 / (double) ((float) wpm * 50));
        s.dot_avg = blk_per_ms * ms_per_elem;
        s.dash_avg = s.dot_avg * 3;
        s.cwspace_avg = (float) ((double) s.dot_avg * 4.2);
        s.symspace_avg = (float) ((double) s.dot_avg * 0.93);
        s.pulse_avg = (float) ((double) (s.dot_avg / 4 + s.dash_avg) / 2.0);
        s.track = 0;
        s.initialized = 1;
        s.initializing = 0;
    } else {
        s.training_interval = training_interval;
        s.track = 1;
    }
}
KG_NR_HD void cmd_pboff(state_t &s, uint32_t pboff)                                                // :296-305, :394-402
{
    s.g_a = pboff_a(s.sampling_freq, pboff);
    s.g_b = (float) ((2 * KG_CW_PI * s.g_a) / (uint32_t) s.blocksize);
    s.g_sin = KG_CW_SINF(s.g_b);
    s.g_cos = KG_CW_COSF(s.g_b);
    s.g_r = (float) (2.0 * (double) s.g_cos);
    s.process_samples = 1;
}
KG_NR_HD void cmd_wsc(state_t &s, int wsc) { s.wsc = wsc; }
KG_NR_HD void cmd_auto_threshold(state_t &s, int on)                                               // :1030-1035
{
    s.isAutoThreshold = on ? 1 : 0;
    if (s.isAutoThreshold) { s.weight_linear = AUTO_WEIGHT_LINEAR; s.threshold_linear = AUTO_THRESHOLD_LINEAR; }
}
KG_NR_HD void cmd_threshold(state_t &s, int param) { s.threshold_linear = (uint32_t) param; }     // :1038

// ---- one Goertzel block (:307-325, :433-442): sample(i), i = 0 .. 87, gives raw_signal_buffer[i]
template <class F>
KG_NR_HD float goertzel_mag(float r, float cosv, float sinv, F sample)
{
    float b1 = 0, b2 = 0;
    for (int i = 0; i < GBLK; i++) {
        const float b0 = r * b1 - b2 + sample(i);
        b2 = b1;
        b1 = b0;
    }
    const float re = b1 - (b2 * cosv);
    const float im = b2 * sinv;
    const float mag_sq = re * re + im * im;
    return sqrtf(mag_sq);
}
KG_NR_HD float sample_in(int16_t v) { return (float) v / 4; }                                      // :617

KG_NR_HD float decayavg(float average, float input, int weight)                                    // :327-339
{
    if (weight <= 1) return input;
    return ((input - average) / (float) weight) + average;
}

// ---- cw_train (:646-732)
KG_NR_HD void cw_train(state_t &s, sink_t &k)
{
    if (!s.initializing) {
        s.startpos = (int16_t) s.sig_outcount;
        s.progress = (int16_t) s.sig_outcount;
        s.initializing = 1;
        s.pulse_avg = 0; s.dot_avg = 0; s.dash_avg = 0; s.symspace_avg = 0; s.cwspace_avg = 0;
        s.w_space = 0;
    }
    if (!s.track) return;
    const int16_t processed = (int16_t) (s.progress < s.startpos ? (SIG_BUFSIZE + s.progress) - s.startpos : s.progress - s.startpos);
    emit(k, EV_TRAIN, processed >= s.training_interval ? 0 : processed, 0, 0);
    if (processed >= s.training_interval) { s.initialized = 1; s.initializing = 0; }
    if (s.progress != s.sig_incount) {
        const float t = (float) sig_time(s.sig[s.progress]);
        if (sig_state(s.sig[s.progress])) {
            if (processed > TRAINING_STABLE) {
                if (t > s.pulse_avg) s.dash_avg = (float) ((double) s.dash_avg + (double) (t - s.dash_avg) / 4.0);
                else s.dot_avg = (float) ((double) s.dot_avg + (double) (t - s.dot_avg) / 4.0);
            } else {
                if (t > s.pulse_avg) s.dash_avg = (float) ((double) (t + s.dash_avg) / 2.0);
                else s.dot_avg = (float) ((double) (t + s.dot_avg) / 2.0);
            }
            s.pulse_avg = (float) ((double) (s.dot_avg / 4 + s.dash_avg) / 2.0);
        } else if (processed > TRAINING_STABLE) {
            if (t > s.pulse_avg) s.cwspace_avg = (float) ((double) s.cwspace_avg + (double) (t - s.cwspace_avg) / 4.0);
            else s.symspace_avg = (float) ((double) s.symspace_avg + (double) (t - s.symspace_avg) / 4.0);
        }
        s.progress = (int16_t) ring_inc(s.progress);
    }
}

// the time of data[data_len - 1] (:862, :874); DEFINED 3 for data_len == 0
KG_NR_HD uint32_t last_time(const state_t &s) { return s.data_len > 0 ? sig_time(s.data[s.data_len - 1]) : ((uint32_t) s.sig_timer >> 1); }

// ---- cw_DataRecognition (:797-938)
KG_NR_HD bool data_recognition(state_t &s, bool *new_char_p)
{
    bool not_done = false;
    *new_char_p = false;
    if (s.sig_outcount != s.sig_incount) {
        not_done = true;
        s.timeout = 0;
        const float t = (float) sig_time(s.sig[s.sig_outcount]);
        if (t > 0) {
            const bool is_markstate = sig_state(s.sig[s.sig_outcount]) != 0;
            s.sig_outcount = ring_inc(s.sig_outcount);
            if (is_markstate) {
                s.processed = 0;
                int32_t st;
                if ((s.pulse_avg - t) >= 0) {
                    s.dash = 0;
                    st = 0;
                    if (s.track) s.dot_avg = (float) ((double) s.dot_avg + (double) (t - s.dot_avg) / 8.0);
                } else {
                    s.dash = 1;
                    st = 1;
                    if (t <= 5 * s.dash_avg) {
                        if (s.track) s.dash_avg = (float) ((double) s.dash_avg + (double) (t - s.dash_avg) / 8.0);
                    }
                }
                s.data[s.data_len] = sig_make(st, (uint32_t) t & 0x7fffffffu);
                s.data_len = (s.data_len + 1) & 0xff;
                if (s.track) s.pulse_avg = (float) ((double) (s.dot_avg / 4 + s.dash_avg) / 2.0);
            } else {
                bool full_char_detected = true;
                if (s.dash) {
                    s.dash = 0;
                    const float eq4_12 = (float) ((double) t - ((double) s.pulse_avg - (double) ((float) last_time(s) - s.pulse_avg) / 4.0));
                    if (eq4_12 < 0) {
                        if (s.track) s.symspace_avg = (float) ((double) s.symspace_avg + (double) (t - s.symspace_avg) / 8.0);
                        full_char_detected = false;
                    } else if (t <= 10 * s.dash_avg) {
                        const float eq4_14 = (float) ((double) t - ((double) s.cwspace_avg - (double) ((float) last_time(s) - s.pulse_avg) / 4.0));
                        if (eq4_14 >= 0) {
                            s.w_space = (int32_t) t;
                            s.wspace = 1;
                        }
                    }
                } else {
                    if ((t - s.pulse_avg) < 0) {
                        if (s.track) s.symspace_avg = (float) ((double) s.symspace_avg + (double) (t - s.symspace_avg) / 8.0);
                        full_char_detected = false;
                    } else if (t <= 10 * s.dash_avg) {
                        if (s.track) s.cwspace_avg = (float) ((double) s.cwspace_avg + (double) (t - s.cwspace_avg) / 8.0);
                        if ((t - s.cwspace_avg) >= 0) {
                            s.w_space = (int32_t) t;
                            s.wspace = 1;
                        }
                    }
                }
                if (full_char_detected && !s.processed) *new_char_p = true;
            }
        }
    } else if ((float) s.cur_time > (10 * s.dash_avg)) {
        if (sig_state(s.sig[s.sig_incount]) == 0 && !s.processed) {
            s.processed = 1;
            s.wspace = 1;
            s.timeout = 1;
            *new_char_p = true;
        }
    }
    if (s.data_len > DATA_BUFSIZE - 2) s.data_len = DATA_BUFSIZE - 2;
    if (*new_char_p) {
        s.last_outcount = s.cur_outcount;
        s.cur_outcount = s.sig_outcount;
    }
    return not_done;
}

KG_NR_HD void code_gen(state_t &s)                                                                 // :946-957
{
    s.code = 0;
    for (int a = 0; a < s.data_len; a++) {
        s.code <<= 2;
        s.code |= sig_state(s.data[a]) ? DAH : DIT;
    }
    s.data_len = 0;
}

KG_NR_HD void print_char(state_t &s, uint8_t c, uint32_t now_sec, sink_t &k)                      // :964-988
{
    emit(k, EV_CHARS, c >= 0x7f ? 0xff : c, 0, 0);
    const uint32_t now = now_sec / 4;
    if (s.wpm_update != now) {
        emit(k, EV_WPM, s.speed, 0, 0);
        s.wpm_update = now;
    }
}

KG_NR_HD void word_space(state_t &s, uint8_t c, sink_t &k)                                         // :998-1018
{
    if (!s.wspace) return;
    s.wspace = 0;
    if (s.wsc && ((c == 'I') || (c == 'J') || (c == 'Q') || (c == 'U') || (c == 'V') || (c == 'Z'))) {
        const int16_t x = (int16_t) cvt_i32((s.cwspace_avg + s.pulse_avg) - (float) s.w_space);  // DEFINED 2
        if (x < 0) emit(k, EV_CHARS, ' ', 0, 0);
    } else emit(k, EV_CHARS, ' ', 0, 0);
}

// ---- ErrorCorrectionFunc (:1058-1228)
KG_NR_HD bool error_correction(state_t &s, uint32_t now_sec, sink_t &k)
{
    bool result = false;
    if (s.data_len >= DATA_BUFSIZE - 2) {
        print_char(s, 0xff, now_sec, k);
        word_space(s, 0xff, k);
        return result;
    }
    s.wspace = 0;
    int32_t temp_outcount = s.last_outcount, slocation = s.last_outcount, plocation = s.last_outcount;
    uint32_t pduration = 0xffffffffu, sduration = 0;
    while (temp_outcount != s.cur_outcount) {
        const uint32_t v = s.sig[temp_outcount];
        if (sig_state(v)) {
            if (sig_time(v) < pduration) { pduration = sig_time(v); plocation = temp_outcount; }
        }
        if ((temp_outcount != s.last_outcount) && (temp_outcount != (s.cur_outcount - 1)) && !sig_state(v)) {
            if (sig_time(v) > sduration) { sduration = sig_time(v); slocation = temp_outcount; }
        }
        temp_outcount = ring_inc(temp_outcount);
    }
    uint8_t decoded[2] = {0xff, 0xff};
    bool dummy;
    int i;
    if (((float) pduration < s.dot_avg / 2) && (plocation != temp_outcount)) {
        const int32_t after = ring_change(plocation, +1), before = ring_change(plocation, -1);
        const uint32_t sum = (sig_time(s.sig[before]) + sig_time(s.sig[plocation]) + sig_time(s.sig[after])) & 0x7fffffffu;
        s.sig[after] = sig_make(sig_state(s.sig[after]), sum);
        temp_outcount = ring_change(plocation, -2);
        while (temp_outcount != s.last_outcount) {
            s.sig[ring_change(temp_outcount, +2)] = s.sig[temp_outcount];
            temp_outcount = ring_dec(temp_outcount);
        }
        s.sig_outcount = ring_change(s.last_outcount, +2);
        for (i = 0; i < 1024 && data_recognition(s, &dummy); i++) {}
        code_gen(s);
        decoded[0] = character_id(s.code);
        if (decoded[0] < 0xfe) {
            print_char(s, decoded[0], now_sec, k);
            result = true;
        } else print_char(s, 0xff, now_sec, k);
    } else {
        const float split = (s.cwspace_avg - 1) >= 1 ? s.cwspace_avg - 1 : 1;
        s.sig[slocation] = sig_make(sig_state(s.sig[slocation]), (uint32_t) split & 0x7fffffffu);
        s.sig_outcount = s.last_outcount;
        for (i = 0; i < 1024 && data_recognition(s, &dummy); i++) {}
        code_gen(s);
        decoded[0] = character_id(s.code);
        for (i = 0; i < 1024 && data_recognition(s, &dummy); i++) {}
        code_gen(s);
        decoded[1] = character_id(s.code);
        if ((decoded[0] < 0xfe) && (decoded[1] < 0xfe)) {
            print_char(s, decoded[0], now_sec, k);
            print_char(s, decoded[1], now_sec, k);
            result = true;
        } else print_char(s, 0xff, now_sec, k);
    }
    return result;
}

// ---- CW_Decode (:1241-1296)
KG_NR_HD void cw_decode(state_t &s, uint32_t now_sec, sink_t &k)
{
    if (!s.initialized) cw_train(s, k);
    if (s.initialized || (s.cur_time >= one_second(s) * CW_TIMEOUT)) {
        bool received;
        data_recognition(s, &received);
        if (received && (s.data_len > 0)) {
            code_gen(s);
            const uint8_t decoded = character_id(s.code);
            if (decoded < 0xfe) {
                print_char(s, decoded, now_sec, k);
                word_space(s, decoded, k);
            } else if (decoded == 0xff) {
                if (!error_correction(s, now_sec, k) && s.track) {
                    s.err_cnt++;
                    s.err_timeout = (int32_t) (now_sec + ERROR_TIMEOUT);
                    emit(k, EV_TRAIN, -(s.err_cnt), 0, 0);
                    if (s.err_cnt > 3) {
                        s.initialized = 0;
                        s.err_cnt = 0;
                        s.err_timeout = 0;
                    }
                }
            }
            if (s.track && s.err_timeout && now_sec >= (uint32_t) s.err_timeout) {
                s.err_cnt = 0;
                s.err_timeout = 0;
                emit(k, EV_TRAIN, 0, 0, 0);
            }
        }
    }
}

// ---- CW_Decode_exe (:423-607) behind the Goertzel: mag is what AudioFilter_GoertzelEnergy returned
KG_NR_HD void exe(state_t &s, float mag, uint32_t now_sec, sink_t &k)
{
    bool newstate;
    float siglevel = mag;
    if (s.isAutoThreshold) {
        s.CW_mag = siglevel;
        s.CW_env = decayavg(s.CW_env, s.CW_mag, (s.CW_mag > s.CW_env) ? (int) (s.weight_linear / 1000 / 4) : (int) (s.weight_linear / 1000 * 16));
        s.CW_noise = decayavg(s.CW_noise, s.CW_mag, (s.CW_mag < s.CW_noise) ? (int) (s.weight_linear / 1000 / 4) : (int) (s.weight_linear / 1000 * 48));
        const float clipped = (s.CW_env < s.CW_noise) ? s.CW_noise : ((s.CW_env > s.CW_mag) ? s.CW_mag : s.CW_env);
        const float env_to_noise = clipped - s.CW_noise;
        float v1 = (float) ((double) ((clipped - s.CW_noise) * env_to_noise) - 0.8 * (double) (env_to_noise * env_to_noise));
        v1 = sqrtf(fabsf(v1)) * (float) ((v1 < 0) ? -1 : 1);
        siglevel = (float) ((double) v1 * KG_CW_SIGNAL_TAU + (1.0 - KG_CW_SIGNAL_TAU) * (double) s.old_siglevel);
        s.old_siglevel = v1;
        newstate = siglevel >= (float) s.threshold_linear;
    } else {
        siglevel = (float) ((double) siglevel * KG_CW_SIGNAL_TAU + (1.0 - KG_CW_SIGNAL_TAU) * (double) s.old_siglevel);
        s.old_siglevel = mag;
        newstate = siglevel >= (float) s.threshold_linear;
    }
    if (s.noisecancel_change) {                                        // noisecancel_enable is 1 (:359)
        s.state = newstate ? 1 : 0;
        s.noisecancel_change = 0;
    } else if ((newstate ? 1 : 0) != s.state) s.noisecancel_change = 1;
    if (s.slowdown++ == 2) {                                           // :519-528, DEFINED 1
        const float sig = s.isAutoThreshold ? fabsf(siglevel) : siglevel;
        float dB = (float) (10.0 * (double) KG_CW_LOG10F((float) ((double) sig + 1e-30)));
        dB = (float) ((dB < 0) ? 0.0 : ((dB > 100.0) ? 100.0 : (double) dB));
        const float threshold_log = (float) (10.0 * (double) KG_CW_LOG10F((float) s.threshold_linear));
        emit(k, EV_PLOT, f_bits(dB), siglevel >= 0 ? 1 : 0, f_bits(threshold_log));
        s.slowdown = 0;
    }
    if (s.state != s.prevstate) {
        s.sig[s.sig_lastrx] = sig_make(s.prevstate, (uint32_t) s.sig_timer & 0x7fffffffu);
        s.sig_lastrx = ring_inc(s.sig_lastrx);
        s.sig_timer = 0;
        s.prevstate = s.state;
    }
    s.sig_timer = s.sig_timer + s.timer_stepsize;
    if (s.sig_timer > one_second(s) * CW_TIMEOUT) s.sig_timer = one_second(s) * CW_TIMEOUT;
    s.sig_incount = s.sig_lastrx;
    s.cur_time = s.sig_timer;
    cw_decode(s, now_sec, k);
    const float spdcalc = (float) (10.0 * (double) s.dot_avg + 4.0 * (double) s.dash_avg + 9.0 * (double) s.symspace_avg + 5.0 * (double) s.cwspace_avg);
    if (s.initialized && spdcalc > 0) {
        const float speed_ms_per_word = (float) ((double) spdcalc * 1000.0 / (double) (s.sampling_freq / (float) (uint8_t) s.blocksize));
        const float speed_wpm_raw = (float) (0.5 + 60000.0 / (double) speed_ms_per_word);
        s.speed_wpm_avg = (float) ((double) speed_wpm_raw * 0.3 + 0.7 * (double) s.speed_wpm_avg);
    } else s.speed_wpm_avg = 0;
    s.speed = cvt_i32(s.speed_wpm_avg) & 0xff;                         // DEFINED 2
}

// Goertzel blocks that a stretch of n samples completes behind sample_counter sc, and what it leaves
KG_NR_HD int32_t gblocks(int32_t sc, int32_t n) { return (sc + n) / GBLK; }
KG_NR_HD int32_t max_events(int32_t nblk) { return EVENTS_PER_GBLK * ((BLK * nblk + GBLK - 1) / GBLK); }

// CwDecode_RxProcessor (:609-625) for one sound block, the host's way: sample by sample
inline void host_block(state_t &s, const int16_t *x, uint32_t now_sec, sink_t &k)
{
    if (!s.started || !s.process_samples) return;
    k.gblk = 0;
    for (int i = 0; i < BLK; i++) {
        s.raw[s.sample_counter] = sample_in(x[i]);
        s.sample_counter++;
        if (s.sample_counter >= s.blocksize) {
            const float *raw = s.raw;
            const float mag = goertzel_mag(s.g_r, s.g_cos, s.g_sin, [raw](int j) { return raw[j]; });
            exe(s, mag, now_sec, k);
            s.sample_counter = 0;
            k.gblk++;
        }
    }
}

}  // namespace kg_cw_cf
#endif
