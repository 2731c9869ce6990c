// kg_fax.h -- the HF weather fax extension (extensions/FAX/FaxDecoder.cpp, FaxDecoder.h; fax.cpp for the commands), the consumer of
// receive_real_samps: the 16-bit mono audio a sound block ends as (rx/rx_sound.cpp:1100-1111).  On the device AND the host, in the
// reference's own operand types (TYPEREAL is float); library, host driver and golden are built with -ffp-contract=off.  What lives here:
//   * Configure (:467-515) with reset, SetupBuffers (:517-541), InitializeImage (:449-465): cmd_start.  ALL parameters of Configure,
//     not only what fax.cpp:131-145 passes.  m_SamplesPerLine = (int) (nom * 60.0 / lpm), m_lineIncrFrac = imagewidth / (M_PI * 576),
//     m_bSkipHeaderDetection = !(phasing || autostop); 300 / 450 Hz, m_StartStopLength 5, m_phasingLines 40.  An object begins zeroed
//     (the static m_FaxDecoder[]).  NOT reset by a later Configure, so carried over a restart: Iprev, Qprev, m_lineBlend, m_skip,
//     m_SamplesPerSec_frac_prev.  What `new` and kiwi_imalloc hand out (m_samples, m_demod_data, phasingPos, m_imgdata, m_outImage) is
//     DEFINED here as zeros; the golden harness zero-fills its allocators to match.
//   * ProcessSamples (:410-447), per block of FASTFIR_OUTBUF_SIZE = 512 samples: walk_block.  m_skip = shift * m_SamplesPerLine (float
//     times int, truncated), the skip off the front of the block, the pick i = trunc(m_fi) behind m_fi += m_SampleRateRatio in double,
//     m_fi -= nsamps with the REDUCED nsamps.  Block boundaries are part of the result.
//   * DemodulateData (:285-334) with UpdateSampleRate (:92-97) and apply_firfilter (:56-90): line_begin, mix, fir17, normalise,
//     pixel_of.  f restarts at 0 on every line, f += ph_inc; if (f > 1.0) f -= 1.0 in double; the 17 taps as sum = 0; sum += c[k] *
//     x[n - k], k = 0 .. 16; the last products are carried across lines although f restarts.  The reference's circular buffer is kept
//     as a linear history (hist[k] = x[n - 1 - k]) and a count modulo 17; fir_circular() gives the reference's layout back.  mag == 0
//     (silence; the first samples behind a Configure) makes x NaN and the reference's int conversion undefined: byte 0 HERE, by an
//     explicit test (x86-64 gives the same); Iprev / Qprev then hold the NaN for a sample, as in the reference.
//   * DetectLineType / FourierTransformSub (:100-129) over min(spl, 3000) bytes: fourier_k, fourier_term, detect_type.  Each of the four
//     sums is a serial float chain in index order.
//   * the typecount / lasttype machine (:178-222): machine_pre.  typecount == 5 * lpm / 60.0 - 4 is a double comparison (never at 90 lpm).
//   * FaxPhasingLinePosition (:136-160): wedge_total, phasing_result; integers, the first minimum wins.
//   * the phasing countdown (:226-245) with median_i (support/misc.cpp:90-96; 38 ints sorted IN PLACE): machine_post.
//   * DecodeImageLine (:341-408): pixel_avg, blend_decide, blend_pixel.  Only the previous line of m_imgdata is ever read: two lines are
//     kept, not the image.  Under autostop a line is counted and not decoded; the reference then blends the next decoded line with
//     malloc's leftovers.  HERE that previous line is zeros.  A row is FAX_MSG_DRAW (254), then imagewidth bytes.
//   * the tail of DecodeFaxLine (:267-280): machine_tail.
// REFUSED, nothing changed (the reference leaves them undefined): lpm < 1; deviation == 0; a bandwidth outside 0 .. 2; imagewidth < 1;
// SamplesPerLine < imagewidth (sampsIncr is 0: the phasing loop never ends); SamplesPerLine > MAX_SPL = 24576 (ours: 60 lpm at 20250 Hz
// is 20250; spl * imagewidth stays an int); a nominal rate outside 1 .. 1e6 Hz; a sample rate outside nom / 2 .. 2 nom (ours: it bounds
// the lines of a push); a shift that is negative, above 1 or not finite (a negative skip walks the sample pointer backwards).
// NOT ported: the pgm file (FileOpen / FileWrite / FileClose, fax_record_line), the shell commands of fax.cpp, fax_task's sequence numbers.
#ifndef KG_FAX_H
#define KG_FAX_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "kg_nr.h"
#if defined(__HIPCC__)
#include "kg_libm_trig.h"
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KG_FAX_SINF(x) kg_libm::sinf_glibc(x)           // the host libm's, bit for bit (kg_libm_trig.h)
#define KG_FAX_COSF(x) kg_libm::cosf_glibc(x)
#else
#define KG_FAX_SINF(x) sinf(x)
#define KG_FAX_COSF(x) cosf(x)
#endif

namespace kg_fax_cf {

enum { BLK = 512, TAPS = 17, PHASING_LINES = 40, PHASING_SKIP = 2, NPOS = 38, START_STOP_LEN = 5, DET_CAP = 3000, MAX_SPL = 24576, MSG_DRAW = 254 };
enum { START_HZ = 300, STOP_HZ = 450, LEEWAY = 4, PIXEL_RESOLUTION = 4 };
enum { IMAGE = 0, START = 1, STOP = 2 };                                                          // FaxDecoder.h:102
enum { F_SPS_CHANGED = 1, F_AUTOSTOPPED_0 = 2, F_AUTOSTOPPED_1 = 4, F_PHASED = 8, F_ROW_SENT = 16, F_PHASING_REJECTED = 32, F_MEDIAN = 64 };
enum { REFUSED_LPM = -1, REFUSED_DEVIATION = -2, REFUSED_BANDWIDTH = -3, REFUSED_WIDTH = -4, REFUSED_SPL_WIDTH = -5, REFUSED_SPL_MAX = -6,
       REFUSED_RATE = -7, REFUSED_SHIFT = -8 };
#define KG_FAX_2PI (2.0 * 3.14159265358979323846)                                                  /* K_2PI, datatypes.h:103 */
#define KG_FAX_PI 3.14159265358979323846                                                           /* M_PI */

// the scalars of a FaxDecoder (FaxDecoder.h:72-137) that the port keeps
struct state_t {
    double nom, frac, frac_prev, ratio, fi, lineIncrFrac, lineIncrAcc, lineBlend, carrier, deviation;
    int32_t lpm, imagewidth, bandwidth, include_headers, use_phasing, autostop, autostopped, debug, skip_header_detection, spl;
    int32_t skip, samp_idx, lasttype, typecount, imageline, phasingLinesLeft, phasingSkipData, have_phasing, fir_count, pad;
    float Iprev, Qprev;
    float hist[2][TAPS];                        // hist[f][k]: the product k + 1 samples back (I: f = 0, Q: f = 1)
    int32_t phasingPos[PHASING_LINES];
};

// one completed line, as it stands behind DecodeFaxLine (:437)
struct rec_t {
    int32_t blk, off;                           // the block of the push and i of :431 (counted from behind the skip) at which it completed
    int32_t type, typecount, imageline, phasingLinesLeft, skip;
    int32_t phasing_pos;                        // what FaxPhasingLinePosition gave for this line, or -1
    int32_t flags;
    int32_t phasingSkipData, ten_pct, ninety_pct;      // under F_MEDIAN: what :239 prints
};

// ---- the arithmetic of one sample (:311-331)
KG_NR_HD float fir_coeff(int bw, int k)                                                           // :61-65
{
    static constexpr float c[3][TAPS] = {{-7, -18, -15, 11, 56, 116, 177, 223, 240, 223, 177, 116, 56, 11, -15, -18, -7},
                                         {0, -18, -38, -39, 0, 83, 191, 284, 320, 284, 191, 83, 0, -39, -38, -18, 0},
                                         {6, 20, 7, -42, -74, -12, 159, 353, 440, 353, 159, -12, -74, -42, 7, 20, 6}};
    return c[bw][k];
}
KG_NR_HD float mix_angle(double f) { return (float) (KG_FAX_2PI * f); }
KG_NR_HD double next_f(double f, double ph_inc)                                                   // :317-318
{
    f += ph_inc;
    if (f > 1.0) f -= 1.0;
    return f;
}
KG_NR_HD void mix(int16_t s, float ang, float *xi, float *xq)                                     // :312-315
{
    const float samp = s * (1.0f / 32768.0f);
    *xi = samp * KG_FAX_COSF(ang);
    *xq = samp * KG_FAX_SINF(ang);
}
// x points at the newest product; x[-k] is k samples back
KG_NR_HD float fir17(int bw, const float *x)
{
    float sum = 0;
    for (int k = 0; k < TAPS; k++) sum += x[-k] * fir_coeff(bw, k);
    return sum;
}
KG_NR_HD void normalise(float *I, float *Q)                                                       // :320-322
{
    const float mag = sqrtf(*Q * *Q + *I * *I);
    *I /= mag;
    *Q /= mag;
}
KG_NR_HD float demod_scale(double nom, double deviation) { return (float) (-1.3 * (nom / deviation / 8)); }      // :303
KG_NR_HD uint8_t pixel_of(float I, float Q, float Iprev, float Qprev, float scale)                // :324-328
{
    float x = (I * (Q - Qprev) - Q * (I - Iprev)) * scale;
    x = (float) (x / 2.0 + 0.5);
    const double v = x * 255.0;
    if (!(v == v)) return 0;                                                                      // NaN: defined here
    return (uint8_t) (v < 0 ? 0 : v > 255 ? 255 : (int) v);
}

// ---- the line's type (:100-129)
KG_NR_HD float fourier_k(int freq, int lpm, int spl) { return (float) (-2 * KG_FAX_PI * freq * 60.0 / lpm / spl); }
KG_NR_HD float fourier_term(uint8_t b, float k, int n, int sine) { return sine ? b * KG_FAX_SINF(k * n) : b * KG_FAX_COSF(k * n); }
KG_NR_HD float fourier_det(float retr, float reti, int len) { return sqrtf(retr * retr + reti * reti) / len; }
KG_NR_HD int detect_type(float start_det, float stop_det) { return start_det > 5 ? START : stop_det > 5 ? STOP : IMAGE; }
KG_NR_HD int det_len(int spl) { return spl < DET_CAP ? spl : DET_CAP; }

// ---- the phasing position (:136-160)
KG_NR_HD int wedge_n(int spl) { return (int) (spl * .07); }
KG_NR_HD int wedge_incr(int spl, int w) { return spl / w * PIXEL_RESOLUTION; }
KG_NR_HD int wedge_total(const uint8_t *image, int spl, int n, int i)
{
    int total = 0;
    for (int j = 0; j < n; j += PIXEL_RESOLUTION) {
        const int d = j - n / 2;
        total += (n / 2 - (d < 0 ? -d : d)) * (255 - image[(i + j) % spl]);
    }
    return total;
}
KG_NR_HD int phasing_result(int min, int n, int spl) { return spl ? ((min + n / 2) % spl) : 0; }

// ---- a pixel of the image line (:356-370) and of the blended row (:388-390)
KG_NR_HD uint8_t pixel_avg(const uint8_t *buffer, int spl, int w, int i)
{
    const int firstsample = spl * i / w, lastsample = spl * (i + 1) / w - 1;
    int pixelSamples = 0, sample = firstsample, pixel = 0;
    do {
        pixel += buffer[sample];
        pixelSamples++;
    } while (sample++ < lastsample);
    return (uint8_t) (pixel / pixelSamples);
}
KG_NR_HD uint8_t blend_pixel(uint8_t image, uint8_t prev, double next, double prevBlend)
{
    int pixel = (int) roundf((float) ((float) image * next + (float) prev * prevBlend));
    if (pixel > 255) pixel = 255;
    return (uint8_t) pixel;
}

// ---- the scalar walk of DecodeFaxLine, in the reference's order.  One caller (one lane) runs these; the arrays are the callers'.
// UpdateSampleRate and the head of DemodulateData (:291-303): srate is what ext_update_get_sample_rateHz answers
KG_NR_HD double line_begin(state_t &s, double srate, rec_t &r)
{
    s.frac = srate;
    s.ratio = s.frac / s.nom;
    if (s.frac != s.frac_prev) { r.flags |= F_SPS_CHANGED; s.frac_prev = s.frac; }
    return s.carrier / s.frac;                                                                    // ph_inc
}
// :178-222 -> whether FaxPhasingLinePosition is wanted for this line (:226)
KG_NR_HD bool machine_pre(state_t &s, int type, rec_t &r)
{
    if (type == s.lasttype && type != IMAGE) s.typecount++;
    else {
        s.typecount--;
        if (s.typecount < 0) s.typecount = 0;
    }
    s.lasttype = type;
    if (type != IMAGE && s.typecount == START_STOP_LEN * s.lpm / 60.0 - LEEWAY) {
        if (type == START) {
            if (!s.include_headers) { s.imageline = 0; s.lineIncrAcc = 0; }
            s.phasingLinesLeft = PHASING_LINES;
            s.phasingSkipData = 0;
            s.have_phasing = 0;
            if (s.autostopped) { r.flags |= F_AUTOSTOPPED_0; s.autostopped = 0; }
        } else if (s.autostop) {
            r.flags |= F_AUTOSTOPPED_1;
            s.autostopped = 1;
        }
    }
    return s.use_phasing && s.phasingLinesLeft > 0 && s.phasingLinesLeft <= PHASING_LINES - PHASING_SKIP;
}
KG_NR_HD void sort_ints(int32_t *a, int n)
{
    for (int i = 1; i < n; i++) {
        const int32_t v = a[i];
        int j = i - 1;
        for (; j >= 0 && a[j] > v; j--) a[j + 1] = a[j];
        a[j + 1] = v;
    }
}
// :231-248 -> whether the line is counted into the image
KG_NR_HD bool machine_post(state_t &s, int type, rec_t &r)
{
    if (s.use_phasing && type == IMAGE && s.phasingLinesLeft >= -PHASING_SKIP) {
        if (--s.phasingLinesLeft == 0) {
            sort_ints(s.phasingPos, NPOS);                                                        // median_i, misc.cpp:90-96
            const int ten = s.phasingPos[(int) (NPOS * ((float) 10 / 100.0))], ninety = s.phasingPos[(int) (NPOS * ((float) 90 / 100.0))];
            s.phasingSkipData = s.phasingPos[NPOS / 2];
            r.flags |= F_MEDIAN;
            r.phasingSkipData = s.phasingSkipData; r.ten_pct = ten; r.ninety_pct = ninety;
            if ((ninety - ten) > s.spl / 6) { r.flags |= F_PHASING_REJECTED; s.phasingSkipData = 0; }
        }
    }
    return s.include_headers || !s.use_phasing || (type == IMAGE && s.phasingLinesLeft < -PHASING_SKIP);
}
// :376-399 -> emit; *blend: the row is blended with next / prevBlend (else m_outImage goes out as it stands)
KG_NR_HD bool blend_decide(state_t &s, bool *blend, double *next, double *prevBlend)
{
    *blend = false;
    *next = *prevBlend = 0;
    if (s.debug) return true;
    bool emit = false;
    if (s.lineIncrAcc >= 1.0) {
        s.lineIncrAcc -= 1.0;
        if (s.imageline != 0 && s.lineIncrAcc != 0) {
            *next = s.lineIncrAcc / s.lineBlend;
            *prevBlend = 1.0 - *next;
            *blend = true;
            s.lineBlend = s.lineIncrFrac;
        }
        emit = true;
    } else {
        s.lineBlend += s.lineIncrFrac;
    }
    s.lineIncrAcc += s.lineIncrFrac;
    return emit;
}
// :270-279, the line counted
KG_NR_HD void machine_tail(state_t &s, rec_t &r)
{
    s.phasingSkipData %= s.spl;
    if (s.phasingSkipData && s.use_phasing && !s.have_phasing) {
        s.skip = s.phasingSkipData;
        s.have_phasing = 1;
        r.flags |= F_PHASED;
    }
    s.imageline++;
}
KG_NR_HD void rec_finish(const state_t &s, int type, rec_t &r)
{
    r.type = type; r.typecount = s.typecount; r.imageline = s.imageline; r.phasingLinesLeft = s.phasingLinesLeft; r.skip = s.skip;
}

// ---- ProcessSamples' head (:416-424) for one block -> the reduced nsamps; *front: what came off the front
KG_NR_HD int block_head(state_t &s, float shift, int *front)
{
    int nsamps = BLK;
    *front = 0;
    if (shift) s.skip = (int) (shift * s.spl);
    if (s.skip) {
        const int skip = nsamps < s.skip ? nsamps : s.skip;
        nsamps -= skip;
        *front = skip;
        s.skip -= skip;
    }
    return nsamps;
}

// ---- the commands
inline bool shift_ok(float shift) { return shift >= 0.0f && shift <= 1.0f; }                      // NaN fails both

// what `SET fax_start` is refused for (0: taken); *spl_out: m_SamplesPerLine
inline int start_check(int lpm, int imagewidth, int deviation, int bandwidth, double nom, double srate, int *spl_out)
{
    if (lpm < 1) return REFUSED_LPM;
    if (deviation == 0) return REFUSED_DEVIATION;
    if (bandwidth < 0 || bandwidth > 2) return REFUSED_BANDWIDTH;
    if (imagewidth < 1) return REFUSED_WIDTH;
    if (!(nom >= 1 && nom <= 1e6)) return REFUSED_RATE;
    if (!(srate >= nom / 2 && srate <= nom * 2)) return REFUSED_RATE;
    const double samplesPerMin = nom * 60.0;
    const double spl_d = samplesPerMin / lpm;
    if (!(spl_d < MAX_SPL + 1.0)) return REFUSED_SPL_MAX;
    const int spl = (int) spl_d;
    if (spl < imagewidth) return REFUSED_SPL_WIDTH;
    *spl_out = spl;
    return 0;
}
inline bool rate_ok(const state_t &s, double srate) { return srate >= s.nom / 2 && srate <= s.nom * 2; }

// Configure with reset (:467-515), SetupBuffers, InitializeImage and FreeImage, on the scalars; the caller zeroes the arrays.
// The arguments have passed start_check.
KG_NR_HD void cmd_start(state_t &s, int lpm, int imagewidth, int carrier, int deviation, int bandwidth, int include_headers, int phasing, int autostop, int debug,
                        double nom, double srate)
{
    s.carrier = carrier; s.deviation = deviation;
    s.include_headers = include_headers ? 1 : 0; s.use_phasing = phasing ? 1 : 0; s.autostop = autostop ? 1 : 0;
    s.skip_header_detection = (s.use_phasing || s.autostop) ? 0 : 1;
    s.lpm = lpm;
    s.bandwidth = bandwidth;
    for (int f = 0; f < 2; f++)
        for (int k = 0; k < TAPS; k++) s.hist[f][k] = 0;
    s.fir_count = 0;
    s.frac = srate; s.nom = nom; s.ratio = s.frac / s.nom;                                        // UpdateSampleRate
    const double samplesPerMin = s.nom * 60.0;
    s.spl = (int) (samplesPerMin / s.lpm);
    s.samp_idx = 0;
    s.fi = 0;
    for (int k = 0; k < PHASING_LINES; k++) s.phasingPos[k] = 0;
    s.phasingLinesLeft = s.phasingSkipData = 0;
    s.have_phasing = 0;
    s.imagewidth = imagewidth;
    s.imageline = 0; s.lineIncrAcc = 0;                                                           // FreeImage
    s.lasttype = IMAGE; s.typecount = 0; s.autostopped = 0;                                       // InitializeImage
    s.lineIncrFrac = s.imagewidth / (KG_FAX_PI * 576);
    s.debug = debug;
}

// the reference's circular firfilter::buffer[17] and ::current from the linear history: sample m behind the Configure sits at slot
// (17 - m % 17) % 17 (`current` walks downwards from 0)
inline void fir_circular(const state_t &s, float out[2][TAPS], int32_t *current)
{
    const int count = s.fir_count;                                                                // samples behind the Configure, modulo 17
    for (int f = 0; f < 2; f++)
        for (int k = 0; k < TAPS; k++) {
            const int m = ((count - 1 - k) % TAPS + TAPS) % TAPS;
            out[f][(TAPS - m) % TAPS] = s.hist[f][k];
        }
    *current = (TAPS - count % TAPS) % TAPS;
}

// how many lines a push of nblk blocks can complete at most: a block gives at most BLK / (1/2) + 2 picks (the rate ratio is 1/2 .. 2)
inline int lines_bound(int spl, int nblk) { return (int) (((int64_t) nblk * (2 * BLK + 2) + spl - 1) / spl) + 1; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the whole object on the host, sample by sample as the reference walks it
struct full_t {
    state_t s;
    int32_t started;
    float shift;                                // fax_t::shift (fax.cpp:28): taken by the next block
    int16_t samples[MAX_SPL];
    uint8_t demod[MAX_SPL], prev[MAX_SPL], out[MAX_SPL], image[MAX_SPL];
};
typedef void (*line_t)(void *user, const rec_t *rec, const uint8_t *row, int nbytes);             // row: null unless F_ROW_SENT

inline void full_start(full_t &q, int lpm, int imagewidth, int carrier, int deviation, int bandwidth, int include_headers, int phasing, int autostop, int debug,
                       double nom, double srate)
{
    cmd_start(q.s, lpm, imagewidth, carrier, deviation, bandwidth, include_headers, phasing, autostop, debug, nom, srate);
    memset(q.samples, 0, sizeof q.samples);
    memset(q.demod, 0, sizeof q.demod);
    memset(q.prev, 0, sizeof q.prev);
    memset(q.out, 0, sizeof q.out);
    q.started = 1;
}

inline void full_line(full_t &q, double srate, rec_t &r, line_t on_line, void *user)
{
    state_t &s = q.s;
    const int spl = s.spl, w = s.imagewidth;
    // DemodulateData
    const double ph_inc = line_begin(s, srate, r);
    const float scale = demod_scale(s.nom, s.deviation);
    double f = 0;
    float xi[2 * TAPS], xq[2 * TAPS];                                   // a window: [TAPS - 1] is the newest
    for (int k = 0; k < TAPS; k++) { xi[TAPS - 1 - k] = s.hist[0][k]; xq[TAPS - 1 - k] = s.hist[1][k]; }
    for (int i = 0; i < spl; i++) {
        memmove(xi, xi + 1, sizeof(float) * (TAPS - 1));
        memmove(xq, xq + 1, sizeof(float) * (TAPS - 1));
        mix(q.samples[i], mix_angle(f), &xi[TAPS - 1], &xq[TAPS - 1]);
        float I = fir17(s.bandwidth, &xi[TAPS - 1]), Q = fir17(s.bandwidth, &xq[TAPS - 1]);
        f = next_f(f, ph_inc);
        normalise(&I, &Q);
        q.demod[i] = pixel_of(I, Q, s.Iprev, s.Qprev, scale);
        s.Iprev = I; s.Qprev = Q;
    }
    for (int k = 0; k < TAPS; k++) { s.hist[0][k] = xi[TAPS - 1 - k]; s.hist[1][k] = xq[TAPS - 1 - k]; }
    s.fir_count = (s.fir_count + spl) % TAPS;
    // DetectLineType
    int type = IMAGE;
    if (!s.skip_header_detection) {
        const int len = det_len(spl);
        float det[2];
        for (int t = 0; t < 2; t++) {
            const float k = fourier_k(t ? STOP_HZ : START_HZ, s.lpm, spl);
            float retr = 0, reti = 0;
            for (int n = 0; n < len; n++) { retr += fourier_term(q.demod[n], k, n, 0); reti += fourier_term(q.demod[n], k, n, 1); }
            det[t] = fourier_det(retr, reti, len);
        }
        type = detect_type(det[0], det[1]);
    }
    r.phasing_pos = -1;
    if (machine_pre(s, type, r)) {
        const int n = wedge_n(spl), incr = wedge_incr(spl, w);
        int mintotal = -1, min = 0;
        for (int i = 0; i < spl; i += incr) {
            const int total = wedge_total(q.demod, spl, n, i);
            if (total < mintotal || mintotal == -1) { mintotal = total; min = i; }
        }
        r.phasing_pos = s.phasingPos[s.phasingLinesLeft - 1] = phasing_result(min, n, spl);
    }
    const uint8_t *row = nullptr;
    uint8_t sent[MAX_SPL + 1];
    if (machine_post(s, type, r)) {
        if (!s.autostopped) {
            for (int i = 0; i < w; i++) q.image[i] = pixel_avg(q.demod, spl, w, i);
            bool blend;
            double next, prevBlend;
            if (blend_decide(s, &blend, &next, &prevBlend)) {
                if (blend)
                    for (int i = 0; i < w; i++) q.out[i] = blend_pixel(q.image[i], q.prev[i], next, prevBlend);
                sent[0] = MSG_DRAW;
                memcpy(sent + 1, s.debug ? q.image : q.out, (size_t) w);
                row = sent;
                r.flags |= F_ROW_SENT;
            }
            memcpy(q.prev, q.image, (size_t) w);
        } else {
            memset(q.prev, 0, (size_t) w);                              // counted, not decoded: DEFINED as zeros
        }
        machine_tail(s, r);
    }
    rec_finish(s, type, r);
    on_line(user, &r, row, w + 1);
}

// ProcessSamples over one block; blk: its number in the push (the record's)
inline void full_block(full_t &q, const int16_t *samps, double srate, int blk, line_t on_line, void *user)
{
    if (!q.started) return;
    state_t &s = q.s;
    int front;
    const int nsamps = block_head(s, q.shift, &front);
    q.shift = 0;
    samps += front;
    int i = 0;
    while (i < nsamps) {
        for (; i < nsamps && s.samp_idx < s.spl;) {
            q.samples[s.samp_idx] = samps[i];
            s.samp_idx++;
            s.fi += s.ratio;
            i = (int) trunc(s.fi);
        }
        if (s.samp_idx == s.spl) {
            rec_t r;
            memset(&r, 0, sizeof r);
            r.blk = blk; r.off = i;
            full_line(q, srate, r, on_line, user);
            s.samp_idx = 0;
        }
    }
    s.fi -= nsamps;
}
#endif

}  // namespace kg_fax_cf
#endif
