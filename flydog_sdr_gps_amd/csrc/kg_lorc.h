// kg_lorc.h -- the Loran-C extension (extensions/Loran_C/loran_c.cpp), a consumer of receive_iq_samps(PRE_AGC): the power of every
// CFastFIR output sample folded into time buckets over one Group Repetition Interval (GRI) of a chain, for two chains at once, under
// one of three averaging rules, and about once a second per chain the averages as a byte row (the "scope").  On the device AND the
// host, in the reference's own operand types; library, host driver and golden are built with -ffp-contract=off.  What lives here:
//   * loran_c_data (:65-196): pwr = re*re + im*im in float; bn = floor(fmod(samp - offset, samp_per_GRI)) with the difference
//     UNSIGNED (u4_t - int: huge while samp < offset, wrapping at 2^32) and converted to double; the emission (:87-122): max the
//     maximum of avg[0 .. nbucket) under auto gain, gain * CUTESDR_MAX_VAL else, byte j + 1 = (u1_t)(int)(255 * (avg / max)) behind
//     the clamp to [0, max], 0 when max == 0, byte 0 the channel; the three rules (:125-189): CMA avg = (avg * navgs + pwr) / (navgs + 1)
//     with navgs a u4_t converted to float, EMA avg += (pwr - avg) / avg_param_i, IIR avg += (pwr - avg) * iir_gain with iir_gain =
//     1.0 - expf(-(avg_param_f) * pwr / CUTESDR_MAX_VAL) -- product and quotient in double, rounded to float for expf, the double
//     difference stored to the FLOAT iir_gain of :186 -- all under the guard bn < nbucket - 1: bucket nbucket - 1 is never written;
//   * init_gri (:198-208) and the commands of loran_c_msgs (:218-302).
// The schedule -- bn, dsp_samps, avg_samps, navgs, restart, redraw_legend: where a sample goes, when a row leaves, when avg[] is
// cleared -- depends on no sample value.  first_sample() is that schedule for one sample, as the reference walks it; run_walk() is
// the same over a stretch of samples cut into RUNS, maximal stretches over which bn rises by one per sample: fmod is exact, so behind
// x0 = fmod(d, samp_per_GRI) sample k of the run has the remainder x0 + k exactly while that is below samp_per_GRI (the sum is
// representable because it IS a remainder), and only a run's first sample can have bn == 0.  One fmod a run, not one a sample.
// Samples are finite with |re|, |im| <= 3e4.  REFUSED, nothing changed (the reference does not define them):
//   * a Loran channel outside 0 .. 1;
//   * a gri outside 1 .. 9999 (MAX_GRI);
//   * a gri whose nbucket (after the halving) is >= 1199 (MAX_BUCKET): the reference then writes scope[1199], one past its array and
//     into redraw_legend -- GRI 9990 at 12 kHz;
//   * `SET offset` before a GRI is set (% 0);
//   * an avg_algo outside 0 .. 2 (the reference panics);
//   * at the push, a started connection one of whose channels has no GRI (fmod(x, 0) is NaN, then an int conversion), is under EMA
//     with avg_param_i < 1, or under IIR with a negative or non-finite avg_param_f: the averages leave the finite floats and the
//     reference's int conversion is undefined.
#ifndef KG_LORC_H
#define KG_LORC_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "kg_nr.h"
#if defined(__HIPCC__)
#include "kg_libm.h"
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KG_LORC_EXPF(x) kg_libm::expf_glibc(x)          // the host libm's expf, bit for bit (kg_libm.h)
#else
#define KG_LORC_EXPF(x) expf(x)
#endif

namespace kg_lorc_cf {

enum { NCH = 2, MAX_GRI = 9999, MAX_BUCKET = 1199, HALF_THRESHOLD = 12000, MAX_NS = 512 };      // :22-24, :47
enum { SCOPE_DATA = 0, SCOPE_RESET = 1 };                                                         // :17-18
enum { AVG_CMA = 0, AVG_EMA = 1, AVG_IIR = 2 };                                                   // :58-60
enum { REFUSED_CH = -1, REFUSED_GRI = -2, REFUSED_NBUCKET = -3, REFUSED_OFFSET = -4, REFUSED_ALGO = -5, REFUSED_NO_GRI = -6, REFUSED_EMA = -7,
       REFUSED_IIR = -8 };
#define KG_LORC_MAX_VAL 32767.0f                                                                   /* CUTESDR_MAX_VAL, kiwi.h:42-43 */

// loran_c_ch_t without avg[] (:29-39); max lives where avg[] lives: the samples decide it
struct chan_t {
    uint32_t gri, samp, nbucket, dsp_samps, avg_samps, navgs;
    double samp_per_GRI;
    float gain;
    int32_t offset, avg_algo;
    double avg_param_f;
    int32_t avg_param_i;
    int32_t restart;
};
// loran_c_t (:41-52) and whether loran_c_data is registered
struct state_t {
    int32_t inited, started;
    uint32_t i_srate;
    double srate;
    chan_t ch[NCH];
    int32_t redraw_legend;
};

// ---- the arithmetic of one sample
KG_NR_HD float power(float re, float im) { return re * re + im * im; }                               // :78
KG_NR_HD float cma_step(float avg, uint32_t navgs, float pwr)                                         // :148-149
{
    avg = (avg * navgs) + pwr;
    avg /= navgs + 1;
    return avg;
}
KG_NR_HD float ema_step(float avg, float pwr, int decay) { return avg + (pwr - avg) / decay; }        // :168
KG_NR_HD float iir_step(float avg, float pwr, double avg_param_f)                                     // :186-187
{
    const float iir_gain = 1.0 - KG_LORC_EXPF(-(avg_param_f) * pwr / KG_LORC_MAX_VAL);
    return avg + (pwr - avg) * iir_gain;
}
KG_NR_HD float update(int algo, float avg, float pwr, uint32_t navgs, int avg_param_i, double avg_param_f)
{
    return algo == AVG_CMA ? cma_step(avg, navgs, pwr) : algo == AVG_EMA ? ema_step(avg, pwr, avg_param_i) : iir_step(avg, pwr, avg_param_f);
}
KG_NR_HD float fixed_max(float gain) { return gain * KG_LORC_MAX_VAL; }                               // :101
KG_NR_HD unsigned char scope_byte(float avg, float max)                                               // :108-114
{
    if (avg > max) avg = max;
    if (avg < 0) avg = 0;
    const int scope = max ? (255 * (avg / max)) : 0;
    return (unsigned char) scope;
}

// ---- the schedule
inline double unsigned_diff(uint32_t samp, int32_t offset) { return (double) (uint32_t) (samp - (uint32_t) offset); }
inline int bucket(const chan_t &c) { return (int) floor(fmod(unsigned_diff(c.samp, c.offset), c.samp_per_GRI)); }      // :85

// What one sample with bucket bn does to the scalars (:87-88, :121-146, :154-159, :173-178, :193), no average touched.  *emit: a
// row goes out ahead of the update (dsp_samps > i_srate was checked ahead of a pending restart); *zero: avg[0 .. nbucket) is cleared
// ahead of the update.  navgs behind the call is the one the update of this sample (and of its run) uses.
inline void first_sample(state_t &e, chan_t &c, int bn, int *emit, int *zero)
{
    *emit = *zero = 0;
    if (bn == 0 && c.dsp_samps > e.i_srate) { c.dsp_samps = 0; *emit = 1; }
    c.dsp_samps++;
    if (c.avg_algo == AVG_CMA) {
        if (bn == 0 && (c.restart || (c.avg_samps > (e.i_srate * (uint32_t) c.avg_param_i)))) {
            if (c.restart) { c.restart = 0; c.dsp_samps = 0; }
            *zero = 1;
            c.avg_samps = 0;
            c.navgs = (uint32_t) -1;
        }
        c.avg_samps++;
        if (bn == 0) c.navgs++;
    } else if (bn == 0 && c.restart) {
        c.restart = 0; c.dsp_samps = 0;
        *zero = 1;
    }
    c.samp++;
}

// a run: samples [start, start + len) of the stretch have the buckets bn0, bn0 + 1 ...; emit / zero belong to its first sample
// (emit behind plan_stretch: 1 + the emission's place in the send order)
struct run_t { int32_t start, len, bn0, emit, zero; uint32_t navgs; };

// The stretch of n samples (n >= 0) of channel c cut into runs, each handed to on_run(user, run) in order; advances c.  A run ends
// where x0 + k reaches samp_per_GRI, where the unsigned difference wraps and where samp wraps.
template <typename F> inline void run_walk(state_t &e, chan_t &c, int n, F on_run)
{
    for (int i = 0; i < n;) {
        const uint32_t d = c.samp - (uint32_t) c.offset;
        const double x0 = fmod((double) d, c.samp_per_GRI);
        int64_t len = (int64_t) ceil(c.samp_per_GRI - x0);            // the count of k >= 0 with x0 + k < samp_per_GRI, then held to that test
        if (len > n - i) len = n - i;
        while (len > 1 && !(x0 + (double) (len - 1) < c.samp_per_GRI)) len--;
        while (len < n - i && x0 + (double) len < c.samp_per_GRI) len++;
        if (len < 1) len = 1;
        const int64_t to_wrap_d = ((int64_t) 1 << 32) - (int64_t) d, to_wrap_s = ((int64_t) 1 << 32) - (int64_t) c.samp;
        if (len > to_wrap_d) len = to_wrap_d;
        if (len > to_wrap_s) len = to_wrap_s;
        run_t r;
        r.start = i; r.len = (int32_t) len; r.bn0 = (int) floor(x0);
        first_sample(e, c, r.bn0, &r.emit, &r.zero);
        r.navgs = c.navgs;
        const uint32_t rest = (uint32_t) (len - 1);                  // bn != 0: dsp_samps, avg_samps (CMA) and samp go on
        c.dsp_samps += rest;
        if (c.avg_algo == AVG_CMA) c.avg_samps += rest;
        c.samp += rest;
        on_run(r);
        i += (int) len;
    }
}

// one ext_send_msg_data of :119-120
struct emis_t { int32_t samp, ch, cmd, len; };
struct plan_t {
    std::vector<run_t> runs[NCH];
    std::vector<emis_t> emis;                   // in the reference's send order: sample-major, channel 0 ahead of channel 1
};

// loran_c_data's schedule over a stretch of n samples of one connection: the runs of both channels and the rows with their commands
// (redraw_legend is the connection's: the first row behind a `SET gri` or `SET start` is the SCOPE_RESET, whichever channel sends it)
inline void plan_stretch(state_t &e, int n, plan_t &p)
{
    p.emis.clear();
    for (int ch = 0; ch < NCH; ch++) {
        p.runs[ch].clear();
        chan_t &c = e.ch[ch];
        run_walk(e, c, n, [&](const run_t &r) {
            p.runs[ch].push_back(r);
            if (r.emit) p.emis.push_back(emis_t{r.start, ch, 0, (int32_t) c.nbucket + 1});
        });
    }
    std::stable_sort(p.emis.begin(), p.emis.end(), [](const emis_t &a, const emis_t &b) { return a.samp != b.samp ? a.samp < b.samp : a.ch < b.ch; });
    for (emis_t &m : p.emis) { m.cmd = e.redraw_legend ? SCOPE_RESET : SCOPE_DATA; e.redraw_legend = 0; }
    for (int ch = 0; ch < NCH; ch++)
        for (run_t &r : p.runs[ch])
            if (r.emit)
                for (size_t k = 0; k < p.emis.size(); k++)
                    if (p.emis[k].samp == r.start && p.emis[k].ch == ch) { r.emit = 1 + (int32_t) k; break; }
}

// ---- init_gri and the commands
inline bool ch_ok(int ch) { return ch >= 0 && ch < NCH; }

// `SET ext_server_init` (:218-228): the memset; srate: ext_update_get_sample_rateHz, i_srate: snd_rate.  The registration stays.
inline void cmd_init(state_t &e, double srate, int i_srate)
{
    const int started = e.started;
    memset(&e, 0, sizeof e);
    e.inited = 1; e.started = started;
    e.srate = srate;
    e.i_srate = (uint32_t) i_srate;
}
inline float ms_per_bin(double srate, int i_srate)                     // :223-224
{
    float ms = 1.0 / srate * 1e3;
    if (i_srate > HALF_THRESHOLD) ms *= 2;
    return ms;
}
inline int cmd_gri(state_t &e, int ch, int gri)                        // :231-240 with init_gri (:198-208)
{
    if (!ch_ok(ch)) return REFUSED_CH;
    if (gri < 1 || gri > MAX_GRI) return REFUSED_GRI;
    double spg = e.srate * ((double) (gri) / 1e5);
    const double nb = floor(spg) + 1;
    if (!(nb >= 1 && nb < 4294967296.0)) return REFUSED_NBUCKET;
    uint32_t nbucket = (uint32_t) nb;
    if (nbucket > MAX_BUCKET) { spg /= 2; nbucket /= 2; }
    if (nbucket >= MAX_BUCKET) return REFUSED_NBUCKET;
    chan_t &c = e.ch[ch];
    c.gri = (uint32_t) gri; c.samp_per_GRI = spg; c.nbucket = nbucket;
    e.redraw_legend = 1;
    c.restart = 1;
    return 0;
}
inline int cmd_offset(state_t &e, int ch, int offset)                  // :243-250: the int sum is converted to unsigned ahead of the modulo
{
    if (!ch_ok(ch)) return REFUSED_CH;
    chan_t &c = e.ch[ch];
    if (c.nbucket == 0) return REFUSED_OFFSET;
    c.offset = (int32_t) (((uint32_t) c.offset + (uint32_t) offset) % c.nbucket);
    c.restart = 1;
    return 0;
}
inline int cmd_gain(state_t &e, int ch, int gain)                      // :253-260
{
    if (!ch_ok(ch)) return REFUSED_CH;
    e.ch[ch].gain = gain ? pow(10.0, ((float) -(int64_t) gain) / 10.0) : 0;
    e.ch[ch].restart = 1;
    return 0;
}
inline int cmd_avg_algo(state_t &e, int ch, int algo)                  // :263-269
{
    if (!ch_ok(ch)) return REFUSED_CH;
    if (algo < AVG_CMA || algo > AVG_IIR) return REFUSED_ALGO;
    e.ch[ch].avg_algo = algo;
    e.ch[ch].restart = 1;
    return 0;
}
inline int cmd_avg_param(state_t &e, int ch, double avg_param)         // :272-280
{
    if (!ch_ok(ch)) return REFUSED_CH;
    e.ch[ch].avg_param_f = avg_param;
    e.ch[ch].avg_param_i = (int32_t) lround(avg_param);
    e.ch[ch].restart = 1;
    return 0;
}
inline void cmd_start(state_t &e)                                      // :282-292
{
    e.redraw_legend = 1;
    e.ch[0].restart = e.ch[1].restart = 1;
    e.started = 1;
}
inline void cmd_stop(state_t &e) { e.started = 0; }                    // :294-302

// what a push of a started connection is refused for (0: taken)
inline int push_check(const state_t &e)
{
    for (int ch = 0; ch < NCH; ch++) {
        const chan_t &c = e.ch[ch];
        if (c.nbucket == 0) return REFUSED_NO_GRI;
        if (c.avg_algo == AVG_EMA && c.avg_param_i < 1) return REFUSED_EMA;
        if (c.avg_algo == AVG_IIR && !(c.avg_param_f >= 0 && c.avg_param_f <= 1.7976931348623157e308)) return REFUSED_IIR;
    }
    return 0;
}

// ---- the whole object on the host
struct full_t {
    state_t s;
    float avg[NCH][MAX_BUCKET];
    float max[NCH];
};
typedef void (*emit_t)(void *user, int samp, int ch, int cmd, const unsigned char *bytes, int nbytes);

// the emission of channel ch (:88-121)
inline void emit_row(full_t &q, int ch, int samp, emit_t emit, void *user)
{
    const chan_t &c = q.s.ch[ch];
    unsigned char scope[MAX_BUCKET + 1];
    float max = 0;
    if (c.gain == 0) {
        for (uint32_t j = 0; j < c.nbucket; j++)
            if (q.avg[ch][j] > max) max = q.avg[ch][j];
    } else max = fixed_max(c.gain);
    q.max[ch] = max;
    for (uint32_t j = 0; j < c.nbucket; j++) scope[j + 1] = scope_byte(q.avg[ch][j], max);
    scope[0] = (unsigned char) ch;
    emit(user, samp, ch, q.s.redraw_legend ? SCOPE_RESET : SCOPE_DATA, scope, (int) c.nbucket + 1);
    q.s.redraw_legend = 0;
}

// loran_c_data, sample by sample with one fmod a sample and channel: the twin run_walk is held to
inline void data_per_sample(full_t &q, int ns, const float *samps, emit_t emit, void *user)
{
    for (int i = 0; i < ns; i++) {
        const float pwr = power(samps[2 * i], samps[2 * i + 1]);
        for (int ch = 0; ch < NCH; ch++) {
            chan_t &c = q.s.ch[ch];
            const int bn = bucket(c);
            int em, zero;
            first_sample(q.s, c, bn, &em, &zero);
            if (em) emit_row(q, ch, i, emit, user);
            if (zero) for (uint32_t j = 0; j < c.nbucket; j++) q.avg[ch][j] = 0;
            if ((uint32_t) bn < c.nbucket - 1) q.avg[ch][bn] = update(c.avg_algo, q.avg[ch][bn], pwr, c.navgs, c.avg_param_i, c.avg_param_f);
        }
    }
}

// the same through plan_stretch, run by run as the kernel walks them
inline void data_by_runs(full_t &q, int ns, const float *samps, emit_t emit, void *user)
{
    plan_t p;
    state_t before = q.s;
    plan_stretch(q.s, ns, p);
    std::vector<std::vector<unsigned char>> rows(p.emis.size());
    for (int ch = 0; ch < NCH; ch++) {
        const chan_t &c = before.ch[ch];                                 // the commands' part: constant over a call
        for (const run_t &r : p.runs[ch]) {
            if (r.emit) {
                std::vector<unsigned char> &row = rows[r.emit - 1];
                row.assign(c.nbucket + 1, 0);
                float max = 0;
                if (c.gain == 0) {
                    for (uint32_t j = 0; j < c.nbucket; j++)
                        if (q.avg[ch][j] > max) max = q.avg[ch][j];
                } else max = fixed_max(c.gain);
                q.max[ch] = max;
                for (uint32_t j = 0; j < c.nbucket; j++) row[j + 1] = scope_byte(q.avg[ch][j], max);
                row[0] = (unsigned char) ch;
            }
            if (r.zero) for (uint32_t j = 0; j < c.nbucket; j++) q.avg[ch][j] = 0;
            for (int k = 0; k < r.len; k++) {
                const int bn = r.bn0 + k, i = r.start + k;
                if ((uint32_t) bn < c.nbucket - 1)
                    q.avg[ch][bn] = update(c.avg_algo, q.avg[ch][bn], power(samps[2 * i], samps[2 * i + 1]), r.navgs, c.avg_param_i, c.avg_param_f);
            }
        }
    }
    for (size_t k = 0; k < p.emis.size(); k++) emit(user, p.emis[k].samp, p.emis[k].ch, p.emis[k].cmd, rows[k].data(), (int) rows[k].size());
}

}  // namespace kg_lorc_cf
#endif
