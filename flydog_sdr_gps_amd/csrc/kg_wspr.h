// kg_wspr.h -- the WSPR extension (extensions/wspr/), stage 1: from the IQ tap (receive_iq_samps, CFastFIR's output of every sound
// block) to the candidate list.  On the device AND the host, in the reference's own operand types; library, host driver and golden are
// built with -ffp-contract=off.  What lives here:
//   * wspr_data (wspr_main.cpp:595-788, the #else branch of FRACTIONAL_DECIMATION, :757-785), wspr_reset (:790-800) and the commands
//     of wspr_msgs (:826-916): reset, capture, drop-sample decimation, the sync to the even minute, ping-pong, the re-arm at group 3,
//     the wait at didx >= TPOINTS, which group's transforms are due and when the cycle ends.  NO SAMPLE DRIVES ANY OF IT: sched_block()
//     walks one callback on sample counts and on the clock the caller hands in, and emits the copy runs, the groups due and the status
//     changes (wspr_status, :96-114) as records;
//   * WSPR_FFT (:117-209): the sine window (:1186-1188), fftin = sample * window in float, the unwrap k = j + SPS, pwr = ii*ii + qq*qq,
//     pwr_samp, pwr_sampavg and savg added to in FFT order.  The transform itself is the caller's (the reference links FFTW);
//   * the group's display row (:211-240) behind renormalize (wspr.cpp:214-253): the 7-bin sums in j order, the 123rd smallest of 411 as
//     the noise level, x / noise - 1.0 in double, the min_snr floor, 10*log10 - snr_scaling_factor, the byte;
//   * pass 0 of wspr_decode: the peak list (wspr.cpp:555-628 with snr_comp / freq_comp, wspr_util.cpp:394-406) and the coarse search
//     over frequency +-2, time -10 .. 21 and drift +-4 (wspr.cpp:658-714).
// Kept to the letter: log10 and sqrt of a float argument are the float overloads (the reference is C++ and includes <math.h>); the
// mixed float / double expression of ifd (:678) and its truncation; if0 = freq0/DF2+SPS taken before the loops; shift0 = HSPS*(k0+1);
// kindex >= 0 && kindex < nffts; the left-to-right sums of ss and power; sync1 > smax in the order ifr, k0, idrift from smax = -1e30:
// the first maximum wins and a NaN (power 0) never does -- such a candidate keeps the zeros of the memset of :560.
// Defined here where the reference leaves it open:
//   * the decoder of stage 1 takes no time: the status events of a cycle end are DECODING, the peaks, then status_resume (:472, :568);
//   * a byte whose y is NaN (silence: the noise level is 0) is 0 -- the comparisons of :232-233 are false and (u1_t) NaN is undefined;
//   * qsort on equal keys is unspecified: ties in snr0 keep frequency order.
// REFUSED, nothing changed: snd_rate below 375 or not finite, a type other than 2 / 15, minute outside 0 .. 59 or second outside
// 0 .. 59, a push before init.  Non-finite samples are undefined as in the reference.
#ifndef KG_WSPR_H
#define KG_WSPR_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "kg_nr.h"
#if defined(__HIPCC__)
#include "kg_libm.h"
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KG_WSPR_LOG10(x) kg_libm::log10f_glibc(x)          // the host libm's log10f, bit for bit (kg_libm.h)
#else
#define KG_WSPR_LOG10(x) log10(x)                          // a float argument: the float overload, as in the reference
#endif
#define KG_WSPR_SQRT(x) sqrtf(x)                           /* sqrt of a float argument: correctly rounded on host and device alike */

namespace kg_wspr_cf {

// wspr.h:142-183 and the assigned constants of wspr_main() (:1154-1156)
enum { SRATE = 375, CTIME = 120, TPOINTS = SRATE * CTIME, NBINS = 411, HBINS = 205, FMIN = -110, FMAX = 110 };
enum { SPS = 256, NFFT = 512, HSPS = 128, GROUPS = TPOINTS / NFFT, FPG = 4, NT = FPG * GROUPS, NFFTS = FPG * (GROUPS - 1) - 1, LAST_GROUP = GROUPS - 2 };
enum { NSYM = 162, NPK = 256, MAX_NPK = 12, GROUP_SPAN = NFFT + (FPG - 1) * HSPS };
enum { NIFR = 5, NK0 = 32, NDRIFT = 9, NHYP = NIFR * NK0 * NDRIFT, K0_MIN = -10, MAXDRIFT = 4 };
enum { ST_NONE = 0, ST_IDLE = 1, ST_SYNC = 2, ST_RUNNING = 3, ST_DECODING = 4 };                   // wspr_main.cpp:49-53
enum { TYPE_2MIN = 2, TYPE_15MIN = 15 };
enum { REFUSED_RATE = -1, REFUSED_TYPE = -2, REFUSED_TIME = -3, REFUSED_NOT_INITED = -4 };
static_assert(TPOINTS == 45000 && GROUPS == 87 && NT == 348 && NFFTS == 343 && LAST_GROUP == 85 && GROUP_SPAN == 896 && NHYP == 1440, "constants");
#define KG_WSPR_DF2 0.732421875f                           /* FSRATE/FSPS/2 (wspr.cpp:490): exact */
#define KG_WSPR_K_PI (3.14159265358979323846)              /* rx/CuteSDR/datatypes.h */

// the sync vector of the WSPR protocol (wspr.cpp:31-40)
#define KG_WSPR_PR3                                                                                                                    \
    {1,1,0,0,0,0,0,0,1,0,0,0,1,1,1,0,0,0,1,0,0,1,0,1,1,1,1,0,0,0,0,0,0,0,1,0,0,1,0,1,0,0,0,0,0,0,1,0,1,1,0,0,1,1,0,1,0,0,0,1,1,0,1,0,  \
     0,0,0,1,1,0,1,0,1,0,1,0,1,0,0,1,0,0,1,0,1,1,0,0,0,1,1,0,1,0,1,0,0,0,1,0,0,0,0,0,1,0,0,1,0,0,1,1,1,0,1,1,0,0,1,1,0,1,0,0,0,1,1,1,  \
     0,0,0,0,0,1,0,1,0,0,1,1,0,0,0,0,0,0,0,1,1,0,1,0,1,1,0,0,0,1,1,0,0,0}

// ---- the arithmetic
inline float window_at(int i) { return sin(i * KG_WSPR_K_PI / (NFFT - 1)); }                      // :1187, host only: the device reads a table
KG_NR_HD float windowed(float x, float w) { return x * w; }                                       // :175-176
KG_NR_HD float power(float ii, float qq) { return ii * ii + qq * qq; }                            // :197
KG_NR_HD int unwrap(int j) { int k = j + SPS; if (k > (NFFT - 1)) k -= NFFT; return k; }         // :192-194: the transform's bin of plane row j
KG_NR_HD float snr_scaling(int type) { return type == TYPE_2MIN ? 26.3 : 35.3; }                  // wspr.cpp:247
inline float min_snr_value() { return pow(10.0, -7.0 / 10.0); }                                   // wspr.cpp:246, host only: the kernels take it as a parameter
// renormalize's 7-point sum of bin i (wspr.cpp:221-229); k < NFFT always holds: k <= 464
KG_NR_HD float smooth7(const float *psavg, int i)
{
    float s = 0.0;
    for (int j = -3; j <= 3; j++) {
        const int k = SPS - HBINS + i + j;
        if (k < NFFT) s += 1 * psavg[k];
    }
    return s;
}
KG_NR_HD float renorm(float x, float noise_level, float min_snr)                                   // wspr.cpp:249-250
{
    x = x / noise_level - 1.0;
    if (x < min_snr) x = 0.1 * min_snr;
    return x;
}
KG_NR_HD float to_db(float x, float scaling) { return 10 * KG_WSPR_LOG10(x) - scaling; }          // :216, wspr.cpp:571
KG_NR_HD unsigned char row_byte(float db)                                                          // :221-234; NaN: 0
{
    const float max_dB = 6, min_dB = -33;
    const float range_dB = max_dB - min_dB;
    const float pix_per_dB = 255.0 / range_dB;
    float y = pix_per_dB * (db - min_dB);
    if (y > 255.0) y = 255.0;
    if (y < 0) y = 0;
    return y == y ? (unsigned char) y : (unsigned char) 0;
}
KG_NR_HD float freq_of_bin(int j) { return (j - HBINS) * KG_WSPR_DF2; }                            // wspr.cpp:570
KG_NR_HD int if0_of(float freq0) { return freq0 / KG_WSPR_DF2 + SPS; }                             // wspr.cpp:665
KG_NR_HD int ifd_of(int ifr, int k, int idrift)                                                    // wspr.cpp:678
{
    return ifr + ((float) k - (162.0 / 2)) / (162.0 / 2) * ((float) idrift) / (2.0 * KG_WSPR_DF2);
}
KG_NR_HD float freq_of_ifr(int ifr) { return (ifr - SPS) * KG_WSPR_DF2; }                          // wspr.cpp:704

// the 123rd smallest of n values (wspr.cpp:233-239): rank counting, any correct selection equals qsort's tmpsort[122] on ordered values
inline float rank_select(const float *v, int n, int rank)
{
    for (int a = 0; a < n; a++) {
        int r = 0;
        for (int b = 0; b < n; b++) r += (v[b] < v[a]) || (v[b] == v[a] && b < a);
        if (r == rank) return v[a];
    }
    return 0.0f;
}

struct pk_t { int32_t bin0; float freq0, snr0; int32_t pad; };                                    // what WSPR_PEAKS needs of a wspr_pk_t (wspr.h:185-191)
struct cand_t { float freq0; int32_t shift0; float drift0, sync0; int32_t freq_idx, bin0; };      // the coarse estimates of one (:702-705)

// The peak list of pass 0 from the renormalised spectrum sm[411] (wspr.cpp:559-628): local maxima or every second bin above min_snr,
// FMIN .. FMAX, the MAX_NPK strongest (ties in frequency order), freq_idx their place in frequency order.  pk: in frequency order;
// cand: in SNR order with freq0 / bin0 / freq_idx set and the rest zero.  Returns npk.  One lane's work on the device.
KG_NR_HD int peak_list(const float *sm, int more_candidates, float min_snr, float scaling, pk_t *pk, cand_t *cand)
{
    int bins[MAX_NPK];
    float snrs[MAX_NPK];
    int npk = 0, all = 0;
    // the MAX_NPK strongest by insertion: an entry goes in front of the first that is strictly weaker, so equals keep frequency order
    for (int j = more_candidates ? 0 : 1; j < (more_candidates ? NBINS : NBINS - 1); j += more_candidates ? 2 : 1) {
        const bool candidate = (more_candidates ? (sm[j] > min_snr) : (sm[j] > sm[j - 1]) && (sm[j] > sm[j + 1])) && (all < NPK);
        if (!candidate) continue;
        all++;
        const float freq0 = freq_of_bin(j);
        if (!(freq0 >= FMIN && freq0 <= FMAX)) continue;
        const float snr0 = to_db(sm[j], scaling);
        int at = npk;
        while (at > 0 && snrs[at - 1] < snr0) at--;
        if (at >= MAX_NPK) continue;
        if (npk < MAX_NPK) npk++;
        for (int m = npk - 1; m > at; m--) { bins[m] = bins[m - 1]; snrs[m] = snrs[m - 1]; }
        bins[at] = j; snrs[at] = snr0;
    }
    for (int r = 0; r < npk; r++) {
        int idx = 0;
        for (int m = 0; m < npk; m++) idx += bins[m] < bins[r];
        cand[r].freq0 = freq_of_bin(bins[r]); cand[r].shift0 = 0; cand[r].drift0 = 0; cand[r].sync0 = 0; cand[r].freq_idx = idx; cand[r].bin0 = bins[r];
        pk[idx].bin0 = bins[r]; pk[idx].freq0 = freq_of_bin(bins[r]); pk[idx].snr0 = snrs[r]; pk[idx].pad = 0;
    }
    return npk;
}

// one hypothesis of the coarse search (wspr.cpp:675-699) on the plane of ROOTS: rt(bin, kindex) = sqrt(pwr_samp[bin][kindex]);
// fd(k) = ifd_of(ifr, k, idrift), which depends on no sample: the kernel reads it from a table it made with that very function
template <typename RT, typename FD> KG_NR_HD float sync_of(RT rt, FD fd, const unsigned char *pr3, int k0)
{
    float ss = 0.0, power = 0.0;
    for (int k = 0; k < NSYM; k++) {
        const int ifd = fd(k);
        const int kindex = k0 + 2 * k;
        if (kindex >= 0 && kindex < NFFTS) {
            const float p0 = rt(ifd - 3, kindex), p1 = rt(ifd - 1, kindex), p2 = rt(ifd + 1, kindex), p3 = rt(ifd + 3, kindex);
            ss = ss + (2 * pr3[k] - 1) * ((p1 + p3) - (p0 + p2));
            power = power + p0 + p1 + p2 + p3;
        }
    }
    return ss / power;
}
// hypothesis h in the order of the loops: ifr outermost, then k0, then idrift
KG_NR_HD void hyp_of(int h, int if0, int *ifr, int *k0, int *idrift)
{
    *ifr = if0 - 2 + h / (NK0 * NDRIFT);
    *k0 = K0_MIN + (h / NDRIFT) % NK0;
    *idrift = -MAXDRIFT + h % NDRIFT;
}
KG_NR_HD void take_hyp(cand_t &c, int h, int if0, float sync1)                                     // :701-705
{
    int ifr, k0, idrift;
    hyp_of(h, if0, &ifr, &k0, &idrift);
    c.shift0 = HSPS * (k0 + 1);
    c.drift0 = idrift;
    c.freq0 = freq_of_ifr(ifr);
    c.sync0 = sync1;
}

// ---- the whole cycle end on the host (the twin the kernels are held to).  pwr_samp[j * NT + i] and pwr_sampavg[j] as the reference has them.
struct cycle_t { int32_t npk; pk_t pk[MAX_NPK]; cand_t cand[MAX_NPK]; };
inline void renormalize(const float *psavg, int type, float *sm)
{
    float tmp[NBINS];
    for (int i = 0; i < NBINS; i++) tmp[i] = sm[i] = smooth7(psavg, i);
    const float noise_level = rank_select(tmp, NBINS, 122);
    const float min_snr = min_snr_value();
    for (int j = 0; j < NBINS; j++) sm[j] = renorm(sm[j], noise_level, min_snr);
    (void) type;
}
inline void row_of(const float *savg, int type, int flag, unsigned char *ws)                       // :211-236
{
    float sm[NBINS];
    renormalize(savg, type, sm);
    for (int j = 0; j < NBINS; j++) ws[j + 1] = row_byte(to_db(sm[j], snr_scaling(type)));
    ws[0] = flag ? 1 : 0;
}
inline void cycle_end(const float *pwr_samp, const float *pwr_sampavg, int type, int more_candidates, cycle_t &out)
{
    static const unsigned char pr3[NSYM] = KG_WSPR_PR3;
    float sm[NBINS];
    memset(&out, 0, sizeof out);
    renormalize(pwr_sampavg, type, sm);
    out.npk = peak_list(sm, more_candidates, min_snr_value(), snr_scaling(type), out.pk, out.cand);
    for (int pki = 0; pki < out.npk; pki++) {
        cand_t &c = out.cand[pki];
        float smax = -1e30;
        const int if0 = if0_of(c.freq0);
        auto rt = [&](int bin, int kindex) { const float p = KG_WSPR_SQRT(pwr_samp[(size_t) bin * NT + kindex]); return p; };
        for (int h = 0; h < NHYP; h++) {
            int ifr, k0, idrift;
            hyp_of(h, if0, &ifr, &k0, &idrift);
            const float sync1 = sync_of(rt, [&](int k) { return ifd_of(ifr, k, idrift); }, pr3, k0);
            if (sync1 > smax) { smax = sync1; take_hyp(c, h, if0, sync1); }
        }
    }
}

// ---- the schedule
// wspr_t, what stage 1 keeps of it (wspr.h:239-312)
struct state_t {
    int32_t inited, capture, reset, tsync;
    int32_t ping_pong, fft_ping_pong, decode_ping_pong, decim, didx, group;
    int32_t status, status_resume, last_sec, abort_decode;
    int32_t wspr_type, more_candidates, int_decimate, cycles;
    double snd_rate;
};
enum { OP_COPY = 0, OP_ZERO = 1, OP_GROUP = 2 };
enum { EV_STATUS = 0, EV_PEAKS = 1 };
// what the device does, in order.  COPY: n samples from src (a sample of the push) every int_decimate-th into half's didx0 ..;
// ZERO: pwr_sampavg[half] = 0 (:649-652); GROUP: WSPR_FFT of group a of half, ws[0] = b, the row's place c, due at sample src of the push
struct op_t { int32_t kind, half, a, b, c, n; int64_t src; };
struct ev_t { int32_t blk, samp, kind, a, b; };             // STATUS: a the status, b the resume (0 NONE); PEAKS: a the decode half
struct sched_t {
    std::vector<op_t> ops;
    std::vector<ev_t> evs;
    int32_t nrows = 0, ncycle = 0, cycle_half = 0, cycle_blk = 0;
};

inline void set_status(state_t &w, sched_t *p, int blk, int samp, int status, int resume)          // :96-114
{
    w.status = status;
    if (resume != ST_NONE) w.status_resume = resume;
    if (p) p->evs.push_back(ev_t{blk, samp, EV_STATUS, status, resume});
}
// one callback of wspr_data (:595-788) with ns samples whose first is sample `base` of the push, at min:sec
inline void sched_block(state_t &w, sched_t &p, int blk, int64_t base, int ns, int min, int sec)
{
    if (w.reset) {                                                                                 // :617-623
        w.ping_pong = w.decim = w.didx = w.group = 0;
        w.tsync = 0;
        w.status_resume = ST_IDLE;
        w.reset = 0;
    }
    if (!w.capture) return;
    if (sec != w.last_sec) {
        if ((min & 1) && sec == 40) w.abort_decode = 1;
        w.last_sec = sec;
    }
    if (!w.tsync) {                                                                                // :637-647
        if (!(min & 1) && (sec == 0)) {
            w.ping_pong ^= 1;
            w.decim = w.didx = w.group = 0;
            if (w.status != ST_DECODING) set_status(w, &p, blk, 0, ST_RUNNING, ST_RUNNING);
            w.tsync = 1;
        }
    }
    if (w.didx == 0) p.ops.push_back(op_t{OP_ZERO, w.ping_pong, 0, 0, 0, 0, 0});
    for (int i = 0; i < ns; i++) {                                                                 // :757-784
        if (w.decim++ < (w.int_decimate - 1)) continue;
        w.decim = 0;
        if (w.didx >= TPOINTS) return;
        if (w.group == 3) w.tsync = 0;
        if (!p.ops.empty() && p.ops.back().kind == OP_COPY && p.ops.back().half == w.ping_pong && p.ops.back().a + p.ops.back().n == w.didx &&
            p.ops.back().src + (int64_t) p.ops.back().n * w.int_decimate == base + i)
            p.ops.back().n++;
        else p.ops.push_back(op_t{OP_COPY, w.ping_pong, w.didx, 0, 0, 1, base + i});
        if ((w.didx % NFFT) == (NFFT - 1)) {
            w.fft_ping_pong = w.ping_pong;
            const int grp = w.group - 1;
            if (w.group) {                                                                         // WSPR_FFT (:140-281), run where it is woken
                p.ops.push_back(op_t{OP_GROUP, w.fft_ping_pong, grp, (grp == 0) && w.tsync, p.nrows++, 0, base + i});
                if (!((grp * FPG + FPG) < NFFTS)) {                                                // :275-281, then WSPR_Deco (:468-472, :568)
                    w.decode_ping_pong = w.fft_ping_pong;
                    w.abort_decode = 0;
                    set_status(w, &p, blk, i, ST_DECODING, ST_NONE);
                    p.evs.push_back(ev_t{blk, i, EV_PEAKS, w.decode_ping_pong, 0});
                    p.ncycle++; p.cycle_half = w.decode_ping_pong; p.cycle_blk = blk;
                    w.cycles++;
                    set_status(w, &p, blk, i, w.status_resume, ST_NONE);
                }
            }
            w.group++;
        }
        w.didx++;
    }
}

// ---- the commands (wspr_msgs, :826-916)
inline int cmd_init(state_t &w, double snd_rate)                                                   // `SET ext_server_init`; int_decimate of :1193
{
    if (!(snd_rate >= 375.0 && snd_rate <= 1e9)) return REFUSED_RATE;
    if (!w.inited) {                                                                               // wspr_main (:1163-1176): the memset, the type, wspr_reset
        memset(&w, 0, sizeof w);
        w.wspr_type = TYPE_2MIN;
        w.last_sec = -1;
    }
    w.inited = 1;
    w.snd_rate = snd_rate;
    w.int_decimate = (int) (snd_rate / 375.0);
    set_status(w, nullptr, 0, 0, ST_IDLE, ST_IDLE);
    return 0;
}
inline void cmd_capture(state_t &w, int capture, sched_t *p)                                       // :880-900 with wspr_close / wspr_reset (:790-824)
{
    w.capture = capture;
    if (capture) {
        w.reset = 1;
        set_status(w, p, 0, 0, ST_SYNC, ST_RUNNING);
    } else {
        w.status_resume = ST_IDLE;
        w.tsync = 0;
        w.capture = 0;
        w.last_sec = -1;
        w.abort_decode = 0;
    }
}
inline int cmd_type(state_t &w, int type)
{
    if (type != TYPE_2MIN && type != TYPE_15MIN) return REFUSED_TYPE;
    w.wspr_type = type;
    return 0;
}
inline bool time_ok(int min, int sec) { return min >= 0 && min <= 59 && sec >= 0 && sec <= 59; }

}  // namespace kg_wspr_cf
#endif
