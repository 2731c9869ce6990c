// kg_wspr.hip -- the WSPR extension, stage 1 (extensions/wspr/; csrc/kg_wspr.h is the one definition of its arithmetic and schedule).
//
// The schedule of wspr_data (wspr_main.cpp:595-788) depends on no sample, so the host walks a push block by block (sched_block of
// kg_wspr.h) and hands the kernels a table: per listed connection an entry {connection, its ops' range, type, decimation, where its
// samples are} and per OP, in the reference's order,
//   COPY   every int_decimate-th sample of a stretch of the push into i_data / q_data of a ping-pong half (:769-772);
//   ZERO   pwr_sampavg of a half cleared (:649-652);
//   GROUP  WSPR_FFT of one group (:140-240): its four windowed 512-point transforms, pwr_samp, pwr_sampavg, savg, the display row.
// ONE launch per push: one workgroup of four waves per connection, the ops in order.  A group's 896 samples are read ONCE into LDS;
// each wave takes its 512 from there, eight points a lane, three radix-8 passes (Stockham autosort, kg_fft.h) through two LDS tiles of
// its own, and leaves its 512 powers in LDS; then the workgroup adds them into pwr_sampavg and savg in FFT order, one bin a lane, and
// makes the row from savg in LDS: the 7-bin sums, the 123rd smallest of 411 by rank counting, the bytes.
// pwr_samp is kept as [half][transform][bin] -- a transform's 512 powers are one contiguous store, and the coarse search reads, per
// candidate, 16 neighbouring bins of every transform: 64 contiguous bytes a row.
//
// The push that completes group 85 enqueues a SECOND launch, the cycle end (pass 0 of wspr_decode, wspr.cpp:555-714): MAX_NPK
// workgroups per connection.  Each makes the peak list from pwr_sampavg (cheap, and no workgroup waits for another), then workgroup
// pki searches candidate pki: the ROOTS of the 16 x 343 powers the candidate's hypotheses can touch are formed once into LDS (21 KB),
// ifd of :678 -- which depends on no sample -- once per (ifr, idrift, symbol) into LDS (7 KB),
// the 1440 hypotheses go over the 256 lanes, each lane sums its 162 symbols in order k = 0 .. 161, and the first maximum in the order
// ifr, k0, idrift wins by a reduction on (sync1, hypothesis index).  It also leaves the candidates with the object, for stage 2.
//
// Stage 2 (csrc/kg_wspr_dec.h: fine sync, soft symbols, the Fano decoder; kg_wspr_decode) is described above its kernels below.
#include "kg_ext.h"
#include "kg_fft.h"
#include "kg_wspr.h"
#include "kg_wspr_dec.h"

using namespace kg_wspr_cf;
namespace wd = kg_wspr_df;

static_assert(sizeof(kg_wspr_row) == 32 && sizeof(kg_wspr_ev) == 24 && sizeof(kg_wspr_pk) == 16 && sizeof(kg_wspr_cand) == 24 && sizeof(kg_wspr_cycle) == 496 &&
              sizeof(kg_wspr_info) == 80, "kg_wspr_* layout");
static_assert(sizeof(pk_t) == sizeof(kg_wspr_pk) && sizeof(cand_t) == sizeof(kg_wspr_cand), "kg_wspr_pk / kg_wspr_cand are pk_t / cand_t");
static_assert(KG_WSPR_NBINS == NBINS && KG_WSPR_NFFT == NFFT && KG_WSPR_NT == NT && KG_WSPR_TPOINTS == TPOINTS && KG_WSPR_MAX_NPK == MAX_NPK &&
              KG_WSPR_ROW_STRIDE >= NBINS + 1 && KG_WSPR_IDLE == ST_IDLE && KG_WSPR_DECODING == ST_DECODING && KG_WSPR_EV_STATUS == EV_STATUS &&
              KG_WSPR_EV_PEAKS == EV_PEAKS, "constants");

enum { WS_THREADS = 256, WS_WAVES = 4, WS_LANES = 64, WS_MAX_CONNS = 256, WS_MAX_BLK = 4096, WS_MAX_NS = 131072, WS_MAX_SAMPLES = 1 << 22 };
enum { RT_BINS = 16, RT_HALF = 8, WS_PENDING = 8 };

struct ws_dev {                                                         // one connection
    float idat[2][TPOINTS], qdat[2][TPOINTS];                           // i_data / q_data (wspr.h:224): stage 2 reads them
    float pwr_samp[2][NT][NFFT];                                        // [half][transform][plane row j]
    float pwr_sampavg[2][NFFT];
    float savg[NFFT];
};
struct ws_entry { int32_t conn, first, nops, type, dec, pad; int64_t in_off; };
struct ws_op { int32_t kind, half, a, b, n, pad; int64_t src, row_off; };
struct ws_cyc { int32_t conn, half, type, more, slot, pad[3]; };
static_assert(sizeof(ws_entry) == 32 && sizeof(ws_op) == 40 && sizeof(ws_cyc) == 32, "table layout");
// what stage 2 reads of a connection's last cycle end: the candidates in SNR order, the decode half, and p->ignore (wspr.h:190) per candidate
struct wd_hold { int32_t ncand, half; int32_t ignore[MAX_NPK]; kg_wspr_cand cand[MAX_NPK]; };

__device__ __constant__ const unsigned char ws_pr3[NSYM] = KG_WSPR_PR3;

// the noise level of renormalize (wspr.cpp:233-239) from s_sm[0 .. 411): rank counting, lane t its own element
__device__ __forceinline__ void ws_noise(const float *s_sm, float *s_noise, int tid)
{
    if (tid == 0) *s_noise = 0.0f;
    __syncthreads();
    for (int a = tid; a < NBINS; a += WS_THREADS) {
        const float v = s_sm[a];
        int r = 0;
        for (int b = 0; b < NBINS; b++) r += (s_sm[b] < v) || (s_sm[b] == v && b < a);
        if (r == 122) *s_noise = v;
    }
    __syncthreads();
}

__global__ __launch_bounds__(WS_THREADS) void wspr_push_kernel(const ws_entry *__restrict__ ents, const ws_op *__restrict__ ops, const float2 *__restrict__ in,
                                                               const float *__restrict__ window, const float2 *__restrict__ tab4096, uint8_t *rows, int32_t *counts,
                                                               ws_dev *dev, float min_snr)
{
    __shared__ float s_i[GROUP_SPAN], s_q[GROUP_SPAN];
    __shared__ float2 s_a[WS_WAVES][NFFT], s_b[WS_WAVES][NFFT];
    __shared__ float s_pw[WS_WAVES][NFFT];
    __shared__ float s_savg[NFFT];
    __shared__ float s_sm[NBINS + 5];
    __shared__ float s_noise;
    const ws_entry e = ents[blockIdx.x];
    const int tid = (int) threadIdx.x, w = tid >> 6, l = tid & 63;
    ws_dev *d = dev + e.conn;
    const float2 *src = in + e.in_off;
    const float scaling = snr_scaling(e.type);
    int nrows = 0;
    for (int o = 0; o < e.nops; o++) {
        const ws_op op = ops[e.first + o];
        if (op.kind == OP_COPY) {
            for (int t = tid; t < op.n; t += WS_THREADS) {
                const float2 x = src[op.src + (int64_t) t * e.dec];
                d->idat[op.half][op.a + t] = x.x;
                d->qdat[op.half][op.a + t] = x.y;
            }
        } else if (op.kind == OP_ZERO) {
            for (int j = tid; j < NFFT; j += WS_THREADS) d->pwr_sampavg[op.half][j] = 0.0f;
        } else {
            const int grp = op.a, half = op.half;
            __syncthreads();                                            // the copies of this workgroup are visible to it
            for (int t = tid; t < GROUP_SPAN; t += WS_THREADS) {
                s_i[t] = d->idat[half][grp * NFFT + t];
                s_q[t] = d->qdat[half][grp * NFFT + t];
            }
            __syncthreads();
            cf x[8], y[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {                               // :172-177
                const int n = l + 64 * j;
                const float wn = window[n];
                x[j] = cf{windowed(s_i[w * HSPS + n], wn), windowed(s_q[w * HSPS + n], wn)};
            }
            kg_radix8<-1>(x, y);                                        // pass 0: Ns = 1
#pragma unroll
            for (int m = 0; m < 8; m++) kg_st(&s_a[w][8 * l + m], y[m]);
            __syncthreads();
            kg_tw7 tw;
#pragma unroll
            for (int j = 0; j < 8; j++) x[j] = kg_ld(&s_a[w][l + 64 * j]);
#pragma unroll
            for (int j = 1; j < 8; j++) tw.w[j - 1] = kg_ld(&tab4096[(j * (l & 7)) << 6]);      // W_64^(j (l mod 8))
            kg_tw_radix8<-1>(x, y, tw);                                 // pass 1: Ns = 8
#pragma unroll
            for (int m = 0; m < 8; m++) kg_st(&s_b[w][(l >> 3) * 64 + (l & 7) + 8 * m], y[m]);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 8; j++) x[j] = kg_ld(&s_b[w][l + 64 * j]);
#pragma unroll
            for (int j = 1; j < 8; j++) tw.w[j - 1] = kg_ld(&tab4096[(j * l) << 3]);            // W_512^(j l)
            kg_tw_radix8<-1>(x, y, tw);                                 // pass 2: Ns = 64, y[m] is bin l + 64 m
            float *plane = d->pwr_samp[half][grp * FPG + w];
#pragma unroll
            for (int m = 0; m < 8; m++) {                               // :191-204: plane row j holds bin unwrap(j)
                const int j = (l + 64 * m + SPS) & (NFFT - 1);
                const float pwr = power(y[m].x, y[m].y);
                s_pw[w][j] = pwr;
                plane[j] = pwr;
            }
            __syncthreads();
            for (int j = tid; j < NFFT; j += WS_THREADS) {              // :205-206, in FFT order
                float avg = d->pwr_sampavg[half][j], sv = 0.0f;
#pragma unroll
                for (int i = 0; i < FPG; i++) { avg += s_pw[i][j]; sv += s_pw[i][j]; }
                d->pwr_sampavg[half][j] = avg;
                d->savg[j] = sv;
                s_savg[j] = sv;
            }
            __syncthreads();
            for (int i = tid; i < NBINS; i += WS_THREADS) s_sm[i] = smooth7(s_savg, i);         // :213 with wspr.cpp:221-229
            __syncthreads();
            ws_noise(s_sm, &s_noise, tid);
            uint8_t *row = rows + op.row_off;
            for (int j = tid; j < NBINS; j += WS_THREADS) row[j + 1] = row_byte(to_db(renorm(s_sm[j], s_noise, min_snr), scaling));
            if (tid == 0) row[0] = (uint8_t) op.b;
            if (tid < KG_WSPR_ROW_STRIDE - (NBINS + 1)) row[NBINS + 1 + tid] = 0;       // a slot is handed out whole: its pad is zeros
            nrows++;
            __syncthreads();
        }
    }
    if (tid == 0) counts[4 * blockIdx.x] = nrows;
}

__global__ __launch_bounds__(WS_THREADS) void wspr_cycle_kernel(const ws_cyc *__restrict__ tab, const ws_dev *__restrict__ dev, kg_wspr_cycle *out, int32_t *counts,
                                                                float min_snr, wd_hold *hold)
{
    __shared__ float s_avg[NFFT];
    __shared__ float s_raw[NBINS + 5], s_sm[NBINS + 5];
    __shared__ float s_noise;
    __shared__ pk_t s_pk[MAX_NPK];
    __shared__ cand_t s_cand[MAX_NPK];
    __shared__ int s_npk;
    __shared__ float s_rt[NFFTS][RT_BINS];
    __shared__ signed char s_ifd[NIFR * NDRIFT][NSYM];                  // ifd - base of (ifr, idrift, k): the double expression of :678 once a triple, not once a hypothesis
    __shared__ float s_best[WS_THREADS];
    __shared__ int s_besth[WS_THREADS];
    const ws_cyc e = tab[blockIdx.y];
    const int tid = (int) threadIdx.x, pki = (int) blockIdx.x;
    const ws_dev *d = dev + e.conn;
    kg_wspr_cycle *res = out + e.slot;
    for (int j = tid; j < NFFT; j += WS_THREADS) s_avg[j] = d->pwr_sampavg[e.half][j];
    __syncthreads();
    for (int i = tid; i < NBINS; i += WS_THREADS) s_raw[i] = smooth7(s_avg, i);
    __syncthreads();
    ws_noise(s_raw, &s_noise, tid);
    for (int j = tid; j < NBINS; j += WS_THREADS) s_sm[j] = renorm(s_raw[j], s_noise, min_snr);
    __syncthreads();
    if (tid == 0) s_npk = peak_list(s_sm, e.more, min_snr, snr_scaling(e.type), s_pk, s_cand);
    __syncthreads();
    const int npk = s_npk;
    if (pki == 0) {
        if (tid == 0) { res->due = 1; res->half = e.half; res->npk = npk; res->pad = 0; counts[4 * e.slot + 1] = 1; counts[4 * e.slot + 2] = npk; }
        if (tid == 0) { hold[e.conn].ncand = npk; hold[e.conn].half = e.half; }
        if (tid < MAX_NPK) {
            pk_t z = {0, 0.0f, 0.0f, 0};
            const pk_t v = tid < npk ? s_pk[tid] : z;
            res->pk[tid].bin0 = v.bin0; res->pk[tid].freq0 = v.freq0; res->pk[tid].snr0 = v.snr0; res->pk[tid].pad = 0;
        }
    }
    if (pki >= npk) {
        if (tid == 0) { kg_wspr_cand z = {0.0f, 0, 0.0f, 0.0f, 0, 0}; res->cand[pki] = z; hold[e.conn].cand[pki] = z; hold[e.conn].ignore[pki] = 0; }
        return;
    }
    const int if0 = if0_of(s_cand[pki].freq0);                          // wspr.cpp:665: before the loops overwrite freq0
    int base = if0 - RT_HALF;
    base = base < 0 ? 0 : base > NFFT - RT_BINS ? NFFT - RT_BINS : base;        // never taken for a bin inside FMIN .. FMAX (if0 is 106 .. 406)
    for (int idx = tid; idx < NFFTS * RT_BINS; idx += WS_THREADS) {     // the roots, once (wspr.cpp:690-693)
        const int t = idx >> 4, o = idx & (RT_BINS - 1);
        s_rt[t][o] = KG_WSPR_SQRT(d->pwr_samp[e.half][t][base + o]);
    }
    for (int idx = tid; idx < NIFR * NDRIFT * NSYM; idx += WS_THREADS) {
        const int a = idx / NSYM, k = idx - a * NSYM;
        s_ifd[a][k] = (signed char) (ifd_of(if0 - 2 + a / NDRIFT, k, -MAXDRIFT + a % NDRIFT) - base);
    }
    __syncthreads();
    auto rt = [&](int bin, int kindex) { return s_rt[kindex][(bin - base) & (RT_BINS - 1)]; };
    float best = -1e30;
    int besth = -1;
    for (int h = tid; h < NHYP; h += WS_THREADS) {
        int ifr, k0, idrift;
        hyp_of(h, if0, &ifr, &k0, &idrift);
        const signed char *row = s_ifd[(ifr - (if0 - 2)) * NDRIFT + idrift + MAXDRIFT];
        const float sync1 = sync_of(rt, [&](int k) { return base + row[k]; }, ws_pr3, k0);
        if (sync1 > best) { best = sync1; besth = h; }                  // :700: a NaN never wins
    }
    s_best[tid] = best; s_besth[tid] = besth;
    __syncthreads();
    for (int m = WS_THREADS / 2; m >= 1; m >>= 1) {                     // the first maximum in loop order: the greatest value, then the least index
        if (tid < m) {
            const float ov = s_best[tid + m];
            const int oh = s_besth[tid + m];
            if (oh >= 0 && (s_besth[tid] < 0 || ov > s_best[tid] || (ov == s_best[tid] && oh < s_besth[tid]))) { s_best[tid] = ov; s_besth[tid] = oh; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        cand_t c = s_cand[pki];
        if (s_besth[0] >= 0) take_hyp(c, s_besth[0], if0, s_best[0]);
        kg_wspr_cand o = {c.freq0, c.shift0, c.drift0, c.sync0, c.freq_idx, c.bin0};
        res->cand[pki] = o;
        hold[e.conn].cand[pki] = o;                                     // stage 2 starts from here, with ignore clear (wspr.cpp:560: the memset)
        hold[e.conn].ignore[pki] = 0;
    }
}

// ---- stage 2 (csrc/kg_wspr_dec.h is the one definition of its arithmetic): one pass of wspr_decode's candidate loop (wspr.cpp:733-883)
// over the held candidates of the listed connections, as a chain of launches on the context's stream with no host read between them:
//   begin    a slot per (list entry, candidate): the held estimates, or inactive (no such candidate, or p->ignore set);
//   six times corr + pick -- the refinement calls of :759-805 -- then corr + soft for ALL jiggles of :819-867 at once, fano, finish.
// corr: one workgroup per (symbol, slot).  The symbol's span of i_data / q_data over every lag of the call goes to LDS once (at most 512
// samples); a lane owns a (tone, hypotheses) pair: it seeds the tone's recurrence (kg_libm_dtrig.h), runs its 255 steps ONCE and adds
// every sample into the float sums of its hypotheses -- the 5 lags of a lag call, or 5 neighbouring jiggles (their samples lie iifac
// apart in LDS); a frequency call's hypotheses differ in the recurrence itself: one each.  The tone's root power goes to the workspace
// [slot][hypothesis][symbol][tone] in double.  pick / soft: a lane per hypothesis sums its 162 symbols IN SYMBOL ORDER (totp in
// double, ss in float: the order is part of the result, no tree), lane 0 takes the first maximum in the order of the reference's loops
// and moves the slot's estimates on; soft makes every jiggle's bytes, rms and gate.  fano: a lane per (slot, jiggle) that passed the
// gate, 32 lanes a workgroup, the 82 nodes of a lane in LDS as [node][lane] words (a lane keeps to its bank; 52 KB a workgroup), the
// branch metrics formed from the symbols and the table (LDS too) where they are needed.  finish: a lane per slot walks the jiggles in
// the reference's order idt = 0, 1, 2 ... to the first whose fano run succeeded and writes the record of that SEQUENTIAL loop.
enum { WD_THREADS = 128, WD_NL = 5, WD_SPAN = 512, WD_SOFT_THREADS = 192, WD_FANO_LANES = 32, WD_CALL_SOFT = 6, WD_MAX_FANO = 4096 };
static_assert(sizeof(wd::rec_t) == sizeof(kg_wspr_dec) && wd::MAX_IDT <= WD_SOFT_THREADS && (wd::MAX_IDT + WD_NL - 1) / WD_NL * 4 <= WD_THREADS, "stage 2 shapes");
static_assert(KG_WSPR_SKIPPED == wd::R_SKIPPED && KG_WSPR_MINSYNC1 == wd::R_MINSYNC1 && KG_WSPR_NO_CHANGE == wd::R_NO_CHANGE && KG_WSPR_TIME_UP == wd::R_TIME_UP &&
              KG_WSPR_DECODED == wd::R_DECODED && KG_WSPR_QUICK_MISS == wd::R_QUICK_MISS, "result classes");

struct wd_slot {                                                        // one candidate's chain
    int32_t conn, pki, half, exists, skipped, active, minsync_ok, pad;  // active: the next call runs; cleared where minsync1 fails
    float f1; int32_t shift1; float drift1, sync1, syncp, syncm;
    float tr_f[wd::NCALLS]; int32_t tr_shift[wd::NCALLS]; float tr_sync[wd::NCALLS];
};
struct wd_jig { float sync, rms; int32_t gate, pad; uint8_t sym[164]; };
struct wd_fano { int32_t ok; uint32_t metric, cycles, maxnp; uint8_t data[12]; };
// the hypotheses of call c: how many, whether they differ in frequency (else in lag), fstep, the first lag and the lag step, the drift's offset
struct wd_call { int32_t nh, freq; float fstep; int32_t lag0, stride; float ddrift; };
__device__ __forceinline__ wd_call wd_call_of(int call, const wd_slot &sl, int iifac, int nidt)
{
    switch (call) {
    case 0: return wd_call{5, 0, 0.0f, sl.shift1 - 128, 64, 0.0f};      // :759-764
    case 1: return wd_call{5, 1, 0.25f, sl.shift1, 0, 0.0f};            // :766-768
    case 2: return wd_call{1, 1, 0.0f, sl.shift1, 0, 0.5f};             // :771-775
    case 3: return wd_call{1, 1, 0.0f, sl.shift1, 0, -0.5f};            // :777-779
    case 4: return wd_call{5, 0, 0.0f, sl.shift1 - 32, 16, 0.0f};       // :798-800
    case 5: return wd_call{5, 1, 0.05f, sl.shift1, 0, 0.0f};            // :803-805
    default: return wd_call{nidt, 0, 0.05f, sl.shift1 - (nidt / 2) * iifac, iifac, 0.0f};     // :819-828, sorted by lag
    }
}
__device__ __forceinline__ float wd_drift_of(const wd_slot &sl, const wd_call &c)
{
    const float d = c.ddrift > 0.0f ? sl.drift1 + 0.5 : c.ddrift < 0.0f ? sl.drift1 - 0.5 : sl.drift1;     // :773, :777
    return d;
}
// the jiggle step idt whose lag is the h-th smallest: m = h - nidt / 2 steps of iifac; an odd idt is the negative side (:820-822)
__device__ __forceinline__ int wd_idt_of_sorted(int h, int nidt) { const int m = h - nidt / 2; return m > 0 ? 2 * m : m < 0 ? -2 * m - 1 : 0; }

__global__ void wspr_dec_begin_kernel(const int32_t *__restrict__ conns, int nslots, const wd_hold *__restrict__ hold, wd_slot *slots)
{
    const int s = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= nslots) return;
    const int conn = conns[s / MAX_NPK], pki = s % MAX_NPK;
    const wd_hold &h = hold[conn];
    wd_slot sl;
    memset(&sl, 0, sizeof sl);
    sl.conn = conn; sl.pki = pki; sl.half = h.half & 1;
    sl.exists = pki < h.ncand;
    sl.skipped = sl.exists && h.ignore[pki] != 0;                       // :740
    sl.active = sl.exists && !sl.skipped;
    const kg_wspr_cand c = h.cand[pki];
    sl.f1 = c.freq0; sl.shift1 = c.shift0; sl.drift1 = c.drift0; sl.sync1 = c.sync0;                         // :745-749
    slots[s] = sl;
}

template <int NL>
__global__ __launch_bounds__(WD_THREADS) void wspr_corr_kernel(const wd_slot *__restrict__ slots, const ws_dev *__restrict__ dev, double *pw, int call, int iifac, int nidt)
{
    __shared__ float s_i[WD_SPAN], s_q[WD_SPAN];
    const wd_slot sl = slots[blockIdx.y];
    if (!sl.active) return;                                             // the whole workgroup
    const wd_call c = wd_call_of(call, sl, iifac, nidt);
    const int i = (int) blockIdx.x, tid = (int) threadIdx.x, tone = tid & 3, grp = tid >> 2;
    const int k0 = c.lag0 + i * SPS;                                    // the first sample of the span
    const int len = (c.nh - 1) * c.stride + SPS;                        // <= 512: 4 * 64 + 256, 128 + 256
    const ws_dev *d = dev + sl.conn;
    for (int t = tid; t < len && t < WD_SPAN; t += WD_THREADS) {
        const int k = k0 + t;
        const bool in = k >= 0 && k < TPOINTS;
        s_i[t] = in ? d->idat[sl.half][k] : 0.0f;
        s_q[t] = in ? d->qdat[sl.half][k] : 0.0f;
    }
    __syncthreads();
    const int h0 = grp * NL;
    if (h0 >= c.nh) return;
    const float f0 = wd::f0_of(sl.f1, c.freq ? h0 - c.nh / 2 : 0, c.fstep);                                   // :88; ifreq = -2 .. 2, or 0
    const float fp = wd::fp_of(f0, wd_drift_of(sl, c), i);
    double cd, sd, cc = 1, ss = 0;
    wd::seed_of(wd::dphi_of(fp, tone), &cd, &sd);
    wd::acc_t ai[NL], aq[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) { ai[l] = 0.0; aq[l] = 0.0; }
    for (int j = 0; j < SPS; j++) {
        if (j) wd::rot_step(cc, ss, cd, sd);
#pragma unroll
        for (int l = 0; l < NL; l++) {
            const int off = (h0 + l) * c.stride + j;                    // a frequency call: stride 0
            if (h0 + l < c.nh && wd::k_used(k0 + off, TPOINTS)) wd::acc_step(ai[l], aq[l], s_i[off], s_q[off], cc, ss);
        }
    }
#pragma unroll
    for (int l = 0; l < NL; l++) {
        const int h = h0 + l;
        if (h < c.nh) {
            const int o = call == WD_CALL_SOFT ? wd_idt_of_sorted(h, nidt) : h;
            pw[(((size_t) blockIdx.y * wd::MAX_IDT + o) * NSYM + i) * 4 + tone] = wd::p_of(ai[l], aq[l]);
        }
    }
}

// calls 0 .. 5: ss of every hypothesis, the first maximum, and what wspr_decode does with it
__global__ __launch_bounds__(64) void wspr_pick_kernel(wd_slot *slots, const double *__restrict__ pw, int call)
{
    __shared__ float s_ss[8];
    wd_slot *sp = slots + blockIdx.x;
    if (!sp->active) return;
    const wd_slot sl = *sp;
    const wd_call c = wd_call_of(call, sl, 1, 1);
    const int h = (int) threadIdx.x;
    if (h < c.nh) {
        const double *p = pw + ((size_t) blockIdx.x * wd::MAX_IDT + h) * NSYM * 4;
        double totp = 0.0;
        float ss = 0.0;
        for (int i = 0; i < NSYM; i++) wd::sym_step(totp, ss, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], ws_pr3[i]);
        s_ss[h] = wd::ss_of(ss, totp);
    }
    __syncthreads();
    if (h != 0) return;
    double syncmax = -1e30;
    int best = -1;
    for (int k = 0; k < c.nh; k++)                                      // ifreq outside, lag inside: a call has one of the two
        if (wd::ss_wins(s_ss[k], syncmax)) { syncmax = s_ss[k]; best = k; }
    const float sync = syncmax;
    const float fbest = best < 0 ? 0.0f : wd::f0_of(sl.f1, c.freq ? best - c.nh / 2 : 0, c.fstep);          // :78-79: silence returns 0.0 and 0
    const int best_shift = best < 0 ? 0 : c.lag0 + best * c.stride;
    sp->f1 = fbest; sp->shift1 = best_shift;                            // :186-188
    sp->tr_f[call] = fbest; sp->tr_shift[call] = best_shift; sp->tr_sync[call] = sync;
    if (call == 2) sp->syncp = sync;
    else if (call == 3) {
        sp->syncm = sync;
        float drift1 = sl.drift1, sync1 = sl.sync1;
        const float driftp = sl.drift1 + 0.5, driftm = sl.drift1 - 0.5;
        if (sl.syncp > sync1) { drift1 = driftp; sync1 = sl.syncp; }   // :781-789
        else if (sync > sync1) { drift1 = driftm; sync1 = sync; }
        sp->drift1 = drift1; sp->sync1 = sync1;
        const int ok = sync1 > KG_WSPR_DEC_MINSYNC1;                        // :795
        sp->minsync_ok = ok;
        if (!ok) sp->active = 0;                                        // the chain ends here; finish reports MINSYNC1
    } else sp->sync1 = sync;
}

// every jiggle of a slot: sync, the bytes, rms, the gate (:826-838)
__global__ __launch_bounds__(WD_SOFT_THREADS) void wspr_soft_kernel(const wd_slot *__restrict__ slots, const double *__restrict__ pw, wd_jig *jig, int nidt)
{
    const int idt = (int) threadIdx.x;
    if (idt >= wd::MAX_IDT) return;
    wd_jig *out = jig + (size_t) blockIdx.x * wd::MAX_IDT + idt;
    if (!slots[blockIdx.x].active || idt >= nidt) { out->gate = 0; return; }
    const double *p = pw + ((size_t) blockIdx.x * wd::MAX_IDT + idt) * NSYM * 4;
    double totp = 0.0;
    float ss = 0.0, fsum = 0.0, f2sum = 0.0;
    for (int i = 0; i < NSYM; i++) {
        wd::sym_step(totp, ss, p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], ws_pr3[i]);
        wd::norm_step(fsum, f2sum, wd::fsymb_of(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], ws_pr3[i]));
    }
    ss = wd::ss_of(ss, totp);
    const float sync = wd::ss_wins(ss, -1e30) ? ss : (float) -1e30;
    const double fac = wd::fac_of(fsum, f2sum);
    float sq = 0.0;
    for (int i = 0; i < NSYM; i++) {
        const uint8_t b = wd::soft_byte(wd::soft_value(wd::fsymb_of(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3], ws_pr3[i]), fac, wd::SYMFAC));
        out->sym[i] = b;
        wd::rms_step(sq, b);
    }
    const float rms = wd::rms_of(sq);
    out->sync = sync; out->rms = rms; out->pad = 0;
    out->gate = wd::gate_of(sync, rms);
}

struct wd_nodes {                                                       // a lane's 82 nodes, [node][lane] in LDS
    uint32_t (*e)[WD_FANO_LANES]; int32_t (*g)[WD_FANO_LANES], (*a)[WD_FANO_LANES], (*b)[WD_FANO_LANES]; uint8_t (*r)[WD_FANO_LANES];
    int lane;
    __device__ uint32_t &enc(int n) { return e[n][lane]; }
    __device__ int32_t &gamma(int n) { return g[n][lane]; }
    __device__ int32_t &tm0(int n) { return a[n][lane]; }
    __device__ int32_t &tm1(int n) { return b[n][lane]; }
    __device__ uint8_t &br(int n) { return r[n][lane]; }
};
// set k: its 162 bytes at sym + k * stride, taken through the deinterleaver where deint; run where gate (null: every set) says so
__global__ __launch_bounds__(WD_FANO_LANES) void wspr_fano_kernel(const uint8_t *__restrict__ sym, size_t stride, const int32_t *__restrict__ gate, size_t gate_stride, int deint,
                                                                  int n, const int32_t *__restrict__ mettab, uint32_t maxcycles, wd_fano *out)
{
    __shared__ int32_t s_met[512];
    __shared__ uint32_t s_e[wd::NNODES][WD_FANO_LANES];
    __shared__ int32_t s_g[wd::NNODES][WD_FANO_LANES], s_a[wd::NNODES][WD_FANO_LANES], s_b[wd::NNODES][WD_FANO_LANES];
    __shared__ uint8_t s_r[wd::NNODES][WD_FANO_LANES];
    __shared__ uint8_t s_sym[NSYM][WD_FANO_LANES];
    __shared__ uint8_t s_perm[NSYM];
    const int lane = (int) threadIdx.x, k = (int) (blockIdx.x * WD_FANO_LANES) + lane;
    for (int t = lane; t < 512; t += WD_FANO_LANES) s_met[t] = mettab[t];
    if (lane == 0) wd::deint_table(s_perm);
    for (int m = 0; m < wd::NNODES; m++) { s_e[m][lane] = 0; s_g[m][lane] = 0; s_a[m][lane] = 0; s_b[m][lane] = 0; s_r[m][lane] = 0; }
    __syncthreads();
    if (k >= n) return;
    wd_fano o;
    memset(&o, 0, sizeof o);
    const bool run = gate == nullptr || *(const int32_t *) ((const char *) gate + (size_t) k * gate_stride) != 0;
    if (run) {
        const uint8_t *src = sym + (size_t) k * stride;
        for (int p = 0; p < NSYM; p++) s_sym[p][lane] = src[deint ? s_perm[p] : p];
        wd_nodes ns = {s_e, s_g, s_a, s_b, s_r, lane};
        o.ok = wd::fano(ns, [&](int p) { return s_sym[p][lane]; }, [&](int a, int v) { return s_met[a * 256 + v]; }, wd::DELTA, maxcycles, &o.metric, &o.cycles, &o.maxnp,
                        o.data);
    }
    out[k] = o;
}

// the record of the sequential loop (:812-883), a lane per slot
__global__ __launch_bounds__(64) void wspr_dec_finish_kernel(const wd_slot *__restrict__ slots, int nslots, const wd_jig *__restrict__ jig, const wd_fano *__restrict__ fano,
                                                             wd_hold *hold, kg_wspr_dec *out_base, int32_t *ncand, int iifac, int nidt, int quickmode,
                                                             int by_conn)
{
    __shared__ uint8_t s_perm[NSYM];
    if (threadIdx.x == 0) wd::deint_table(s_perm);
    __syncthreads();
    const int s = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= nslots) return;
    const wd_slot sl = slots[s];
    kg_wspr_dec *out = by_conn ? out_base + ((size_t) sl.conn * MAX_NPK + sl.pki) - s : out_base;          // out[s]: by list entry, or by connection
    kg_wspr_dec r;
    memset(&r, 0, sizeof r);
    if (sl.pki == 0) ncand[by_conn ? sl.conn : s / MAX_NPK] = hold[sl.conn].ncand;
    if (!sl.exists) { out[s] = r; return; }
    if (sl.skipped) { r.result = KG_WSPR_SKIPPED; r.ignore = 1; out[s] = r; return; }
    for (int c = 0; c < wd::NCALLS; c++) { r.tr_f[c] = sl.tr_f[c]; r.tr_shift[c] = sl.tr_shift[c]; r.tr_sync[c] = sl.tr_sync[c]; }
    r.f1 = sl.f1; r.shift1 = sl.shift1; r.drift1 = sl.drift1; r.sync1 = sl.sync1;
    if (!sl.minsync_ok) {
        r.result = KG_WSPR_MINSYNC1; r.ignore = 1;                      // :807
        hold[sl.conn].ignore[sl.pki] = 1;
        out[s] = r;
        return;
    }
    const wd_jig *jg = jig + (size_t) s * wd::MAX_IDT;
    const wd_fano *fn = fano + (size_t) s * wd::MAX_IDT;
    int idt = 0, last = 0, gates = 0, decoded = 0, lastf = -1;
    while (!decoded && idt < nidt) {                                    // :819
        last = idt;
        if (jg[idt].gate) { gates++; lastf = idt; decoded = fn[idt].ok; }
        idt++;
        if (quickmode) break;
    }
    const bool time_up = !decoded && idt > wd::JIG_RANGE / iifac;       // :869
    r.result = decoded ? KG_WSPR_DECODED : (time_up && gates == 0) ? KG_WSPR_NO_CHANGE : time_up ? KG_WSPR_TIME_UP : KG_WSPR_QUICK_MISS;
    r.ignore = decoded || (time_up && gates == 0);                      // :875, :883
    if (r.ignore) hold[sl.conn].ignore[sl.pki] = 1;
    r.sync1 = jg[last].sync; r.rms = jg[last].rms;
    r.idt = idt; r.ii = wd::ii_of(last, iifac); r.jig_shift = sl.shift1 + r.ii; r.gates = gates;
    if (lastf >= 0) {
        r.metric = fn[lastf].metric; r.cycles = fn[lastf].cycles; r.maxnp = fn[lastf].maxnp;
        for (int k = 0; k < wd::NDATA; k++) r.decdata[k] = fn[lastf].data[k];
    }
    for (int p = 0; p < NSYM; p++) r.symbols[p] = jg[last].sym[jg[last].gate ? s_perm[p] : p];            // deinterleaved only behind the gate (:839)
    out[s] = r;
}

struct ws_conn {
    state_t st;
    std::vector<ev_t> pending;                  // the status changes of commands since the last push (blk -1)
    int decode_on = 0;                          // kg_wspr_set_decode: a cycle end of a push also runs pass 0 (200, 2)
};

// a command's status change waits for the connection's next push; the last WS_PENDING of them are kept (a host that sends commands and
// never pushes must not grow the list, nor a push's events without bound)
static void ws_pend(ws_conn &c, const ev_t &m)
{
    if (c.pending.size() >= WS_PENDING) c.pending.erase(c.pending.begin());
    c.pending.push_back(m);
}

struct kg_wspr {
    kg_ctx *ctx;
    int nconn;
    float min_snr;
    std::vector<ws_conn> c;
    kg_dbuf<ws_dev> d_state;                    // [nconn]
    kg_dbuf<float> d_window;                    // [512], :1186-1188
    // stage 2
    kg_dbuf<wd_hold> d_hold;                    // [nconn]
    kg_dbuf<int32_t> d_mettab;                  // [2][256], the caller's (kg_wspr_set_metric_table)
    bool have_table = false;
    size_t ws_slots = 0;                        // the decode workspace holds this many candidates: grown whole, capacity published last
    kg_dbuf<kg_wspr_dec> d_dec;                 // [nconn][12]: the records of a connection's last pass 0 run by a push (kg_wspr_decodes)
    kg_dbuf<int32_t> d_dec_ncand;               // [nconn]
    kg_dbuf<unsigned char> d_slots, d_jig, d_fano;
    kg_dbuf<double> d_pow;
};

struct ws_plan {
    std::vector<int> conn;                      // the initialised connections of the list, in list order
    std::vector<state_t> st;                    // their states behind the push
    std::vector<ws_entry> ents;
    std::vector<ws_op> ops;
    std::vector<ws_cyc> cyc;
    std::vector<int32_t> dec;                   // the connections whose cycle end also runs pass 0
    std::vector<kg_wspr_row> rows;
    std::vector<kg_wspr_ev> evs;
};

// the decode workspace for nslots candidates: released whole, allocated whole, its capacity published last
static int wd_workspace(kg_wspr *q, size_t nslots, const char *who)
{
    if (nslots <= q->ws_slots) return KG_OK;
    q->ws_slots = 0;
    q->d_slots.reset(); q->d_jig.reset(); q->d_fano.reset(); q->d_pow.reset();
    KG_TRY(q->d_slots.alloc(nslots * sizeof(wd_slot), who));
    KG_TRY(q->d_jig.alloc(nslots * wd::MAX_IDT * sizeof(wd_jig), who));
    KG_TRY(q->d_fano.alloc(nslots * wd::MAX_IDT * sizeof(wd_fano), who));
    KG_TRY(q->d_pow.alloc(nslots * wd::MAX_IDT * NSYM * 4, who));
    q->ws_slots = nslots;
    return KG_OK;
}

// One pass over the held candidates of the listed connections, enqueued on the context's stream: d_conns [nconn] on the device,
// d_out [nconn][12] and d_ncand [nconn] too -- by list entry, or (by_conn) by connection.  Enqueue only; the workspace is sized by the caller.
static int wd_enqueue(kg_wspr *q, const int32_t *d_conns, int nconn, uint32_t maxcycles, int iifac, int quickmode, kg_wspr_dec *d_out, int32_t *d_ncand, int by_conn)
{
    hipStream_t s = q->ctx->stream;
    const int nslots = nconn * MAX_NPK, nidt = wd::nidt_of(iifac, quickmode);
    wd_slot *slots = (wd_slot *) q->d_slots.p;
    wd_jig *jig = (wd_jig *) q->d_jig.p;
    wd_fano *fano = (wd_fano *) q->d_fano.p;
    const ws_dev *dev = q->d_state.p;
    hipLaunchKernelGGL(wspr_dec_begin_kernel, dim3((unsigned) ((nslots + 63) / 64)), dim3(64), 0, s, d_conns, nslots, (const wd_hold *) q->d_hold.p, slots);
    KG_HIP(hipGetLastError());
    for (int call = 0; call < wd::NCALLS; call++) {
        if (call == 0 || call == 4) hipLaunchKernelGGL(wspr_corr_kernel<WD_NL>, dim3(NSYM, (unsigned) nslots), dim3(WD_THREADS), 0, s, (const wd_slot *) slots, dev, q->d_pow.p, call, 1, 1);
        else hipLaunchKernelGGL(wspr_corr_kernel<1>, dim3(NSYM, (unsigned) nslots), dim3(WD_THREADS), 0, s, (const wd_slot *) slots, dev, q->d_pow.p, call, 1, 1);
        KG_HIP(hipGetLastError());
        hipLaunchKernelGGL(wspr_pick_kernel, dim3((unsigned) nslots), dim3(64), 0, s, slots, (const double *) q->d_pow.p, call);
        KG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(wspr_corr_kernel<WD_NL>, dim3(NSYM, (unsigned) nslots), dim3(WD_THREADS), 0, s, (const wd_slot *) slots, dev, q->d_pow.p, (int) WD_CALL_SOFT, iifac, nidt);
    KG_HIP(hipGetLastError());
    hipLaunchKernelGGL(wspr_soft_kernel, dim3((unsigned) nslots), dim3(WD_SOFT_THREADS), 0, s, (const wd_slot *) slots, (const double *) q->d_pow.p, jig, nidt);
    KG_HIP(hipGetLastError());
    const int nf = nslots * wd::MAX_IDT;
    hipLaunchKernelGGL(wspr_fano_kernel, dim3((unsigned) ((nf + WD_FANO_LANES - 1) / WD_FANO_LANES)), dim3(WD_FANO_LANES), 0, s, (const uint8_t *) jig + offsetof(wd_jig, sym),
                       sizeof(wd_jig), (const int32_t *) ((const char *) jig + offsetof(wd_jig, gate)), sizeof(wd_jig), 1, nf, (const int32_t *) q->d_mettab.p, maxcycles, fano);
    KG_HIP(hipGetLastError());
    hipLaunchKernelGGL(wspr_dec_finish_kernel, dim3((unsigned) ((nslots + 63) / 64)), dim3(64), 0, s, (const wd_slot *) slots, nslots, (const wd_jig *) jig,
                       (const wd_fano *) fano, q->d_hold.p, d_out, d_ncand, iifac, nidt, quickmode, by_conn);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

static int ws_walk(kg_wspr *q, const int32_t *conns, int nconn, const int32_t *nblk, const int32_t *in_row, int ns, size_t iq_stride, const int32_t *minute, const int32_t *second,
                   size_t time_stride, size_t rows_cap, int max_rows, int max_events, ws_plan &p, const char *who)
{
    KG_REQUIRE(nconn >= 1 && nconn <= q->nconn, KG_ERR_INVALID, "%s: nconn %d (1..%d)", who, nconn, q->nconn);
    KG_REQUIRE(ns >= 1 && ns <= WS_MAX_NS, KG_ERR_INVALID, "%s: ns %d (1..%d)", who, ns, WS_MAX_NS);
    KG_REQUIRE(max_rows >= 0 && max_events >= 0, KG_ERR_INVALID, "%s: max_rows %d, max_events %d", who, max_rows, max_events);
    std::vector<char> listed((size_t) q->nconn, 0);
    for (int i = 0; i < nconn; i++) {
        const int c = conns[i];
        KG_TRY(kg_ext_list_entry(who, listed, nconn, i, c, nblk[i], WS_MAX_BLK, "iq_stride", iq_stride, (size_t) ns, false, "sample row", in_row ? in_row[i] : 0));
        KG_REQUIRE((size_t) nblk[i] * (size_t) ns <= WS_MAX_SAMPLES, KG_ERR_INVALID, "%s: entry %d has %zu samples (at most %d)", who, i, (size_t) nblk[i] * ns, WS_MAX_SAMPLES);
        KG_REQUIRE(nblk[i] <= 0 || nconn == 1 || time_stride >= (size_t) nblk[i], KG_ERR_INVALID, "%s: time_stride %zu below the %d blocks of entry %d", who, time_stride,
                   nblk[i], i);
        KG_REQUIRE(q->c[c].st.inited, KG_ERR_STATE, "%s: connection %d was never initialised (kg_wspr_init)", who, c);
        for (int b = 0; b < nblk[i]; b++)
            KG_REQUIRE(time_ok(minute[i * time_stride + b], second[i * time_stride + b]), KG_ERR_INVALID, "%s: block %d of entry %d at %d:%d (0..59 each)", who, b, i,
                       minute[i * time_stride + b], second[i * time_stride + b]);
        state_t st = q->c[c].st;
        sched_t sp;
        for (const ev_t &m : q->c[c].pending) p.evs.push_back(kg_wspr_ev{c, -1, 0, m.kind, m.a, m.b});
        for (int b = 0; b < nblk[i]; b++) sched_block(st, sp, b, (int64_t) b * ns, ns, minute[i * time_stride + b], second[i * time_stride + b]);
        KG_REQUIRE(sp.ncycle <= 1, KG_ERR_INVALID, "%s: entry %d completes %d cycles; a push takes at most one (cut it)", who, i, sp.ncycle);
        ws_entry e;
        memset(&e, 0, sizeof e);
        e.conn = c; e.first = (int32_t) p.ops.size(); e.nops = (int32_t) sp.ops.size(); e.type = st.wspr_type; e.dec = st.int_decimate;
        e.in_off = (int64_t) ((size_t) (in_row ? in_row[i] : i) * iq_stride);
        const size_t row0 = p.rows.size();
        for (const op_t &o : sp.ops) {
            ws_op d = {o.kind, o.half, o.a, o.b, o.n, 0, o.kind == OP_COPY ? o.src : 0, 0};
            if (o.kind == OP_GROUP) {
                d.row_off = (int64_t) ((row0 + (size_t) o.c) * KG_WSPR_ROW_STRIDE);
                KG_REQUIRE((size_t) d.row_off + KG_WSPR_ROW_STRIDE <= rows_cap, KG_ERR_INVALID, "%s: more row bytes than the capacity %zu", who, rows_cap);
                KG_REQUIRE(p.rows.size() < (size_t) max_rows, KG_ERR_INVALID, "%s: more rows than max_rows = %d", who, max_rows);
                p.rows.push_back(kg_wspr_row{c, (int32_t) (o.src / ns), (int32_t) (o.src % ns), o.a, o.half, o.b, d.row_off});
            }
            p.ops.push_back(d);
        }
        for (const ev_t &m : sp.evs) {
            p.evs.push_back(kg_wspr_ev{c, m.blk, m.samp, m.kind, m.a, m.b});
            if (m.kind == EV_PEAKS && q->c[c].decode_on) p.evs.push_back(kg_wspr_ev{c, m.blk, m.samp, KG_WSPR_EV_DECODES, m.a, 0});        // between PEAKS and the resume
        }
        KG_REQUIRE(p.evs.size() <= (size_t) max_events, KG_ERR_INVALID, "%s: more events than max_events = %d", who, max_events);
        if (sp.ncycle) p.cyc.push_back(ws_cyc{c, sp.cycle_half, st.wspr_type, st.more_candidates, i, {0, 0, 0}});
        if (sp.ncycle && q->c[c].decode_on) p.dec.push_back(c);
        p.ents.push_back(e);
        p.conn.push_back(c);
        p.st.push_back(st);
    }
    return KG_OK;
}

// A walked push enqueued on device memory, samples and outputs alike: ONE table -- entries, ops, then the cycle ends -- staged ahead of
// the plan pass's return; d_cycles and d_counts (an entry of the list each) are cleared here.  The commit is the last act.  Enqueue only.
static int ws_enqueue(kg_wspr *q, ws_plan &p, int nconn, const float *d_iq, uint8_t *d_rows, kg_wspr_row *row_map, int32_t *nrows, kg_wspr_ev *evs, int32_t *nevents,
                      kg_wspr_cycle *d_cycles, int32_t *d_counts)
{
    hipStream_t s = q->ctx->stream;
    const size_t ne = sizeof(ws_entry) * p.ents.size(), no = sizeof(ws_op) * p.ops.size(), nc = sizeof(ws_cyc) * p.cyc.size(), nd = sizeof(int32_t) * p.dec.size();
    std::vector<unsigned char> tab(ne + no + nc + nd);
    memcpy(tab.data(), p.ents.data(), ne);
    if (no) memcpy(tab.data() + ne, p.ops.data(), no);
    if (nc) memcpy(tab.data() + ne + no, p.cyc.data(), nc);
    if (nd) memcpy(tab.data() + ne + no + nc, p.dec.data(), nd);
    void *d_tab = nullptr;
    KG_TRY(kg_ctx_stage(q->ctx, tab.data(), tab.size(), &d_tab));
    KG_PLAN_ONLY(q->ctx);
    KG_HIP(hipMemsetAsync(d_cycles, 0, sizeof(kg_wspr_cycle) * (size_t) nconn, s));
    KG_HIP(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * 4 * (size_t) nconn, s));
    const unsigned char *t = (const unsigned char *) d_tab;
    hipLaunchKernelGGL(wspr_push_kernel, dim3((unsigned) p.ents.size()), dim3(WS_THREADS), 0, s, (const ws_entry *) t, (const ws_op *) (t + ne), (const float2 *) d_iq,
                       (const float *) q->d_window.p, (const float2 *) q->ctx->d_tab4096, d_rows, d_counts, q->d_state.p, q->min_snr);
    KG_HIP(hipGetLastError());
    if (nc) {
        hipLaunchKernelGGL(wspr_cycle_kernel, dim3(MAX_NPK, (unsigned) p.cyc.size()), dim3(WS_THREADS), 0, s, (const ws_cyc *) (t + ne + no), (const ws_dev *) q->d_state.p,
                           d_cycles, d_counts, q->min_snr, q->d_hold.p);
        KG_HIP(hipGetLastError());
    }
    // pass 0 (wspr.cpp:505, :508) behind the cycle end, on the same stream: no host wait; its workspace is kg_wspr_set_decode's
    if (nd) KG_TRY(wd_enqueue(q, (const int32_t *) (t + ne + no + nc), (int) p.dec.size(), 200, 2, 0, q->d_dec.p, q->d_dec_ncand.p, 1));
    for (size_t k = 0; k < p.conn.size(); k++) { q->c[p.conn[k]].st = p.st[k]; q->c[p.conn[k]].pending.clear(); }       // commit: the enqueue succeeded
    if (row_map && !p.rows.empty()) memcpy(row_map, p.rows.data(), sizeof(kg_wspr_row) * p.rows.size());
    if (evs && !p.evs.empty()) memcpy(evs, p.evs.data(), sizeof(kg_wspr_ev) * p.evs.size());
    *nrows = (int32_t) p.rows.size();
    *nevents = (int32_t) p.evs.size();
    return KG_OK;
}

// kg_wspr_push on device memory, entry i's samples at row in_row[i] of d_iq (null: row i), the outputs on the device too.  Enqueue only.
int kg_wspr_push_rows_(kg_wspr *q, const int32_t *conns, int nconn, const int32_t *nblk, const int32_t *in_row, int ns, const float *d_iq, size_t iq_stride,
                       const int32_t *minute, const int32_t *second, size_t time_stride, uint8_t *d_rows, size_t rows_cap, kg_wspr_row *row_map, int max_rows,
                       int32_t *nrows, kg_wspr_ev *evs, int max_events, int32_t *nevents, kg_wspr_cycle *d_cycles, int32_t *d_counts)
{
    KG_REQUIRE(q && conns && nblk && d_iq && minute && second && d_rows && nrows && nevents && d_cycles && d_counts, KG_ERR_INVALID, "kg_wspr_push: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_REQUIRE(KG_ALIGNED(d_iq, 8) && KG_ALIGNED(d_cycles, 4) && KG_ALIGNED(d_counts, 4), KG_ERR_INVALID,
               "kg_wspr_push: the samples must be 8-byte aligned, cycles and counts 4-byte aligned");
    ws_plan p;
    KG_TRY(ws_walk(q, conns, nconn, nblk, in_row, ns, iq_stride, minute, second, time_stride, rows_cap, max_rows, max_events, p, "kg_wspr_push"));
    return ws_enqueue(q, p, nconn, d_iq, d_rows, row_map, nrows, evs, nevents, d_cycles, d_counts);
}

// the records and counts of the pushes' pass 0, by connection (device memory of the object), for kg_rxbank.hip
void kg_wspr_dec_buffers_(kg_wspr *q, kg_wspr_dec **d_decs, int32_t **d_ncand) { *d_decs = q->d_dec.p; *d_ncand = q->d_dec_ncand.p; }
int kg_wspr_decode_on_(const kg_wspr *q, int conn) { return q->c[conn].decode_on; }

// what the table of a push over nconn connections takes when no connection has more than ops_per_conn ops (and its alignment)
size_t kg_wspr_table_bytes_(size_t nconn, size_t ops_per_conn) { return 64 + nconn * (sizeof(ws_entry) + sizeof(ws_op) * ops_per_conn + sizeof(ws_cyc) + sizeof(int32_t)); }

// connection conn as a new connection finds it: the zeroed object, not initialised, nothing pending.  Enqueue only.
int kg_wspr_reset_(kg_wspr *q, int conn)
{
    KG_REQUIRE(q != nullptr && conn >= 0 && conn < q->nconn, KG_ERR_INVALID, "kg_wspr: connection %d", conn);
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_HIP(hipMemsetAsync(q->d_state.p + conn, 0, sizeof(ws_dev), q->ctx->stream));
    KG_HIP(hipMemsetAsync(q->d_hold.p + conn, 0, sizeof(wd_hold), q->ctx->stream));            // the candidates and their ignore flags
    KG_HIP(hipMemsetAsync(q->d_dec.p + (size_t) conn * MAX_NPK, 0, sizeof(kg_wspr_dec) * MAX_NPK, q->ctx->stream));
    KG_HIP(hipMemsetAsync(q->d_dec_ncand.p + conn, 0, sizeof(int32_t), q->ctx->stream));
    q->c[conn].decode_on = 0;
    memset(&q->c[conn].st, 0, sizeof q->c[conn].st);
    q->c[conn].pending.clear();
    return KG_OK;
}

extern "C" {

int kg_wspr_create(kg_ctx *ctx, int nconn, kg_wspr **out)
{
    return kg_ext_create(ctx, nconn, WS_MAX_CONNS, "kg_wspr_create", "nconn", out, [=](kg_wspr *q) -> int {
        q->nconn = nconn;
        q->min_snr = min_snr_value();
        q->c.resize(nconn);
        for (ws_conn &c : q->c) memset(&c.st, 0, sizeof c.st);
        KG_TRY(q->d_state.alloc((size_t) nconn, "kg_wspr_create: connection state"));
        KG_TRY(q->d_window.alloc(NFFT, "kg_wspr_create: window"));
        KG_TRY(q->d_hold.alloc((size_t) nconn, "kg_wspr_create: held candidates"));
        KG_TRY(q->d_mettab.alloc(512, "kg_wspr_create: metric table"));
        KG_TRY(kg_ext_zero(ctx, q->d_hold.p, (size_t) nconn, "kg_wspr_create"));
        KG_TRY(q->d_dec.alloc((size_t) nconn * MAX_NPK, "kg_wspr_create: decode records"));
        KG_TRY(q->d_dec_ncand.alloc((size_t) nconn, "kg_wspr_create: decode counts"));
        KG_TRY(kg_ext_zero(ctx, q->d_dec.p, (size_t) nconn * MAX_NPK, "kg_wspr_create"));
        KG_TRY(kg_ext_zero(ctx, q->d_dec_ncand.p, (size_t) nconn, "kg_wspr_create"));
        float win[NFFT];
        for (int i = 0; i < NFFT; i++) win[i] = window_at(i);
        KG_HIP(hipMemcpyAsync(q->d_window.p, win, sizeof win, hipMemcpyHostToDevice, ctx->stream));
        KG_HIP(hipStreamSynchronize(ctx->stream));                      // win[] is this frame's
        return kg_ext_zero(ctx, q->d_state.p, (size_t) nconn, "kg_wspr_create");
    });
}

void kg_wspr_destroy(kg_wspr *q) { kg_drain_delete(q); }

#define WS_INITED(who)                                                                               \
    KG_EXT_INDEX(who, q, conn, q->nconn, "connection");                                               \
    KG_REQUIRE(q->c[conn].st.inited, KG_ERR_STATE, who ": connection %d was never initialised (kg_wspr_init)", conn)

int kg_wspr_init(kg_wspr *q, int conn, double snd_rate)
{
    KG_EXT_INDEX("kg_wspr_init", q, conn, q->nconn, "connection");
    state_t st = q->c[conn].st;
    KG_REQUIRE(cmd_init(st, snd_rate) == 0, KG_ERR_INVALID, "kg_wspr_init: snd_rate %g (375 .. 1e9)", snd_rate);
    q->c[conn].st = st;
    ws_pend(q->c[conn], ev_t{-1, 0, EV_STATUS, ST_IDLE, ST_IDLE});
    return KG_OK;
}

int kg_wspr_set_capture(kg_wspr *q, int conn, int capture)
{
    WS_INITED("kg_wspr_set_capture");
    sched_t sp;
    cmd_capture(q->c[conn].st, capture != 0, &sp);
    for (const ev_t &m : sp.evs) ws_pend(q->c[conn], m);
    return KG_OK;
}

int kg_wspr_set_type(kg_wspr *q, int conn, int type)
{
    WS_INITED("kg_wspr_set_type");
    KG_REQUIRE(cmd_type(q->c[conn].st, type) == 0, KG_ERR_INVALID, "kg_wspr_set_type: type %d (2 or 15)", type);
    return KG_OK;
}

int kg_wspr_set_more_candidates(kg_wspr *q, int conn, int on)
{
    WS_INITED("kg_wspr_set_more_candidates");
    q->c[conn].st.more_candidates = on != 0;
    return KG_OK;
}

int kg_wspr_push(kg_wspr *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, const float *iq, size_t iq_stride, const int32_t *minute,
                 const int32_t *second, size_t time_stride, uint8_t *rows, size_t rows_cap, kg_wspr_row *row_map, int max_rows, int32_t *nrows, kg_wspr_ev *evs,
                 int max_events, int32_t *nevents, kg_wspr_cycle *cycles, int32_t *counts)
{
    KG_REQUIRE(q && conns && nblk && iq && minute && second && rows && row_map && nrows && evs && nevents && cycles && counts, KG_ERR_INVALID,
               "kg_wspr_push: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    ws_plan p;                                          // walked (on copies) ahead of the first copy: a push that will be refused enqueues nothing
    KG_TRY(ws_walk(q, conns, nconn, nblk, nullptr, ns, iq_stride, minute, second, time_stride, rows_cap, max_rows, max_events, p, "kg_wspr_push"));
    size_t last = 0;
    for (int i = 0; i < nconn; i++)
        if (nblk[i] > 0) last = (size_t) i * iq_stride + (size_t) ns * nblk[i];
    float *d_iq = nullptr;
    uint8_t *d_rows = nullptr;
    kg_wspr_cycle *d_cycles = nullptr;
    int32_t *d_counts = nullptr;
    hipStream_t s = q->ctx->stream;
    kg_scope tmp(q->ctx);                               // the caller's arrays and the temporaries are in use until it has drained the stream
    KG_TRY(tmp.alloc(&d_iq, 2 * (last ? last : 1), "kg_wspr_push: samples"));
    KG_TRY(tmp.alloc(&d_rows, rows_cap ? rows_cap : 1, "kg_wspr_push: rows"));
    KG_TRY(tmp.alloc(&d_cycles, (size_t) nconn, "kg_wspr_push: cycles"));
    KG_TRY(tmp.alloc(&d_counts, (size_t) 4 * nconn, "kg_wspr_push: counts"));
    for (int i = 0; i < nconn; i++)
        if (nblk[i] > 0)
            KG_HIP(hipMemcpyAsync(d_iq + 2 * (size_t) i * iq_stride, iq + 2 * (size_t) i * iq_stride, sizeof(float) * 2 * ns * (size_t) nblk[i], hipMemcpyHostToDevice, s));
    int32_t n = 0, ne = 0;
    KG_TRY(ws_enqueue(q, p, nconn, d_iq, d_rows, row_map, &n, evs, &ne, d_cycles, d_counts));
    KG_HIP(hipMemcpyAsync(cycles, d_cycles, sizeof(kg_wspr_cycle) * (size_t) nconn, hipMemcpyDeviceToHost, s));
    KG_HIP(hipMemcpyAsync(counts, d_counts, sizeof(int32_t) * 4 * (size_t) nconn, hipMemcpyDeviceToHost, s));
    if (n > 0) {                                        // one copy back, then the rows alone: what lies between them stays the caller's
        std::vector<uint8_t> back((size_t) n * KG_WSPR_ROW_STRIDE);
        KG_HIP(hipMemcpyAsync(back.data(), d_rows, back.size(), hipMemcpyDeviceToHost, s));
        KG_HIP(hipStreamSynchronize(s));
        for (int r = 0; r < n; r++) memcpy(rows + row_map[r].off, back.data() + row_map[r].off, NBINS + 1);
    }
    KG_HIP(hipStreamSynchronize(s));
    *nrows = n;
    *nevents = ne;
    return KG_OK;                                       // tmp drains the stream
}

int kg_wspr_plan(kg_wspr *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, const int32_t *minute, const int32_t *second, size_t time_stride,
                 int32_t *nops, int32_t *nrows, int32_t *nevents, int32_t *ncycles)
{
    KG_REQUIRE(q && conns && nblk && minute && second, KG_ERR_INVALID, "kg_wspr_plan: null argument");
    ws_plan p;
    KG_TRY(ws_walk(q, conns, nconn, nblk, nullptr, ns, ~(size_t) 0 >> 1, minute, second, time_stride, ~(size_t) 0 >> 1, 0x7fffffff, 0x7fffffff, p, "kg_wspr_plan"));
    if (nops) *nops = (int32_t) p.ops.size();
    if (nrows) *nrows = (int32_t) p.rows.size();
    if (nevents) *nevents = (int32_t) p.evs.size();
    if (ncycles) *ncycles = (int32_t) p.cyc.size();
    return KG_OK;
}

int kg_wspr_state(kg_wspr *q, int conn, kg_wspr_info *info, float *pwr_sampavg, float *pwr_samp, float *iq_data)
{
    KG_EXT_INDEX("kg_wspr_state", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const ws_dev *d = q->d_state.p + conn;
    hipStream_t s = q->ctx->stream;
    std::vector<float> planes;
    if (pwr_sampavg) KG_HIP(hipMemcpyAsync(pwr_sampavg, d->pwr_sampavg, sizeof(float) * 2 * NFFT, hipMemcpyDeviceToHost, s));
    if (pwr_samp) {
        planes.resize((size_t) 2 * NT * NFFT);
        KG_HIP(hipMemcpyAsync(planes.data(), d->pwr_samp, sizeof(float) * planes.size(), hipMemcpyDeviceToHost, s));
    }
    if (iq_data) {
        KG_HIP(hipMemcpyAsync(iq_data, d->idat, sizeof(float) * 2 * TPOINTS, hipMemcpyDeviceToHost, s));
        KG_HIP(hipMemcpyAsync(iq_data + 2 * TPOINTS, d->qdat, sizeof(float) * 2 * TPOINTS, hipMemcpyDeviceToHost, s));
    }
    KG_HIP(hipStreamSynchronize(s));
    if (pwr_samp)                                       // handed out as the reference has it: [half][j][i]
        for (int h = 0; h < 2; h++)
            for (int i = 0; i < NT; i++)
                for (int j = 0; j < NFFT; j++) pwr_samp[((size_t) h * NFFT + j) * NT + i] = planes[((size_t) h * NT + i) * NFFT + j];
    if (info) {
        const state_t &w = q->c[conn].st;
        memset(info, 0, sizeof *info);
        info->inited = w.inited; info->capture = w.capture; info->reset = w.reset; info->tsync = w.tsync; info->ping_pong = w.ping_pong;
        info->fft_ping_pong = w.fft_ping_pong; info->decode_ping_pong = w.decode_ping_pong; info->decim = w.decim; info->didx = w.didx; info->group = w.group;
        info->status = w.status; info->status_resume = w.status_resume; info->last_sec = w.last_sec; info->abort_decode = w.abort_decode;
        info->wspr_type = w.wspr_type; info->more_candidates = w.more_candidates; info->int_decimate = w.int_decimate; info->cycles = w.cycles;
        info->snd_rate = w.snd_rate;
    }
    return KG_OK;
}

int kg_wspr_load(kg_wspr *q, int conn, int half, const float *pwr_samp, const float *pwr_sampavg, kg_wspr_cycle *cycle)
{
    WS_INITED("kg_wspr_load");
    KG_REQUIRE(half == 0 || half == 1, KG_ERR_INVALID, "kg_wspr_load: half %d (0..1)", half);
    KG_REQUIRE(pwr_samp && pwr_sampavg && cycle, KG_ERR_INVALID, "kg_wspr_load: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    ws_dev *d = q->d_state.p + conn;
    hipStream_t s = q->ctx->stream;
    std::vector<float> planes((size_t) NT * NFFT);
    for (int i = 0; i < NT; i++)
        for (int j = 0; j < NFFT; j++) planes[(size_t) i * NFFT + j] = pwr_samp[(size_t) j * NT + i];
    kg_wspr_cycle *d_cycle = nullptr;
    int32_t *d_counts = nullptr;
    kg_scope tmp(q->ctx);
    KG_TRY(tmp.alloc(&d_cycle, 1, "kg_wspr_load: cycle"));
    KG_TRY(tmp.alloc(&d_counts, 4, "kg_wspr_load: counts"));
    KG_HIP(hipMemcpyAsync(d->pwr_samp[half], planes.data(), sizeof(float) * planes.size(), hipMemcpyHostToDevice, s));
    KG_HIP(hipMemcpyAsync(d->pwr_sampavg[half], pwr_sampavg, sizeof(float) * NFFT, hipMemcpyHostToDevice, s));
    KG_HIP(hipMemsetAsync(d_cycle, 0, sizeof(kg_wspr_cycle), s));
    KG_HIP(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * 4, s));
    const state_t &w = q->c[conn].st;
    const ws_cyc cyc = {conn, half, w.wspr_type, w.more_candidates, 0, {0, 0, 0}};
    void *d_tab = nullptr;
    KG_TRY(kg_ctx_stage(q->ctx, &cyc, sizeof cyc, &d_tab));
    hipLaunchKernelGGL(wspr_cycle_kernel, dim3(MAX_NPK, 1), dim3(WS_THREADS), 0, s, (const ws_cyc *) d_tab, (const ws_dev *) q->d_state.p, d_cycle, d_counts, q->min_snr, q->d_hold.p);
    KG_HIP(hipGetLastError());
    KG_HIP(hipMemcpyAsync(cycle, d_cycle, sizeof(kg_wspr_cycle), hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    q->c[conn].st.decode_ping_pong = half;
    return KG_OK;                                       // tmp drains the stream
}

// ---- stage 2
int kg_wspr_set_metric_table(kg_wspr *q, const int32_t mettab[2][256])
{
    KG_REQUIRE(q != nullptr && mettab != nullptr, KG_ERR_INVALID, "kg_wspr_set_metric_table: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    for (int i = 0; i < 512; i++)
        KG_REQUIRE(mettab[i >> 8][i & 255] <= wd::MAX_METRIC && mettab[i >> 8][i & 255] >= -wd::MAX_METRIC, KG_ERR_INVALID,
                   "kg_wspr_set_metric_table: mettab[%d][%d] = %d (within +-%d)", i >> 8, i & 255, mettab[i >> 8][i & 255], (int) wd::MAX_METRIC);
    KG_HIP(hipMemcpyAsync(q->d_mettab.p, mettab, sizeof(int32_t) * 512, hipMemcpyHostToDevice, q->ctx->stream));
    KG_HIP(hipStreamSynchronize(q->ctx->stream));       // mettab is the caller's
    q->have_table = true;
    return KG_OK;
}

int kg_wspr_load_iq(kg_wspr *q, int conn, int half, const float *i_data, const float *q_data, const kg_wspr_cand *cands, int ncand)
{
    WS_INITED("kg_wspr_load_iq");
    KG_REQUIRE(half == 0 || half == 1, KG_ERR_INVALID, "kg_wspr_load_iq: half %d (0..1)", half);
    KG_REQUIRE(i_data && q_data && (cands || ncand == 0), KG_ERR_INVALID, "kg_wspr_load_iq: null argument");
    KG_REQUIRE(ncand >= 0 && ncand <= MAX_NPK, KG_ERR_INVALID, "kg_wspr_load_iq: ncand %d (0..%d)", ncand, (int) MAX_NPK);
    wd_hold h;
    memset(&h, 0, sizeof h);
    h.ncand = ncand; h.half = half;
    for (int c = 0; c < ncand; c++) {                   // every dphi of the refinement stays inside kg_libm_dtrig.h's domain
        KG_REQUIRE(fabsf(cands[c].freq0) <= 113.0f && cands[c].shift0 >= -TPOINTS && cands[c].shift0 <= TPOINTS && fabsf(cands[c].drift0) <= 4.0f, KG_ERR_INVALID,
                   "kg_wspr_load_iq: candidate %d: freq0 %g (+-113), shift0 %d (+-%d), drift0 %g (+-4)", c, (double) cands[c].freq0, cands[c].shift0, (int) TPOINTS,
                   (double) cands[c].drift0);
        h.cand[c] = cands[c];
    }
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    ws_dev *d = q->d_state.p + conn;
    hipStream_t s = q->ctx->stream;
    KG_HIP(hipMemcpyAsync(d->idat[half], i_data, sizeof(float) * TPOINTS, hipMemcpyHostToDevice, s));
    KG_HIP(hipMemcpyAsync(d->qdat[half], q_data, sizeof(float) * TPOINTS, hipMemcpyHostToDevice, s));
    KG_HIP(hipMemcpyAsync(q->d_hold.p + conn, &h, sizeof h, hipMemcpyHostToDevice, s));
    KG_HIP(hipStreamSynchronize(s));                    // the arrays are the caller's, h this frame's; the schedule's state (st) is not touched
    return KG_OK;
}

int kg_wspr_decode(kg_wspr *q, const int32_t *conns, int nconn, uint32_t maxcycles, int iifac, int quickmode, kg_wspr_dec *out, int32_t *ncand)
{
    KG_REQUIRE(q && conns && out && ncand, KG_ERR_INVALID, "kg_wspr_decode: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_REQUIRE(q->have_table, KG_ERR_STATE, "kg_wspr_decode: no metric table yet (kg_wspr_set_metric_table)");
    KG_REQUIRE(nconn >= 1 && nconn <= q->nconn, KG_ERR_INVALID, "kg_wspr_decode: nconn %d (1..%d)", nconn, q->nconn);
    KG_REQUIRE(iifac >= 1 && iifac <= wd::JIG_RANGE, KG_ERR_INVALID, "kg_wspr_decode: iifac %d (1..%d)", iifac, (int) wd::JIG_RANGE);
    KG_REQUIRE(maxcycles >= 1 && maxcycles <= (uint32_t) wd::MAX_MAXCYCLES, KG_ERR_INVALID, "kg_wspr_decode: maxcycles %u (1..%d)", maxcycles, (int) wd::MAX_MAXCYCLES);
    std::vector<char> listed((size_t) q->nconn, 0);
    for (int i = 0; i < nconn; i++) {
        const int c = conns[i];
        KG_REQUIRE(c >= 0 && c < q->nconn, KG_ERR_INVALID, "kg_wspr_decode: conns[%d] = %d of %d", i, c, q->nconn);
        KG_REQUIRE(!listed[c], KG_ERR_INVALID, "kg_wspr_decode: connection %d is listed twice", c);
        listed[c] = 1;
        KG_REQUIRE(q->c[c].st.inited, KG_ERR_STATE, "kg_wspr_decode: connection %d was never initialised (kg_wspr_init)", c);
    }
    const size_t nslots = (size_t) nconn * MAX_NPK;
    KG_TRY(wd_workspace(q, nslots, "kg_wspr_decode: workspace"));
    hipStream_t s = q->ctx->stream;
    kg_wspr_dec *d_out = nullptr;
    int32_t *d_ncand = nullptr;
    void *d_conns = nullptr;
    kg_scope tmp(q->ctx);                               // out and ncand are in use until the stream has drained
    KG_TRY(tmp.alloc(&d_out, nslots, "kg_wspr_decode: records"));
    KG_TRY(tmp.alloc(&d_ncand, (size_t) nconn, "kg_wspr_decode: counts"));
    KG_TRY(kg_ctx_stage(q->ctx, conns, sizeof(int32_t) * (size_t) nconn, &d_conns));
    KG_TRY(wd_enqueue(q, (const int32_t *) d_conns, nconn, maxcycles, iifac, quickmode != 0, d_out, d_ncand, 0));
    KG_HIP(hipMemcpyAsync(out, d_out, sizeof(kg_wspr_dec) * nslots, hipMemcpyDeviceToHost, s));
    KG_HIP(hipMemcpyAsync(ncand, d_ncand, sizeof(int32_t) * (size_t) nconn, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    return KG_OK;                                       // tmp drains the stream
}

int kg_wspr_set_decode(kg_wspr *q, int conn, int on)
{
    WS_INITED("kg_wspr_set_decode");
    if (on) {
        KG_REQUIRE(q->have_table, KG_ERR_STATE, "kg_wspr_set_decode: no metric table yet (kg_wspr_set_metric_table)");
        int rc = kg_ctx_use(q->ctx);
        if (rc) return rc;
        if ((size_t) q->nconn * MAX_NPK > q->ws_slots) KG_HIP(hipStreamSynchronize(q->ctx->stream));       // a pass under way still reads the workspace that grows
        KG_TRY(wd_workspace(q, (size_t) q->nconn * MAX_NPK, "kg_wspr_set_decode: workspace"));             // a push must not allocate
    }
    q->c[conn].decode_on = on != 0;
    return KG_OK;
}

int kg_wspr_decodes(kg_wspr *q, int conn, kg_wspr_dec *out, int32_t *ncand)
{
    KG_EXT_INDEX("kg_wspr_decodes", q, conn, q->nconn, "connection");
    KG_REQUIRE(out && ncand, KG_ERR_INVALID, "kg_wspr_decodes: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    hipStream_t s = q->ctx->stream;
    KG_HIP(hipMemcpyAsync(out, q->d_dec.p + (size_t) conn * MAX_NPK, sizeof(kg_wspr_dec) * MAX_NPK, hipMemcpyDeviceToHost, s));
    KG_HIP(hipMemcpyAsync(ncand, q->d_dec_ncand.p + conn, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    return KG_OK;
}

int kg_wspr_fano(kg_wspr *q, const uint8_t *symbols, int n, uint32_t maxcycles, int32_t *ok, uint32_t *metric, uint32_t *cycles, uint32_t *maxnp,
                 uint8_t *data)
{
    KG_REQUIRE(q && symbols && ok && metric && cycles && maxnp && data, KG_ERR_INVALID, "kg_wspr_fano: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_REQUIRE(q->have_table, KG_ERR_STATE, "kg_wspr_fano: no metric table yet (kg_wspr_set_metric_table)");
    KG_REQUIRE(n >= 1 && n <= WD_MAX_FANO, KG_ERR_INVALID, "kg_wspr_fano: n %d (1..%d)", n, (int) WD_MAX_FANO);
    KG_REQUIRE(maxcycles >= 1 && maxcycles <= (uint32_t) wd::MAX_MAXCYCLES, KG_ERR_INVALID, "kg_wspr_fano: maxcycles %u (1..%d)", maxcycles, (int) wd::MAX_MAXCYCLES);
    hipStream_t s = q->ctx->stream;
    uint8_t *d_sym = nullptr;
    wd_fano *d_res = nullptr;
    kg_scope tmp(q->ctx);
    KG_TRY(tmp.alloc(&d_sym, (size_t) n * NSYM, "kg_wspr_fano: symbols"));
    KG_TRY(tmp.alloc(&d_res, (size_t) n, "kg_wspr_fano: results"));
    KG_HIP(hipMemcpyAsync(d_sym, symbols, (size_t) n * NSYM, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(wspr_fano_kernel, dim3((unsigned) ((n + WD_FANO_LANES - 1) / WD_FANO_LANES)), dim3(WD_FANO_LANES), 0, s, (const uint8_t *) d_sym, (size_t) NSYM,
                       (const int32_t *) nullptr, (size_t) 0, 0, n, (const int32_t *) q->d_mettab.p, maxcycles, d_res);
    KG_HIP(hipGetLastError());
    std::vector<wd_fano> res((size_t) n);
    KG_HIP(hipMemcpyAsync(res.data(), d_res, sizeof(wd_fano) * (size_t) n, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < n; k++) {
        ok[k] = res[k].ok; metric[k] = res[k].metric; cycles[k] = res[k].cycles; maxnp[k] = res[k].maxnp;
        memcpy(data + (size_t) k * wd::NDATA, res[k].data, wd::NDATA);
    }
    return KG_OK;                                       // tmp drains the stream
}

}  // extern "C"
