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
// ifr, k0, idrift wins by a reduction on (sync1, hypothesis index).
#include "kg_ext.h"
#include "kg_fft.h"
#include "kg_wspr.h"

using namespace kg_wspr_cf;

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
                                                                float min_snr)
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
        if (tid < MAX_NPK) {
            pk_t z = {0, 0.0f, 0.0f, 0};
            const pk_t v = tid < npk ? s_pk[tid] : z;
            res->pk[tid].bin0 = v.bin0; res->pk[tid].freq0 = v.freq0; res->pk[tid].snr0 = v.snr0; res->pk[tid].pad = 0;
        }
    }
    if (pki >= npk) {
        if (tid == 0) { kg_wspr_cand z = {0.0f, 0, 0.0f, 0.0f, 0, 0}; res->cand[pki] = z; }
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
    }
}

struct ws_conn {
    state_t st;
    std::vector<ev_t> pending;                  // the status changes of commands since the last push (blk -1)
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
};

struct ws_plan {
    std::vector<int> conn;                      // the initialised connections of the list, in list order
    std::vector<state_t> st;                    // their states behind the push
    std::vector<ws_entry> ents;
    std::vector<ws_op> ops;
    std::vector<ws_cyc> cyc;
    std::vector<kg_wspr_row> rows;
    std::vector<kg_wspr_ev> evs;
};

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
        for (const ev_t &m : sp.evs) p.evs.push_back(kg_wspr_ev{c, m.blk, m.samp, m.kind, m.a, m.b});
        KG_REQUIRE(p.evs.size() <= (size_t) max_events, KG_ERR_INVALID, "%s: more events than max_events = %d", who, max_events);
        if (sp.ncycle) p.cyc.push_back(ws_cyc{c, sp.cycle_half, st.wspr_type, st.more_candidates, i, {0, 0, 0}});
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
    const size_t ne = sizeof(ws_entry) * p.ents.size(), no = sizeof(ws_op) * p.ops.size(), nc = sizeof(ws_cyc) * p.cyc.size();
    std::vector<unsigned char> tab(ne + no + nc);
    memcpy(tab.data(), p.ents.data(), ne);
    if (no) memcpy(tab.data() + ne, p.ops.data(), no);
    if (nc) memcpy(tab.data() + ne + no, p.cyc.data(), nc);
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
                           d_cycles, d_counts, q->min_snr);
        KG_HIP(hipGetLastError());
    }
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

// what the table of a push over nconn connections takes when no connection has more than ops_per_conn ops (and its alignment)
size_t kg_wspr_table_bytes_(size_t nconn, size_t ops_per_conn) { return 64 + nconn * (sizeof(ws_entry) + sizeof(ws_op) * ops_per_conn + sizeof(ws_cyc)); }

// connection conn as a new connection finds it: the zeroed object, not initialised, nothing pending.  Enqueue only.
int kg_wspr_reset_(kg_wspr *q, int conn)
{
    KG_REQUIRE(q != nullptr && conn >= 0 && conn < q->nconn, KG_ERR_INVALID, "kg_wspr: connection %d", conn);
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_HIP(hipMemsetAsync(q->d_state.p + conn, 0, sizeof(ws_dev), q->ctx->stream));
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
    hipLaunchKernelGGL(wspr_cycle_kernel, dim3(MAX_NPK, 1), dim3(WS_THREADS), 0, s, (const ws_cyc *) d_tab, (const ws_dev *) q->d_state.p, d_cycle, d_counts, q->min_snr);
    KG_HIP(hipGetLastError());
    KG_HIP(hipMemcpyAsync(cycle, d_cycle, sizeof(kg_wspr_cycle), hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    q->c[conn].st.decode_ping_pong = half;
    return KG_OK;                                       // tmp drains the stream
}

}  // extern "C"
