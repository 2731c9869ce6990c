// kg_nb.hip -- the standard noise blanker (NB_STD): CNoiseProc::ProcessBlanker (rx/CuteSDR/noiseproc.cpp:147-203) on gfx950.
//
// Call sites replaced:
//   audio      rx/rx_sound.cpp:593-598  m_NoiseProc_snd[ch].ProcessBlanker(ns_in, in_samps_c, in_samps_c), in place, before CFastFIR
//   waterfall  rx/rx_waterfall.cpp:1087-1099  m_NoiseProc_wf[ch].ProcessBlankerOneShot(8192, hw_c_samps, hw_c_samps) on the
//              windowed frame of sample_wf() (:1049-1066), before compute_frame()  (the pre-pass of kg_wf.hip's frame kernel)
//
// Only the running sum is serial.  One 256-thread workgroup per channel walks its stream in tiles of NB_T samples:
//   1. the tile's inputs into LDS behind the delay ring, their magnitudes behind the magnitude ring -- across lanes;
//   2. the sum walk (two dependent float adds per sample, kg_nbk::sum_walk) on lane 0, its operands read from LDS eight samples at
//      a time ahead of the adds, the sums written back eight at a time; then the trigger test (kg_nbk::trigger) across lanes;
//   3. the gate: sample i is zero iff i - last(i) < G, last(i) the index of the latest trigger at or before i (or, before the first
//      one, the counter carried in as a virtual trigger at cnt - G) -- a prefix-max scan across lanes;
//   4. the output, the delayed sample or zero, across lanes.
// Nothing is reassociated: the sum walk is the reference's loop; the rest is exact (max, compares, copies).
#include "kg_common.h"
#include "kg_nb.h"

#include <math.h>
#include <new>
#include <vector>

#define NB_T 2048                          // samples per tile
#define NB_MAG_STRIDE 1032                 // >= kg_nbk::MAG_RING, floats per channel
#define NB_DLY_STRIDE 2056                 // >= kg_nbk::DLY_RING, complex samples per channel

struct nb_lds {
    float m[kg_nbk::MAG_RING + NB_T];       // the magnitude ring (oldest first), then the tile's magnitudes
    float2 x[kg_nbk::DLY_RING + NB_T];      // the delay ring (oldest first), then the tile's inputs
    float sum[NB_T];                       // the running sum after each sample of the tile
    int wmax[4];
};

// The stream of one channel: `len` samples, sample p read by load(p) and its output handed to store(p, v).
template <class Load, class Store>
__device__ __forceinline__ void nb_run(nb_lds &L, kg_nbk::st *gst, float *gmag, float2 *gdly, long len, Load load, Store store)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const kg_nbk::st s = *gst;
    const int M1 = s.M + 1, D1 = s.D + 1;
    for (int k = t; k < M1; k += 256) { int r = s.mptr + k; if (r >= M1) r -= M1; L.m[k] = gmag[r]; }
    for (int k = t; k < D1; k += 256) { int r = s.dptr + k; if (r >= D1) r -= D1; L.x[k] = gdly[r]; }
    float sum = s.sum;                     // lane 0's
    long last = (long) s.cnt - s.G;        // the counter carried in, as a trigger cnt - G samples before the stream
    for (long base = 0; base < len; base += NB_T) {
        const int nt = (int) (len - base < NB_T ? len - base : NB_T);
        __syncthreads();
        for (int k = t; k < nt; k += 256) {
            const float2 v = load(base + k);
            L.x[D1 + k] = v;
            L.m[M1 + k] = kg_nbk::mag(v.x, v.y);
        }
        __syncthreads();
        if (t == 0) {
            int k = 0;
            for (; k + 8 <= nt; k += 8) {
                float o[8], w[8], sv[8];
#pragma unroll
                for (int j = 0; j < 8; j++) { o[j] = L.m[k + j]; w[j] = L.m[M1 + k + j]; }
#pragma unroll
                for (int j = 0; j < 8; j++) { kg_nbk::sum_walk(sum, o[j], w[j]); sv[j] = sum; }
#pragma unroll
                for (int j = 0; j < 8; j++) L.sum[k + j] = sv[j];
            }
            for (; k < nt; k++) { kg_nbk::sum_walk(sum, L.m[k], L.m[M1 + k]); L.sum[k] = sum; }
        }
        __syncthreads();
        // prefix max of the trigger indices: eight consecutive samples per lane, then across lanes and waves
        int loc[8], run = -1;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int i = 8 * t + j;
            const int v = (i < nt && kg_nbk::trigger(L.m[M1 + i], s.ratio, L.sum[i])) ? i : -1;
            run = v > run ? v : run;
            loc[j] = run;
        }
        int incl = run;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off);
            if (lane >= off) incl = y > incl ? y : incl;
        }
        if (lane == 63) L.wmax[wave] = incl;
        int excl = __shfl_up(incl, 1);
        if (lane == 0) excl = -1;
        __syncthreads();
        for (int w = 0; w < wave; w++) excl = L.wmax[w] > excl ? L.wmax[w] : excl;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int i = 8 * t + j;
            if (i < nt) {
                const int r = loc[j] > excl ? loc[j] : excl;
                const long lst = r >= 0 ? base + r : last;
                const float2 v = (base + i) - lst < (long) s.G ? make_float2(0.0f, 0.0f) : L.x[i];
                store(base + i, v);
            }
        }
        int tmax = -1;
        for (int w = 0; w < 4; w++) tmax = L.wmax[w] > tmax ? L.wmax[w] : tmax;
        if (tmax >= 0) last = base + tmax;
        __syncthreads();
        // the rings move on by nt: their newest M + 1 / D + 1 entries to the front
        float mv[5];
        float2 xv[9];
#pragma unroll
        for (int q = 0; q < 5; q++) { const int k = t + 256 * q; if (k < M1) mv[q] = L.m[nt + k]; }
#pragma unroll
        for (int q = 0; q < 9; q++) { const int k = t + 256 * q; if (k < D1) xv[q] = L.x[nt + k]; }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 5; q++) { const int k = t + 256 * q; if (k < M1) L.m[k] = mv[q]; }
#pragma unroll
        for (int q = 0; q < 9; q++) { const int k = t + 256 * q; if (k < D1) L.x[k] = xv[q]; }
    }
    __syncthreads();
    const int mend = (int) ((s.mptr + len) % M1), dend = (int) ((s.dptr + len) % D1);
    for (int k = t; k < M1; k += 256) { int r = mend + k; if (r >= M1) r -= M1; gmag[r] = L.m[k]; }
    for (int k = t; k < D1; k += 256) { int r = dend + k; if (r >= D1) r -= D1; gdly[r] = L.x[k]; }
    if (t == 0) {
        kg_nbk::st n = s;
        n.mptr = mend; n.dptr = dend;
        const long c = (long) s.G - len + last;
        n.cnt = c > 0 ? (int) c : 0;
        n.sum = sum;
        *gst = n;
    }
}

// ProcessBlanker on row `row` of in / out, one workgroup per listed channel (in == out allowed: a tile is read before it is written,
// and the delayed samples come from LDS)
__global__ __launch_bounds__(256) void nb_audio_kernel(const int *__restrict__ list, const int *__restrict__ nlist, const float2 *in,
                                                       long in_stride, float2 *out, long out_stride, kg_nbk::st *S, float *mag,
                                                       float2 *dly, int by_chan)
{
    __shared__ nb_lds L;
    const int i = blockIdx.x, ch = list[i], n = nlist[i];
    if (n == 0) return;
    const long row = by_chan ? ch : i;                    // kg_ctx::rows_by_chan
    const float2 *src = in + row * in_stride;
    float2 *dst = out + row * out_stride;
    nb_run(L, S + ch, mag + (size_t) ch * NB_MAG_STRIDE, dly + (size_t) ch * NB_DLY_STRIDE, (long) n,
           [&](long p) { return src[p]; }, [&](long p, float2 v) { dst[p] = v; });
}

// The waterfall's pre-pass: one workgroup per blanked channel walks that channel's frames in list order, each frame the windowed
// samples of sample_wf() (fi = (float) ii * window[sn], :1054-1061) and D zeros through one stream (ProcessBlankerOneShot); the
// outputs from sample D of each frame's stream on are the blanked frame.
struct nb_wf_chan { int ch, first, count, wfn; };
struct nb_wf_frame { unsigned off; int slot; };          // the frame's first iq_t in d_iq; its row of d_out (8192 complex floats)

__global__ __launch_bounds__(256) void nb_wf_kernel(const short2 *__restrict__ iq, const nb_wf_chan *__restrict__ chl,
                                                    const nb_wf_frame *__restrict__ fl, const float *__restrict__ windows,
                                                    kg_nbk::st *S, float *mag, float2 *dly, float2 *__restrict__ out)
{
    __shared__ nb_lds L;
    const nb_wf_chan c = chl[blockIdx.x];
    const int D = S[c.ch].D;
    const long per = kg_nbk::WF_NSAMPS + D;
    const float *win = windows + (size_t) c.wfn * kg_nbk::WF_NSAMPS;
    const nb_wf_frame *mine = fl + c.first;
    nb_run(L, S + c.ch, mag + (size_t) c.ch * NB_MAG_STRIDE, dly + (size_t) c.ch * NB_DLY_STRIDE, (long) c.count * per,
           [&](long p) {
               const long f = p / per, r = p - f * per;
               if (r >= kg_nbk::WF_NSAMPS) return make_float2(0.0f, 0.0f);
               const short2 v = iq[(size_t) mine[f].off + r];
               const float w = win[r];
               return make_float2(((float) v.x) * w, ((float) v.y) * w);
           },
           [&](long p, float2 v) {
               const long f = p / per, r = p - f * per;
               if (r >= D) out[(size_t) mine[f].slot * kg_nbk::WF_NSAMPS + (r - D)] = v;
           });
}

// SetupBlanker's reset in stream order: both rings zeroed, the derived state stored
__global__ __launch_bounds__(256) void nb_reset_kernel(kg_nbk::st *S, float *mag, float2 *dly, kg_nbk::st v)
{
    for (int k = threadIdx.x; k < NB_MAG_STRIDE; k += 256) mag[k] = 0.0f;
    for (int k = threadIdx.x; k < NB_DLY_STRIDE; k += 256) dly[k] = make_float2(0.0f, 0.0f);
    if (threadIdx.x == 0) *S = v;
}

// ---------------------------------------------------------------------------
struct kg_nb_store {
    int nchan;
    kg_dbuf<kg_nbk::st> d_st;
    kg_dbuf<float> d_mag;
    kg_dbuf<float2> d_dly;
    std::vector<kg_nbk::st> h;                 // the derived M, D, G, ratio of each channel's last setup
    std::vector<char> was;                    // set up at least once
};

static int nb_store_init(kg_nb_store *s, int nchan)
{
    s->nchan = nchan;
    s->h.assign(nchan, kg_nbk::st{});
    s->was.assign(nchan, 0);
    KG_TRY(s->d_st.alloc(nchan, "kg_nb: states"));
    KG_TRY(s->d_mag.alloc(NB_MAG_STRIDE * (size_t) nchan, "kg_nb: magnitudes"));
    return s->d_dly.alloc(NB_DLY_STRIDE * (size_t) nchan, "kg_nb: delay lines");
}

int kg_nb_store_create(int nchan, kg_nb_store **out)
{
    *out = nullptr;
    kg_nb_store *s = new (std::nothrow) kg_nb_store();
    KG_REQUIRE(s != nullptr, KG_ERR_NOMEM, "kg_nb: alloc");
    const int rc = nb_store_init(s, nchan);
    if (rc) { kg_nb_store_destroy(s); return rc; }
    *out = s;
    return KG_OK;
}

void kg_nb_store_destroy(kg_nb_store *s) { delete s; }

int kg_nb_store_was_setup(const kg_nb_store *s, int ch) { return s->was[ch]; }

int kg_nb_store_setup(kg_ctx *ctx, kg_nb_store *s, int ch, float sample_rate, const float *nb_param, const char *who)
{
    KG_REQUIRE(nb_param != nullptr, KG_ERR_INVALID, "%s: null argument", who);
    KG_REQUIRE(ch >= 0 && ch < s->nchan, KG_ERR_INVALID, "%s: channel %d (0..%d)", who, ch, s->nchan - 1);
    kg_nbk::st v = s->h[ch];
    const int r = kg_nbk::setup(v, s->was[ch] != 0, sample_rate, nb_param);
    KG_REQUIRE(r != kg_nbk::SETUP_BAD_GATE, KG_ERR_INVALID, "%s: gate %g us x %g Hz is not an int number of samples", who,
               (double) nb_param[kg_nbk::GATE], (double) sample_rate);
    KG_REQUIRE(r != kg_nbk::SETUP_BAD_RATE, KG_ERR_INVALID, "%s: sample rate %g (0.005 x rate must stay below %d)", who,
               (double) sample_rate, kg_nbk::MAG_CAP + 1);
    KG_REQUIRE(r != kg_nbk::SETUP_NEVER, KG_ERR_STATE, "%s: sample rate 0 on channel %d, which was never set up", who, ch);
    KG_PLAN_ONLY(ctx);
    hipLaunchKernelGGL(nb_reset_kernel, dim3(1), dim3(256), 0, ctx->stream, s->d_st + ch, s->d_mag + (size_t) ch * NB_MAG_STRIDE,
                       s->d_dly + (size_t) ch * NB_DLY_STRIDE, v);
    KG_HIP(hipGetLastError());
    s->h[ch] = v;
    s->was[ch] = 1;
    return KG_OK;
}

int kg_nb_store_state(kg_ctx *ctx, kg_nb_store *s, const int32_t *chans, int nch, int32_t *ints, float *flts, const char *who)
{
    KG_REQUIRE(chans && nch >= 1 && (ints || flts), KG_ERR_INVALID, "%s: null argument", who);
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(chans[i] >= 0 && chans[i] < s->nchan, KG_ERR_INVALID, "%s: channel %d", who, chans[i]);
        KG_REQUIRE(s->was[chans[i]], KG_ERR_STATE, "%s: channel %d was never set up", who, chans[i]);
    }
    KG_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < nch; i++) {
        kg_nbk::st v;
        KG_HIP(hipMemcpy(&v, s->d_st + chans[i], sizeof v, hipMemcpyDeviceToHost));
        if (ints) {
            int32_t *o = ints + 6 * (size_t) i;
            o[0] = v.mptr; o[1] = v.dptr; o[2] = v.cnt; o[3] = v.M; o[4] = v.D; o[5] = v.G;
        }
        if (flts) { flts[2 * (size_t) i] = v.ratio; flts[2 * (size_t) i + 1] = v.sum; }
    }
    return KG_OK;
}

int kg_nb_wf_launch(kg_ctx *ctx, kg_nb_store *s, int nbch, const void *d_chl, const void *d_fl, const void *d_iq,
                    const float *d_windows, void *d_out)
{
    hipLaunchKernelGGL(nb_wf_kernel, dim3(nbch), dim3(256), 0, ctx->stream, (const short2 *) d_iq, (const nb_wf_chan *) d_chl,
                       (const nb_wf_frame *) d_fl, d_windows, s->d_st, s->d_mag, s->d_dly, (float2 *) d_out);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

// ---------------------------------------------------------------------------
struct kg_nb {
    kg_ctx *ctx;
    int nchan, max_in;
    kg_nb_store *st;
    kg_dbuf<float2> d_stage;                  // kg_nb_process's staging row
    std::vector<char> seen;
};

int kg_nb_was_setup(const kg_nb *nb, int ch) { return kg_nb_store_was_setup(nb->st, ch); }

extern "C" {

int kg_nb_create(kg_ctx *ctx, int nchan, int max_in, kg_nb **out)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "kg_nb_create: out is null");
    *out = nullptr;
    KG_REQUIRE(nchan >= 1 && nchan <= 65536, KG_ERR_INVALID, "kg_nb_create: nchan %d", nchan);
    KG_REQUIRE(max_in >= 1 && max_in <= (1 << 24), KG_ERR_INVALID, "kg_nb_create: max_in %d", max_in);
    kg_nb *b = new (std::nothrow) kg_nb();
    KG_REQUIRE(b != nullptr, KG_ERR_NOMEM, "kg_nb_create: alloc");
    b->ctx = ctx; b->nchan = nchan; b->max_in = max_in;
    b->seen.assign(nchan, 0);
    if ((rc = kg_nb_store_create(nchan, &b->st)) != KG_OK) { kg_nb_destroy(b); return rc; }
    *out = b;
    return KG_OK;
}

void kg_nb_destroy(kg_nb *nb)
{
    if (!nb) return;
    (void) hipSetDevice(nb->ctx->device);
    (void) hipStreamSynchronize(nb->ctx->stream);
    kg_nb_store_destroy(nb->st);
    delete nb;
}

int kg_nb_setup(kg_nb *nb, int ch, float sample_rate, const float *nb_param)
{
    KG_REQUIRE(nb != nullptr, KG_ERR_INVALID, "kg_nb_setup: null argument");
    int rc = kg_ctx_use(nb->ctx);
    if (rc) return rc;
    return kg_nb_store_setup(nb->ctx, nb->st, ch, sample_rate, nb_param, "kg_nb_setup");
}

int kg_nb_process_dev(kg_nb *nb, const int32_t *chans, int nch, const void *d_in, size_t in_stride, const int32_t *n_each,
                      void *d_out, size_t out_stride)
{
    KG_REQUIRE(nb && chans && n_each && d_in && d_out, KG_ERR_INVALID, "kg_nb_process_dev: null argument");
    int rc = kg_ctx_use(nb->ctx);
    if (rc) return rc;
    KG_REQUIRE(nch >= 1 && nch <= nb->nchan, KG_ERR_INVALID, "kg_nb_process_dev: nch %d", nch);
    KG_REQUIRE(((uintptr_t) d_in & 7) == 0 && ((uintptr_t) d_out & 7) == 0, KG_ERR_INVALID, "kg_nb_process_dev: misaligned pointer");
    KG_REQUIRE(d_in != d_out || in_stride == out_stride, KG_ERR_INVALID,
               "kg_nb_process_dev: in place (d_in == d_out) needs in_stride == out_stride (rows would overlap)");
    nb->seen.assign(nb->nchan, 0);
    int any = 0;
    for (int i = 0; i < nch; i++) {
        const int ch = chans[i];
        KG_REQUIRE(ch >= 0 && ch < nb->nchan, KG_ERR_INVALID, "kg_nb_process_dev: channel %d", ch);
        KG_REQUIRE(!nb->seen[ch], KG_ERR_INVALID, "kg_nb_process_dev: channel %d listed twice", ch);
        nb->seen[ch] = 1;
        KG_REQUIRE(kg_nb_store_was_setup(nb->st, ch), KG_ERR_STATE, "kg_nb_process_dev: channel %d was never set up (kg_nb_setup)", ch);
        KG_REQUIRE(n_each[i] >= 0 && n_each[i] <= nb->max_in, KG_ERR_INVALID, "kg_nb_process_dev: n[%d] = %d (max %d)", i, n_each[i],
                   nb->max_in);
        KG_REQUIRE((size_t) n_each[i] <= in_stride && (size_t) n_each[i] <= out_stride, KG_ERR_INVALID,
                   "kg_nb_process_dev: n[%d] = %d above a stride", i, n_each[i]);
        if (n_each[i] > 0) any = 1;
    }
    if (!any) return KG_OK;
    void *base = nullptr;
    {
        std::vector<int32_t> pack(2 * (size_t) nch);
        memcpy(pack.data(), chans, sizeof(int32_t) * nch);
        memcpy(pack.data() + nch, n_each, sizeof(int32_t) * nch);
        if ((rc = kg_ctx_stage(nb->ctx, pack.data(), sizeof(int32_t) * pack.size(), &base))) return rc;
    }
    KG_PLAN_ONLY(nb->ctx);
    const int *s_list = (const int *) base;
    hipLaunchKernelGGL(nb_audio_kernel, dim3(nch), dim3(256), 0, nb->ctx->stream, s_list, s_list + nch, (const float2 *) d_in,
                       (long) in_stride, (float2 *) d_out, (long) out_stride, nb->st->d_st, nb->st->d_mag, nb->st->d_dly,
                       nb->ctx->rows_by_chan);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

int kg_nb_process(kg_nb *nb, int ch, const float *in, int n, float *out)
{
    KG_REQUIRE(nb && in && out, KG_ERR_INVALID, "kg_nb_process: null argument");
    int rc = kg_ctx_use(nb->ctx);
    if (rc) return rc;
    KG_REQUIRE(!nb->ctx->rows_by_chan, KG_ERR_STATE, "kg_nb_process: this object belongs to a receiver bank (its rows go by receiver "
               "number): step the bank");
    KG_REQUIRE(n >= 0 && n <= nb->max_in, KG_ERR_INVALID, "kg_nb_process: n %d (max %d)", n, nb->max_in);
    KG_REQUIRE(ch >= 0 && ch < nb->nchan, KG_ERR_INVALID, "kg_nb_process: channel %d", ch);
    KG_REQUIRE(kg_nb_store_was_setup(nb->st, ch), KG_ERR_STATE, "kg_nb_process: channel %d was never set up (kg_nb_setup)", ch);
    if (n == 0) return KG_OK;
    hipStream_t st = nb->ctx->stream;
    if (!nb->d_stage && (rc = nb->d_stage.alloc(nb->max_in, "kg_nb_process: staging")) != KG_OK) return rc;
    KG_HIP(hipMemcpyAsync(nb->d_stage, in, sizeof(float2) * n, hipMemcpyHostToDevice, st));
    const int32_t c = ch, cnt = n;
    if ((rc = kg_nb_process_dev(nb, &c, 1, nb->d_stage, nb->max_in, &cnt, nb->d_stage, nb->max_in))) return rc;
    KG_HIP(hipMemcpyAsync(out, nb->d_stage, sizeof(float2) * n, hipMemcpyDeviceToHost, st));
    KG_HIP(hipStreamSynchronize(st));
    return KG_OK;
}

int kg_nb_state(kg_nb *nb, const int32_t *chans, int nch, int32_t *ints, float *flts)
{
    KG_REQUIRE(nb != nullptr, KG_ERR_INVALID, "kg_nb_state: null argument");
    int rc = kg_ctx_use(nb->ctx);
    if (rc) return rc;
    return kg_nb_store_state(nb->ctx, nb->st, chans, nch, ints, flts, "kg_nb_state");
}

}  // extern "C"
