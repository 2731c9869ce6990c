// kg_cw.hip -- the CW decoder extension (extensions/CW_decoder/uhsdr_cw_decoder.cpp; csrc/kg_cw.h is the one definition of its
// arithmetic).
//
// As with kg_fax the SCHEDULE depends on the samples: every Goertzel magnitude moves the ring, the averages and the training, and these
// decide which characters, speeds and training messages a block sends.  The whole cw_decoder_t lives on the device (state_t) and the
// outputs carry counts the device writes.  The host keeps what the commands alone decide (started, the rates, blocksize for the
// refusals).
//
// ONE launch per push, one workgroup of 256 per listed connection, nothing shared between workgroups, no atomics.
//   Phase A, across the lanes: the Goertzel blocks of the push are independent of one another -- the recurrence restarts from zero in
//     every block (:323) and the coefficients are fixed within a push -- so each takes one lane: 88 dependent float steps over the
//     carried raw_signal_buffer entries (the first block's head) and the push's samples, then the energy.  The magnitudes go to LDS; a
//     push of 256 sound blocks gives at most 1490 of them.  What the last partial block leaves goes into raw[] as the reference's
//     buffer would hold it (entry i: the latest sample that fell on i).
//   Phase B, one lane: exe() of kg_cw.h, the very function the host twin runs, on the magnitudes in order, on the state in LDS, writing
//     the event records.
// LDS: 1490 * 4 + sizeof(state_t) (1760) + 16 = 7736 bytes a workgroup; four waves a workgroup.  Neither bounds the occupancy: a push
// has one workgroup per connection, at most 256 of them.
#include "kg_ext.h"
#include "kg_cw.h"

using namespace kg_cw_cf;

static_assert(BLK == KG_CW_BLK && GBLK == KG_CW_GBLK && EVENTS_PER_GBLK == KG_CW_EVENTS_PER_GBLK, "constants");
static_assert(EV_CHARS == KG_CW_CHARS && EV_WPM == KG_CW_WPM && EV_TRAIN == KG_CW_TRAIN && EV_PLOT == KG_CW_PLOT, "event kinds");
static_assert(sizeof(kg_cw_ev) == 24 && sizeof(ev_t) == 24 && sizeof(kg_cw_info) == 1760 && sizeof(state_t) == 1760, "kg_cw_ev / kg_cw_info layout");

enum { CW_THREADS = 256, CW_MAX_CONNS = 256, CW_MAX_BLK = 256, CW_MAX_GBLK = (BLK * CW_MAX_BLK + GBLK - 1) / GBLK };
enum { E_STARTED = 1 };
enum { OP_INIT = 0, OP_PBOFF = 1, OP_WSC = 2, OP_AUTO = 3, OP_THRESHOLD = 4 };

struct cw_entry {
    int32_t conn, nblk, flags, max_events;
    int64_t in_off;                             // samples from d_s16
    uint32_t now_sec; int32_t pad;
};
struct cw_cmd { int32_t op, a, b, snd_rate; double srate; };
static_assert(sizeof(cw_entry) == 32 && sizeof(cw_cmd) == 24, "table layout");

// a command on the device's object, in stream order
__global__ __launch_bounds__(64) void cw_cmd_kernel(state_t *dev, int conn, cw_cmd c)
{
    if (threadIdx.x != 0) return;
    state_t &s = dev[conn];
    switch (c.op) {
    case OP_INIT: cmd_init(s, c.a, c.b, c.snd_rate, c.srate); break;
    case OP_PBOFF: cmd_pboff(s, (uint32_t) c.a); break;
    case OP_WSC: cmd_wsc(s, c.a); break;
    case OP_AUTO: cmd_auto_threshold(s, c.a); break;
    case OP_THRESHOLD: cmd_threshold(s, c.a); break;
    }
}

struct cw_shared {
    state_t st;
    int32_t n, overflow, pad[2];
    float mag[CW_MAX_GBLK];
};

// entry e: events at evs + e * max_events, counts[4 e ..]: events, Goertzel blocks completed, overflow, 0
__global__ __launch_bounds__(CW_THREADS) void cw_push_kernel(const cw_entry *__restrict__ entries, const int16_t *__restrict__ in, kg_cw_ev *evs, int32_t *counts,
                                                            state_t *dev)
{
    __shared__ cw_shared sh;
    const cw_entry e = entries[blockIdx.x];
    const int tid = (int) threadIdx.x;
    state_t *d = dev + e.conn;
    if (!(e.flags & E_STARTED) || e.nblk <= 0 || !d->process_samples) {      // process_samples: uniform, and only commands write it
        if (tid < 4) counts[4 * blockIdx.x + tid] = 0;
        return;
    }
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(d);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&sh.st);
        for (int i = tid; i < (int) (sizeof(state_t) / 4); i += CW_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    state_t &st = sh.st;
    const int16_t *x = in + e.in_off;
    const int sc = st.sample_counter, n = BLK * e.nblk;
    const int nfull = gblocks(sc, n), rem = (sc + n) - nfull * GBLK;
    // ---- Phase A
    {
        const float r = st.g_r, cosv = st.g_cos, sinv = st.g_sin;
        const float *raw = st.raw;
        for (int j = tid; j < nfull; j += CW_THREADS) {
            const int p0 = j * GBLK - sc;                                // the block's first sample, counted in the push
            sh.mag[j] = goertzel_mag(r, cosv, sinv, [=](int i) { return p0 + i < 0 ? raw[sc + p0 + i] : sample_in(x[p0 + i]); });
        }
    }
    __syncthreads();
    if (tid < GBLK) {                                                    // raw_signal_buffer behind the push
        const int last = sc + n - 1;                                     // stream position of the push's last sample; position p falls on p % 88
        const int p = last - ((last - tid) % GBLK + GBLK) % GBLK;         // the latest position on tid
        if (p >= sc) st.raw[tid] = sample_in(x[p - sc]);
    }
    // ---- Phase B
    if (tid == 0) {
        sink_t k = {reinterpret_cast<ev_t *>(evs + (size_t) blockIdx.x * (size_t) e.max_events), 0, e.max_events, 0, 0, 0};
        for (int j = 0; j < nfull; j++) {
            const int blk = ((j + 1) * GBLK - 1 - sc) / BLK;              // the sound block in which the Goertzel block ended
            k.blk = blk;
            k.gblk = j - gblocks(sc, BLK * blk);
            exe(st, sh.mag[j], e.now_sec, k);
        }
        st.sample_counter = rem;
        sh.n = k.n; sh.overflow = k.overflow;
    }
    __syncthreads();
    {
        uint32_t *dst = reinterpret_cast<uint32_t *>(d);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&sh.st);
        for (int i = tid; i < (int) (sizeof(state_t) / 4); i += CW_THREADS) dst[i] = src[i];
    }
    if (tid == 0) {
        counts[4 * blockIdx.x] = sh.n; counts[4 * blockIdx.x + 1] = nfull; counts[4 * blockIdx.x + 2] = sh.overflow; counts[4 * blockIdx.x + 3] = 0;
    }
}

struct cw_conn {                                // what the commands alone decide
    int started, blocksize;
    double nom, srate;
};

struct kg_cw {
    kg_ctx *ctx;
    int nconn;
    std::vector<cw_conn> c;
    kg_dbuf<state_t> d_state;                   // [nconn]
};

// The checks of a push and its table.
static int cw_table(kg_cw *q, const int32_t *conns, int nconn, const int32_t *nblk, const int64_t *in_off, size_t stride, const uint32_t *now_sec, int max_events_,
                    std::vector<cw_entry> &tab, const char *who)
{
    KG_REQUIRE(nconn >= 1 && nconn <= q->nconn, KG_ERR_INVALID, "%s: nconn %d (1..%d)", who, nconn, q->nconn);
    KG_REQUIRE(max_events_ >= 0, KG_ERR_INVALID, "%s: max_events %d", who, max_events_);
    std::vector<char> listed((size_t) q->nconn, 0);
    for (int i = 0; i < nconn; i++) {
        const int c = conns[i];
        KG_TRY(kg_ext_list_entry(who, listed, nconn, i, c, nblk[i], CW_MAX_BLK, "stride", stride, BLK, in_off != nullptr, "sample offset", in_off ? in_off[i] : 0));
        cw_entry e;
        memset(&e, 0, sizeof e);
        e.conn = c; e.nblk = nblk[i]; e.max_events = max_events_;
        e.in_off = in_off ? in_off[i] : (int64_t) ((size_t) i * stride);
        e.now_sec = now_sec[i];
        if (q->c[c].started && nblk[i] > 0) {                           // cw_task is not woken for anybody else: the samples go nowhere
            KG_REQUIRE(max_events_ >= max_events(nblk[i]), KG_ERR_INVALID, "%s: max_events %d; %d blocks of connection %d can send %d events", who, max_events_,
                       nblk[i], c, max_events(nblk[i]));
            e.flags = E_STARTED;
        }
        tab.push_back(e);
    }
    return KG_OK;
}

// kg_cw_push on device memory, samples and outputs alike, with entry i's samples at in_off[i] samples from d_s16 (null: i * stride).  Enqueue only.
int kg_cw_push_at_(kg_cw *q, const int32_t *conns, int nconn, const int32_t *nblk, const int64_t *in_off, const int16_t *d_s16, size_t stride, const uint32_t *now_sec,
                   kg_cw_ev *d_evs, int max_events_, int32_t *d_counts)
{
    KG_REQUIRE(q && conns && nblk && d_s16 && now_sec && d_evs && d_counts, KG_ERR_INVALID, "kg_cw_push: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_REQUIRE(KG_ALIGNED(d_s16, 2) && KG_ALIGNED(d_evs, 4) && KG_ALIGNED(d_counts, 4), KG_ERR_INVALID, "kg_cw_push: the samples must be 2-byte aligned, events and counts 4-byte aligned");
    std::vector<cw_entry> tab;
    KG_TRY(cw_table(q, conns, nconn, nblk, in_off, stride, now_sec, max_events_, tab, "kg_cw_push"));
    void *d_tab = nullptr;
    if ((rc = kg_ctx_stage(q->ctx, tab.data(), sizeof(cw_entry) * tab.size(), &d_tab))) return rc;
    KG_PLAN_ONLY(q->ctx);
    hipLaunchKernelGGL(cw_push_kernel, dim3((unsigned) tab.size()), dim3(CW_THREADS), 0, q->ctx->stream, (const cw_entry *) d_tab, d_s16, d_evs, d_counts, q->d_state.p);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

// what the table of a push over nconn connections takes (and its alignment)
size_t kg_cw_table_bytes_(size_t nconn) { return 64 + nconn * sizeof(cw_entry); }

// a fresh object for the connection (a receiver joined or left): zeroed, as the static cw_decoder[] begins, slowdown with it.  Enqueue only.
int kg_cw_reset_(kg_cw *q, int conn)
{
    KG_REQUIRE(q != nullptr && conn >= 0 && conn < q->nconn, KG_ERR_INVALID, "kg_cw: connection %d", conn);
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_HIP(hipMemsetAsync(q->d_state.p + conn, 0, sizeof(state_t), q->ctx->stream));
    memset(&q->c[conn], 0, sizeof q->c[conn]);
    return KG_OK;
}

static int cw_command(kg_cw *q, int conn, const cw_cmd &c)
{
    KG_PLAN_ONLY(q->ctx);
    hipLaunchKernelGGL(cw_cmd_kernel, dim3(1), dim3(64), 0, q->ctx->stream, q->d_state.p, conn, c);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

extern "C" {

int kg_cw_create(kg_ctx *ctx, int nconn, kg_cw **out)
{
    return kg_ext_create(ctx, nconn, CW_MAX_CONNS, "kg_cw_create", "nconn", out, [=](kg_cw *q) {
        q->nconn = nconn;
        q->c.resize(nconn);
        for (cw_conn &c : q->c) memset(&c, 0, sizeof c);
        KG_TRY(q->d_state.alloc((size_t) nconn, "kg_cw_create: connection state"));
        return kg_ext_zero(ctx, q->d_state.p, (size_t) nconn, "kg_cw_create");
    });
}

void kg_cw_destroy(kg_cw *q) { kg_drain_delete(q); }

int kg_cw_start(kg_cw *q, int conn, int training_interval, double nom_rate, double srate)
{
    KG_EXT_INDEX("kg_cw_start", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const int bad = start_check(training_interval, nom_rate, srate);
    KG_REQUIRE(bad != REFUSED_INTERVAL, KG_ERR_INVALID, "kg_cw_start: training_interval %d (1 .. %d: the ring)", training_interval, SIG_BUFSIZE - 1);
    KG_REQUIRE(bad == 0, KG_ERR_INVALID, "kg_cw_start: nominal rate %g (%d .. 1e6), sample rate %g (half to twice the nominal)", nom_rate, GBLK, srate);
    const cw_cmd c = {OP_INIT, 0, training_interval, (int32_t) nom_rate, srate};
    KG_TRY(cw_command(q, conn, c));
    cw_conn &k = q->c[conn];
    k.started = 1; k.blocksize = GBLK; k.nom = nom_rate; k.srate = srate;
    return KG_OK;
}

int kg_cw_set_wpm(kg_cw *q, int conn, int wpm, int training_interval)
{
    KG_EXT_INDEX("kg_cw_set_wpm", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const cw_conn &k = q->c[conn];
    KG_REQUIRE(k.blocksize != 0, KG_ERR_INVALID, "kg_cw_set_wpm: connection %d was never started (its rates are not known)", conn);
    KG_REQUIRE(wpm >= 0, KG_ERR_INVALID, "kg_cw_set_wpm: wpm %d", wpm);
    KG_REQUIRE(wpm != 0 || start_check(training_interval, k.nom, k.srate) == 0, KG_ERR_INVALID, "kg_cw_set_wpm: training_interval %d (1 .. %d: the ring)",
               training_interval, SIG_BUFSIZE - 1);
    const cw_cmd c = {OP_INIT, wpm, training_interval, (int32_t) k.nom, k.srate};
    return cw_command(q, conn, c);
}

int kg_cw_set_pboff(kg_cw *q, int conn, uint32_t pboff)
{
    KG_EXT_INDEX("kg_cw_set_pboff", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const cw_conn &k = q->c[conn];
    const int bad = pboff_check((float) k.srate, k.blocksize, pboff);
    KG_REQUIRE(bad != REFUSED_NOT_STARTED, KG_ERR_INVALID, "kg_cw_set_pboff: connection %d was never started (blocksize is 0)", conn);
    KG_REQUIRE(bad == 0, KG_ERR_INVALID, "kg_cw_set_pboff: pboff %u at %g Hz selects bin %d (0 .. %d)", pboff, k.srate, pboff_a((float) k.srate, pboff), GBLK / 2);
    const cw_cmd c = {OP_PBOFF, (int32_t) pboff, 0, 0, 0.0};
    return cw_command(q, conn, c);
}

int kg_cw_set_wsc(kg_cw *q, int conn, int wsc)
{
    KG_EXT_INDEX("kg_cw_set_wsc", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const cw_cmd c = {OP_WSC, wsc, 0, 0, 0.0};
    return cw_command(q, conn, c);
}

int kg_cw_set_auto_threshold(kg_cw *q, int conn, int on)
{
    KG_EXT_INDEX("kg_cw_set_auto_threshold", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const cw_cmd c = {OP_AUTO, on, 0, 0, 0.0};
    return cw_command(q, conn, c);
}

int kg_cw_set_threshold(kg_cw *q, int conn, int threshold)
{
    KG_EXT_INDEX("kg_cw_set_threshold", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const cw_cmd c = {OP_THRESHOLD, threshold, 0, 0, 0.0};
    return cw_command(q, conn, c);
}

int kg_cw_stop(kg_cw *q, int conn)
{
    KG_EXT_INDEX("kg_cw_stop", q, conn, q->nconn, "connection");
    q->c[conn].started = 0;                     // cw_close (cw_decoder.cpp:107-119): the task tap goes; the decoder stays
    return KG_OK;
}

int kg_cw_max_events(int nblk) { return nblk < 0 || nblk > CW_MAX_BLK ? -1 : max_events(nblk); }

int kg_cw_push(kg_cw *q, const int32_t *conns, int nconn, const int32_t *nblk, const int16_t *s16, size_t stride, const uint32_t *now_sec, kg_cw_ev *evs,
               int max_events, int32_t *counts)
{
    KG_REQUIRE(q && conns && nblk && s16 && now_sec && evs && counts, KG_ERR_INVALID, "kg_cw_push: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    {   // checked ahead of the first copy: a push that will be refused enqueues nothing here either
        std::vector<cw_entry> tab;
        KG_TRY(cw_table(q, conns, nconn, nblk, nullptr, stride, now_sec, max_events, tab, "kg_cw_push"));
    }
    size_t last = 0;
    for (int i = 0; i < nconn; i++)
        if (nblk[i] > 0) last = (size_t) i * stride + (size_t) BLK * nblk[i];
    const size_t nev = (size_t) nconn * (size_t) max_events;
    int16_t *d_s16 = nullptr;
    kg_cw_ev *d_evs = nullptr;
    int32_t *d_counts = nullptr;
    hipStream_t s = q->ctx->stream;
    kg_scope tmp(q->ctx);                               // the caller's arrays and the temporaries are in use until it has drained the stream
    KG_TRY(tmp.alloc(&d_s16, last ? last : 1, "kg_cw_push: samples"));
    KG_TRY(tmp.alloc(&d_evs, nev ? nev : 1, "kg_cw_push: events"));
    KG_TRY(tmp.alloc(&d_counts, (size_t) 4 * nconn, "kg_cw_push: counts"));
    for (int i = 0; i < nconn; i++)
        if (nblk[i] > 0)
            KG_HIP(hipMemcpyAsync(d_s16 + (size_t) i * stride, s16 + (size_t) i * stride, sizeof(int16_t) * BLK * (size_t) nblk[i], hipMemcpyHostToDevice, s));
    KG_TRY(kg_cw_push_at_(q, conns, nconn, nblk, nullptr, d_s16, stride, now_sec, d_evs, max_events, d_counts));
    KG_HIP(hipMemcpyAsync(counts, d_counts, sizeof(int32_t) * 4 * (size_t) nconn, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < nconn; i++) {                   // the events the device counted, nothing else of the caller's array
        const size_t n = (size_t) counts[4 * i];
        if (n) KG_HIP(hipMemcpyAsync(evs + (size_t) i * max_events, d_evs + (size_t) i * max_events, sizeof(kg_cw_ev) * n, hipMemcpyDeviceToHost, s));
    }
    KG_HIP(hipStreamSynchronize(s));
    return KG_OK;                                       // tmp drains the stream
}

int kg_cw_state(kg_cw *q, int conn, kg_cw_info *info)
{
    KG_EXT_INDEX("kg_cw_state", q, conn, q->nconn, "connection");
    KG_REQUIRE(info != nullptr, KG_ERR_INVALID, "kg_cw_state: info is null");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    hipStream_t s = q->ctx->stream;
    KG_HIP(hipMemcpyAsync(info, q->d_state.p + conn, sizeof(state_t), hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    info->started = q->c[conn].started;
    return KG_OK;
}

}  // extern "C"
