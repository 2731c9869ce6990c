// kg_lorc.hip -- the Loran-C extension (extensions/Loran_C/loran_c.cpp; csrc/kg_lorc.h is the one definition of its arithmetic).
//
// The schedule of loran_c_data (:65-196: bn, dsp_samps, avg_samps, navgs, restart, redraw_legend) depends on no sample, so the host
// walks it per call (plan_stretch of kg_lorc.h) and hands the kernel a table: per listed and started connection and Loran channel a
// group {connection, channel, its runs' range, rule, parameters, nbucket, gain, where its samples are}, per RUN -- a maximal stretch
// of samples over which bn rises by one per sample -- {first sample, length, bn0, navgs, flags (row / clear), the row's place}.
// Within a run every sample has a bucket of its own; a row and a clear can only stand at a run's first sample (bn == 0 only there);
// navgs is constant over a run.  ONE launch per call: one workgroup of ONE wave64 per group, the channel's avg[] (4.8 KB) in
// LDS for the whole call, read at the start and written back at the end.  Per run, in the reference's order:
//   the row    max -- a wave maximum of avg[0 .. nbucket) under auto gain, gain * CUTESDR_MAX_VAL else --, then the bytes across
//              lanes into LDS and from there to the row's place, 16 bytes a lane (rows start at multiples of 16) and the tail by bytes;
//   the clear  avg[0 .. nbucket) = 0;
//   the update one sample a lane, 64 at a time: power, then the rule's recurrence on the sample's own bucket, unreassociated.
// The two channels of a connection share nothing on the device (their rows' places and commands are the host's), so each has a
// workgroup of its own; one wave a workgroup makes a barrier a wait for the wave's own memory operations.
#include "kg_ext.h"
#include "kg_lorc.h"

using namespace kg_lorc_cf;

static_assert(MAX_BUCKET == KG_LORC_MAX_BUCKET && MAX_NS == KG_LORC_MAX_NS && MAX_GRI == KG_LORC_MAX_GRI, "constants");
static_assert(AVG_CMA == KG_LORC_CMA && AVG_EMA == KG_LORC_EMA && AVG_IIR == KG_LORC_IIR && SCOPE_DATA == KG_LORC_SCOPE_DATA && SCOPE_RESET == KG_LORC_SCOPE_RESET,
              "constants");
static_assert(sizeof(kg_lorc_row) == 32 && sizeof(kg_lorc_chan) == 64 && sizeof(kg_lorc_info) == 152, "kg_lorc_row / kg_lorc_info layout");

enum { LO_LANES = 64, LO_PAD = 1200 };                                  // avg[] padded to a multiple of 16 bytes
enum { LO_MAX_CONNS = 1024, LO_MAX_BLK = 256 };
enum { R_EMIT = 1, R_ZERO = 2 };
enum { G_FRESH = 1 };                                                   // `SET ext_server_init` since the last call: avg[] and max are zero

struct lo_dev { float avg[NCH][LO_PAD]; float max[NCH]; float pad[2]; };      // one connection
static_assert(sizeof(lo_dev) == 9616, "device state");

struct lo_group {
    int32_t conn, ch, first, nruns, algo, param_i, flags;
    uint32_t nbucket;
    int64_t in_off;                                                     // complex samples from d_iq
    double param_f;
    float gain; int32_t pad[3];
};
struct lo_run { int32_t start, len, bn0, flags; uint32_t navgs; int32_t pad; int64_t row_off; };
static_assert(sizeof(lo_group) == 64 && sizeof(lo_run) == 32, "table layout");

static inline size_t row_room(size_t len) { return (len + 15) & ~(size_t) 15; }      // rows start at multiples of 16 bytes

__global__ __launch_bounds__(LO_LANES) void lorc_kernel(const lo_group *__restrict__ groups, const lo_run *__restrict__ runs, const float2 *__restrict__ in,
                                                        uint8_t *rows, lo_dev *dev)
{
    __shared__ float s_avg[LO_PAD];
    __shared__ __align__(16) uint8_t s_row[LO_PAD + 16];
    const lo_group g = groups[blockIdx.x];
    const int lane = (int) threadIdx.x;
    lo_dev *d = dev + g.conn;
    const bool fresh = (g.flags & G_FRESH) != 0;
    for (int i = lane; i < LO_PAD; i += LO_LANES) s_avg[i] = fresh || i >= MAX_BUCKET ? 0.0f : d->avg[g.ch][i];
    float max = fresh ? 0.0f : d->max[g.ch];
    __syncthreads();
    const uint32_t nb = g.nbucket;
    const float2 *src = in + g.in_off;
    for (int r = 0; r < g.nruns; r++) {
        const lo_run run = runs[g.first + r];
        if (run.flags & R_EMIT) {
            if (g.gain == 0.0f) {                                       // auto-scale (:91-97): the maximum, from 0 on
                max = 0.0f;
                for (uint32_t j = lane; j < nb; j += LO_LANES)
                    if (s_avg[j] > max) max = s_avg[j];
                for (int m = LO_LANES / 2; m >= 1; m >>= 1) {
                    const float o = __shfl_xor(max, m, LO_LANES);
                    if (o > max) max = o;
                }
            } else max = fixed_max(g.gain);
            for (uint32_t j = lane; j < nb; j += LO_LANES) s_row[j + 1] = scope_byte(s_avg[j], max);
            if (lane == 0) s_row[0] = (uint8_t) g.ch;
            __syncthreads();
            const int len = (int) nb + 1;
            uint8_t *dst = rows + run.row_off;
            const uint4 *s16 = reinterpret_cast<const uint4 *>(s_row);
            uint4 *d16 = reinterpret_cast<uint4 *>(dst);
            for (int i = lane; i < len / 16; i += LO_LANES) d16[i] = s16[i];
            for (int i = (len & ~15) + lane; i < len; i += LO_LANES) dst[i] = s_row[i];
            __syncthreads();
        }
        if (run.flags & R_ZERO) {
            for (uint32_t j = lane; j < nb; j += LO_LANES) s_avg[j] = 0.0f;
            __syncthreads();
        }
        for (int k = lane; k < run.len; k += LO_LANES) {
            const uint32_t bn = (uint32_t) (run.bn0 + k);
            if (bn < nb - 1u) {
                const float2 x = src[run.start + k];
                s_avg[bn] = update(g.algo, s_avg[bn], power(x.x, x.y), run.navgs, g.param_i, g.param_f);
            }
        }
        __syncthreads();
    }
    for (int i = lane; i < MAX_BUCKET; i += LO_LANES) d->avg[g.ch][i] = s_avg[i];
    if (lane == 0) d->max[g.ch] = max;
}

struct lo_conn {
    state_t st;                                 // avg[] and max live on the device
    int fresh;                                  // the connection's next call zeroes them first
};

struct kg_lorc {
    kg_ctx *ctx;
    int nconn;
    std::vector<lo_conn> c;
    kg_dbuf<lo_dev> d_state;                    // [nconn]
};

struct lo_plan {
    std::vector<int> conn;                      // the started connections of the list with samples, in list order
    std::vector<state_t> st;                    // their states behind the call
    std::vector<lo_group> groups;
    std::vector<lo_run> runs;
    std::vector<kg_lorc_row> rows;
    size_t row_bytes = 0;
};

static const char *refusal_text(int rc)
{
    return rc == REFUSED_NO_GRI ? "a channel without a GRI" : rc == REFUSED_EMA ? "EMA with avg_param below 1" : "IIR with a negative or non-finite avg_param";
}

static int lo_walk(kg_lorc *q, const int32_t *conns, int nconn, const int32_t *nblk, const int32_t *in_row, int ns, size_t iq_stride, size_t rows_cap, int max_rows,
                   lo_plan &p, const char *who)
{
    KG_REQUIRE(nconn >= 1 && nconn <= q->nconn, KG_ERR_INVALID, "%s: nconn %d (1..%d)", who, nconn, q->nconn);
    KG_REQUIRE(ns >= 1 && ns <= MAX_NS, KG_ERR_INVALID, "%s: ns %d (1..%d)", who, ns, MAX_NS);
    KG_REQUIRE(max_rows >= 0, KG_ERR_INVALID, "%s: max_rows %d", who, max_rows);
    std::vector<char> listed((size_t) q->nconn, 0);
    plan_t sp;
    for (int i = 0; i < nconn; i++) {
        const int c = conns[i];
        // a row is a multiple of the stride: the stride bounds an entry's blocks whoever places the rows
        KG_TRY(kg_ext_list_entry(who, listed, nconn, i, c, nblk[i], LO_MAX_BLK, "iq_stride", iq_stride, (size_t) ns, false, "sample row", in_row ? in_row[i] : 0));
        KG_REQUIRE(q->c[c].st.inited, KG_ERR_STATE, "%s: connection %d was never initialised (kg_lorc_init)", who, c);
        if (!q->c[c].st.started || nblk[i] == 0) continue;             // loran_c_data is not registered: the samples go nowhere
        const int bad = push_check(q->c[c].st);
        KG_REQUIRE(bad == 0, KG_ERR_INVALID, "%s: connection %d is started with %s", who, c, refusal_text(bad));
        const state_t &before = q->c[c].st;
        state_t st = before;
        plan_stretch(st, ns * nblk[i], sp);
        const size_t row0 = p.rows.size();
        for (const emis_t &m : sp.emis) {
            KG_REQUIRE(p.row_bytes + (size_t) m.len <= rows_cap, KG_ERR_INVALID, "%s: more row bytes than the capacity %zu", who, rows_cap);
            KG_REQUIRE(p.rows.size() < (size_t) max_rows, KG_ERR_INVALID, "%s: more rows than max_rows = %d", who, max_rows);
            p.rows.push_back(kg_lorc_row{c, m.samp / ns, m.samp % ns, m.ch, m.cmd, m.len, (int64_t) p.row_bytes});
            p.row_bytes += row_room((size_t) m.len);
        }
        for (int ch = 0; ch < NCH; ch++) {
            const chan_t &cc = before.ch[ch];                          // the commands' part: what it was when the call began
            lo_group g;
            memset(&g, 0, sizeof g);
            g.conn = c; g.ch = ch; g.first = (int32_t) p.runs.size(); g.nruns = (int32_t) sp.runs[ch].size();
            g.algo = cc.avg_algo; g.param_i = cc.avg_param_i; g.flags = q->c[c].fresh ? G_FRESH : 0; g.nbucket = cc.nbucket;
            g.in_off = (int64_t) ((size_t) (in_row ? in_row[i] : i) * iq_stride);
            g.param_f = cc.avg_param_f; g.gain = cc.gain;
            for (const run_t &r : sp.runs[ch]) {
                lo_run o = {r.start, r.len, r.bn0, (r.emit ? R_EMIT : 0) | (r.zero ? R_ZERO : 0), r.navgs, 0, 0};
                if (r.emit) o.row_off = p.rows[row0 + r.emit - 1].off;                // the row's command is the map's: the kernel sends nothing
                p.runs.push_back(o);
            }
            p.groups.push_back(g);
        }
        p.conn.push_back(c);
        p.st.push_back(st);
    }
    return KG_OK;
}

// kg_lorc_process on device memory, entry i's samples at row in_row[i] of d_iq (null: row i).  Enqueue only.
int kg_lorc_process_rows_(kg_lorc *q, const int32_t *conns, int nconn, const int32_t *nblk, const int32_t *in_row, int ns, const float *d_iq, size_t iq_stride,
                          uint8_t *d_rows, size_t rows_cap, kg_lorc_row *row_map, int max_rows, int32_t *nrows)
{
    KG_REQUIRE(q && conns && nblk && d_iq && d_rows && nrows, KG_ERR_INVALID, "kg_lorc_process: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_REQUIRE(KG_ALIGNED(d_iq, 8) && KG_ALIGNED(d_rows, 16), KG_ERR_INVALID, "kg_lorc_process: the samples must be 8-byte aligned, the rows 16-byte aligned");
    lo_plan p;
    KG_TRY(lo_walk(q, conns, nconn, nblk, in_row, ns, iq_stride, rows_cap, max_rows, p, "kg_lorc_process"));
    if (!p.groups.empty()) {
        std::vector<unsigned char> tab(sizeof(lo_group) * p.groups.size() + sizeof(lo_run) * p.runs.size());
        memcpy(tab.data(), p.groups.data(), sizeof(lo_group) * p.groups.size());
        if (!p.runs.empty()) memcpy(tab.data() + sizeof(lo_group) * p.groups.size(), p.runs.data(), sizeof(lo_run) * p.runs.size());
        void *d_tab = nullptr;
        if ((rc = kg_ctx_stage(q->ctx, tab.data(), tab.size(), &d_tab))) return rc;
        KG_PLAN_ONLY(q->ctx);
        hipLaunchKernelGGL(lorc_kernel, dim3((unsigned) p.groups.size()), dim3(LO_LANES), 0, q->ctx->stream, (const lo_group *) d_tab,
                           (const lo_run *) ((const unsigned char *) d_tab + sizeof(lo_group) * p.groups.size()), (const float2 *) d_iq, d_rows, q->d_state.p);
        KG_HIP(hipGetLastError());
    } else {
        KG_PLAN_ONLY(q->ctx);
    }
    for (size_t k = 0; k < p.conn.size(); k++) { q->c[p.conn[k]].st = p.st[k]; q->c[p.conn[k]].fresh = 0; }      // commit: the enqueue succeeded
    if (row_map && !p.rows.empty()) memcpy(row_map, p.rows.data(), sizeof(kg_lorc_row) * p.rows.size());
    *nrows = (int32_t) p.rows.size();
    return KG_OK;
}

// what the table of a call over nconn connections takes when no channel has more than runs_per_channel runs (and its alignment)
size_t kg_lorc_table_bytes_(size_t nconn, size_t runs_per_channel) { return 64 + nconn * NCH * (sizeof(lo_group) + sizeof(lo_run) * runs_per_channel); }

int kg_lorc_reset_(kg_lorc *q, int conn)
{
    KG_REQUIRE(q != nullptr && conn >= 0 && conn < q->nconn, KG_ERR_INVALID, "kg_lorc: connection %d", conn);
    memset(&q->c[conn].st, 0, sizeof q->c[conn].st);
    q->c[conn].fresh = 1;
    return KG_OK;
}

// kg_lorc_set_gri that also refuses a GRI of fewer than min_spg samples (a receiver bank bounds the runs of a step by it)
int kg_lorc_set_gri_min_(kg_lorc *q, int conn, int ch, int gri, double min_spg)
{
    KG_REQUIRE(q != nullptr && conn >= 0 && conn < q->nconn, KG_ERR_INVALID, "kg_lorc_set_gri: connection %d", conn);
    KG_REQUIRE(q->c[conn].st.inited, KG_ERR_STATE, "kg_lorc_set_gri: connection %d was never initialised (kg_lorc_init)", conn);
    KG_REQUIRE(ch_ok(ch), KG_ERR_INVALID, "kg_lorc_set_gri: Loran channel %d (0..1)", ch);
    state_t st = q->c[conn].st;
    const int rc = cmd_gri(st, ch, gri);
    KG_REQUIRE(rc != REFUSED_GRI, KG_ERR_INVALID, "kg_lorc_set_gri: gri %d (1..%d)", gri, MAX_GRI);
    KG_REQUIRE(rc == 0, KG_ERR_INVALID, "kg_lorc_set_gri: gri %d at %g Hz needs %d buckets or more (the reference's scope[] holds %d)", gri, st.srate, MAX_BUCKET,
               MAX_BUCKET);
    KG_REQUIRE(st.ch[ch].samp_per_GRI >= min_spg, KG_ERR_INVALID, "kg_lorc_set_gri: gri %d at %g Hz is %g samples; a receiver bank takes %g or more", gri, st.srate,
               st.ch[ch].samp_per_GRI, min_spg);
    q->c[conn].st = st;
    return KG_OK;
}

extern "C" {

int kg_lorc_create(kg_ctx *ctx, int nconn, kg_lorc **out)
{
    return kg_ext_create(ctx, nconn, LO_MAX_CONNS, "kg_lorc_create", "nconn", out, [=](kg_lorc *q) {
        q->nconn = nconn;
        q->c.resize(nconn);
        for (lo_conn &c : q->c) { memset(&c.st, 0, sizeof c.st); c.fresh = 1; }     // fresh: the device state needs no zeroing here
        return q->d_state.alloc((size_t) nconn, "kg_lorc_create: connection state");
    });
}

void kg_lorc_destroy(kg_lorc *q) { kg_drain_delete(q); }

#define LO_INITED(who)                                                                               \
    KG_EXT_INDEX(who, q, conn, q->nconn, "connection");                                               \
    KG_REQUIRE(q->c[conn].st.inited, KG_ERR_STATE, who ": connection %d was never initialised (kg_lorc_init)", conn)
#define LO_CH(who) KG_REQUIRE(ch_ok(ch), KG_ERR_INVALID, who ": Loran channel %d (0..1)", ch)

int kg_lorc_init(kg_lorc *q, int conn, double srate, int i_srate)
{
    KG_EXT_INDEX("kg_lorc_init", q, conn, q->nconn, "connection");
    KG_REQUIRE(srate >= 1 && srate <= 1e9 && i_srate >= 0, KG_ERR_INVALID, "kg_lorc_init: sample rate %g (1 .. 1e9), snd_rate %d", srate, i_srate);
    cmd_init(q->c[conn].st, srate, i_srate);
    q->c[conn].fresh = 1;
    return KG_OK;
}

int kg_lorc_set_gri(kg_lorc *q, int conn, int ch, int gri) { return kg_lorc_set_gri_min_(q, conn, ch, gri, 0.0); }

int kg_lorc_set_offset(kg_lorc *q, int conn, int ch, int offset)
{
    LO_INITED("kg_lorc_set_offset");
    LO_CH("kg_lorc_set_offset");
    KG_REQUIRE(cmd_offset(q->c[conn].st, ch, offset) == 0, KG_ERR_INVALID, "kg_lorc_set_offset: channel %d has no GRI yet (the reference divides by zero)", ch);
    return KG_OK;
}

int kg_lorc_set_gain(kg_lorc *q, int conn, int ch, int gain)
{
    LO_INITED("kg_lorc_set_gain");
    LO_CH("kg_lorc_set_gain");
    cmd_gain(q->c[conn].st, ch, gain);
    return KG_OK;
}

int kg_lorc_set_avg_algo(kg_lorc *q, int conn, int ch, int avg_algo)
{
    LO_INITED("kg_lorc_set_avg_algo");
    LO_CH("kg_lorc_set_avg_algo");
    KG_REQUIRE(cmd_avg_algo(q->c[conn].st, ch, avg_algo) == 0, KG_ERR_INVALID, "kg_lorc_set_avg_algo: rule %d (0 CMA, 1 EMA, 2 IIR; the reference panics)", avg_algo);
    return KG_OK;
}

int kg_lorc_set_avg_param(kg_lorc *q, int conn, int ch, double avg_param)
{
    LO_INITED("kg_lorc_set_avg_param");
    LO_CH("kg_lorc_set_avg_param");
    cmd_avg_param(q->c[conn].st, ch, avg_param);
    return KG_OK;
}

int kg_lorc_start(kg_lorc *q, int conn)
{
    LO_INITED("kg_lorc_start");
    cmd_start(q->c[conn].st);
    return KG_OK;
}

int kg_lorc_stop(kg_lorc *q, int conn)
{
    LO_INITED("kg_lorc_stop");
    cmd_stop(q->c[conn].st);
    return KG_OK;
}

int kg_lorc_process(kg_lorc *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, const float *iq, size_t iq_stride,
                    uint8_t *rows, size_t rows_cap, kg_lorc_row *row_map, int max_rows, int32_t *nrows)
{
    KG_REQUIRE(q && conns && nblk && iq && rows && row_map && nrows, KG_ERR_INVALID, "kg_lorc_process: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    size_t last = 0;
    {   // the schedule is walked (on copies) ahead of the first copy: a call that will be refused enqueues nothing here either
        lo_plan p;
        KG_TRY(lo_walk(q, conns, nconn, nblk, nullptr, ns, iq_stride, rows_cap, max_rows, p, "kg_lorc_process"));
    }
    for (int i = 0; i < nconn; i++)
        if (nblk[i] > 0) last = (size_t) i * iq_stride + (size_t) ns * nblk[i];
    float *d_iq = nullptr;
    uint8_t *d_rows = nullptr;
    hipStream_t s = q->ctx->stream;
    kg_scope tmp(q->ctx);                               // the caller's arrays and the temporaries are in use until it has drained the stream
    KG_TRY(tmp.alloc(&d_iq, 2 * (last ? last : 1), "kg_lorc_process: samples"));
    KG_TRY(tmp.alloc(&d_rows, rows_cap ? rows_cap : 1, "kg_lorc_process: rows"));
    bool dense = true;                                  // every entry fills its row: one copy
    for (int i = 0; i < nconn; i++) dense = dense && (size_t) ns * (size_t) nblk[i] == iq_stride;
    if (dense && last) KG_HIP(hipMemcpyAsync(d_iq, iq, sizeof(float) * 2 * last, hipMemcpyHostToDevice, s));
    else
        for (int i = 0; i < nconn; i++)
            if (nblk[i] > 0)
                KG_HIP(hipMemcpyAsync(d_iq + 2 * (size_t) i * iq_stride, iq + 2 * (size_t) i * iq_stride, sizeof(float) * 2 * ns * (size_t) nblk[i],
                                      hipMemcpyHostToDevice, s));
    int32_t n = 0;
    KG_TRY(kg_lorc_process_rows_(q, conns, nconn, nblk, nullptr, ns, d_iq, iq_stride, d_rows, rows_cap, row_map, max_rows, &n));
    if (n > 0) {                                        // one copy back, then the rows alone: what lies between them stays the caller's
        std::vector<uint8_t> back((size_t) row_map[n - 1].off + (size_t) row_map[n - 1].len);
        KG_HIP(hipMemcpyAsync(back.data(), d_rows, back.size(), hipMemcpyDeviceToHost, s));
        KG_HIP(hipStreamSynchronize(s));
        for (int r = 0; r < n; r++) memcpy(rows + row_map[r].off, back.data() + row_map[r].off, (size_t) row_map[r].len);
    }
    *nrows = n;
    return KG_OK;                                       // tmp drains the stream
}

int kg_lorc_plan(kg_lorc *q, const int32_t *conns, int nconn, const int32_t *nblk, int ns, int32_t *nruns, int32_t *nrows, size_t *row_bytes)
{
    KG_REQUIRE(q && conns && nblk, KG_ERR_INVALID, "kg_lorc_plan: null argument");
    lo_plan p;
    KG_TRY(lo_walk(q, conns, nconn, nblk, nullptr, ns, ~(size_t) 0 >> 1, ~(size_t) 0 >> 1, 0x7fffffff, p, "kg_lorc_plan"));
    if (nruns) *nruns = (int32_t) p.runs.size();
    if (nrows) *nrows = (int32_t) p.rows.size();
    if (row_bytes) *row_bytes = p.rows.empty() ? 0 : (size_t) p.rows.back().off + (size_t) p.rows.back().len;
    return KG_OK;
}

int kg_lorc_state(kg_lorc *q, int conn, kg_lorc_info *info, float *avg)
{
    KG_EXT_INDEX("kg_lorc_state", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const lo_conn &c = q->c[conn];
    const lo_dev *d = q->d_state.p + conn;
    hipStream_t s = q->ctx->stream;
    float max[NCH] = {0, 0};
    const bool zero = c.fresh != 0;                     // a fresh object whose zeroing waits for the connection's next call
    if (!zero) KG_HIP(hipMemcpyAsync(max, d->max, sizeof max, hipMemcpyDeviceToHost, s));
    if (avg) {
        if (zero) memset(avg, 0, sizeof(float) * NCH * MAX_BUCKET);
        else
            for (int ch = 0; ch < NCH; ch++)
                KG_HIP(hipMemcpyAsync(avg + (size_t) ch * MAX_BUCKET, d->avg[ch], sizeof(float) * MAX_BUCKET, hipMemcpyDeviceToHost, s));
    }
    KG_HIP(hipStreamSynchronize(s));
    if (info) {
        const state_t &e = c.st;
        memset(info, 0, sizeof *info);
        info->inited = e.inited; info->started = e.started; info->i_srate = e.i_srate; info->redraw_legend = e.redraw_legend; info->srate = e.srate;
        for (int ch = 0; ch < NCH; ch++) {
            const chan_t &k = e.ch[ch];
            kg_lorc_chan &o = info->ch[ch];
            o.gri = k.gri; o.samp = k.samp; o.nbucket = k.nbucket; o.dsp_samps = k.dsp_samps; o.avg_samps = k.avg_samps; o.navgs = k.navgs;
            o.samp_per_GRI = k.samp_per_GRI; o.gain = k.gain; o.max = max[ch]; o.offset = k.offset; o.avg_algo = k.avg_algo;
            o.avg_param_f = k.avg_param_f; o.avg_param_i = k.avg_param_i; o.restart = k.restart;
        }
    }
    return KG_OK;
}

float kg_lorc_ms_per_bin(double srate, int i_srate) { return ms_per_bin(srate, i_srate); }

}  // extern "C"
