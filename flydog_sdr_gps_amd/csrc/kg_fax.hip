// kg_fax.hip -- the HF weather fax extension (extensions/FAX/FaxDecoder.cpp; csrc/kg_fax.h is the one definition of its arithmetic).
//
// Unlike kg_iqd and kg_lorc the SCHEDULE depends on the samples: the phasing result sets m_skip, which moves every later line
// boundary, and the stop tone sets m_autostopped, which suppresses rows.  The host cannot walk it ahead of the device, so the whole
// FaxDecoder lives on the device (fx_dev: the scalars, the line of samples, the previous image line, m_outImage) and the outputs
// carry counts the device writes.  The host keeps what the commands alone decide (started, the pending shift, spl and imagewidth for
// the bounds).
//
// ONE launch per push, one workgroup of 256 per listed connection, nothing shared between workgroups, no atomics.  The workgroup
// walks its blocks in order as ProcessSamples does (:410-447): one lane runs the double chain m_fi += ratio; i = trunc(m_fi) and
// leaves the picks in LDS, all lanes copy them into the line; where a line completes it is run in full before the walk goes on
// inside the same block:
//   demodulate  in chunks of 1024 samples: the mixer products across lanes into LDS (behind the 16 carried over), then the two 17-tap
//               sums, the normalisation and the discriminator per sample, each with the operand order of kg_fax.h.  The mixer angles
//               (float) (K_2PI * f) depend on ph_inc alone: one lane walks f += ph_inc once and the table stays until ph_inc changes;
//   detect      the four Fourier sums are serial float chains: the products across lanes, 1024 at a time, then one lane of each of
//               the four waves adds its chain in index order;
//   phasing     one candidate position per lane, then the workgroup's minimum of (total, position): the first minimum;
//   decode      one pixel per lane: the integer average, the blend with the previous line, the row;
// the scalar decisions between them (machine_pre / machine_post / blend_decide / machine_tail of kg_fax.h) are one lane's.
#include "kg_ext.h"
#include "kg_fax.h"

using namespace kg_fax_cf;

static_assert(MAX_SPL == KG_FAX_MAX_SPL && BLK == KG_FAX_BLK && MSG_DRAW == KG_FAX_MSG_DRAW, "constants");
static_assert(F_SPS_CHANGED == KG_FAX_SPS_CHANGED && F_AUTOSTOPPED_0 == KG_FAX_AUTOSTOPPED_0 && F_AUTOSTOPPED_1 == KG_FAX_AUTOSTOPPED_1 && F_PHASED == KG_FAX_PHASED &&
                  F_ROW_SENT == KG_FAX_ROW_SENT && F_PHASING_REJECTED == KG_FAX_PHASING_REJECTED && F_MEDIAN == KG_FAX_MEDIAN,
              "flags");
static_assert(sizeof(kg_fax_rec) == 48 && sizeof(rec_t) == 48 && sizeof(kg_fax_info) == 472 && sizeof(state_t) % 8 == 0, "kg_fax_rec / kg_fax_info layout");

enum { FX_THREADS = 256, FX_CHUNK = 1024, FX_PICKS = 1024, FX_MAX_CONNS = 256, FX_MAX_BLK = 256, FX_HIST = TAPS - 1 };
enum { E_STARTED = 1 };

struct fx_dev {                                 // one connection
    state_t s;
    double ang_ph_inc;                          // ang[0 .. ang_n) is the mixer's angle table for this ph_inc
    int32_t ang_n, pad;
    int16_t samples[MAX_SPL];
    uint8_t demod[MAX_SPL], prev[MAX_SPL], out[MAX_SPL];
    float ang[MAX_SPL];
};
struct fx_entry {
    int32_t conn, nblk, flags, max_lines;
    int64_t in_off;                             // samples from d_s16
    double srate;
    float shift; int32_t pad;
};
struct fx_cfg { int32_t lpm, imagewidth, carrier, deviation, bandwidth, include_headers, phasing, autostop, debug, pad; double nom, srate; };
static_assert(sizeof(fx_entry) == 40 && sizeof(fx_cfg) == 56, "table layout");

// Configure with reset (:467-515) on the device's object
__global__ __launch_bounds__(FX_THREADS) void fax_start_kernel(fx_dev *dev, int conn, fx_cfg c)
{
    fx_dev *d = dev + conn;
    const int tid = (int) threadIdx.x;
    if (tid == 0) {
        cmd_start(d->s, c.lpm, c.imagewidth, c.carrier, c.deviation, c.bandwidth, c.include_headers, c.phasing, c.autostop, c.debug, c.nom, c.srate);
        d->ang_n = 0;
    }
    for (int i = tid; i < MAX_SPL; i += FX_THREADS) { d->samples[i] = 0; d->demod[i] = 0; d->prev[i] = 0; d->out[i] = 0; }
}

struct fx_shared {
    state_t st;
    rec_t rec;
    double ph_inc, next, prevBlend, ang_ph_inc;
    int32_t ang_n, i, nsamps, front, npick, idx0, line, type, need, counted, decode, emit, blend, nrows, nrec, overflow;
    float acc[4];
    long long red[FX_THREADS];
    uint16_t pick[FX_PICKS];
    float f[4 * (FX_CHUNK + FX_HIST)];          // the demodulator's xi, xq, I, Q; the detector's four term arrays
    uint8_t demod[MAX_SPL];
};

// DecodeFaxLine (:162-283) on the line in d->samples; rec.blk / rec.off are set.  All lanes; ends behind a barrier.
__device__ void fx_line(fx_shared &sh, fx_dev *d, double srate, uint8_t *rows, size_t row_stride, kg_fax_rec *recs, int max_lines)
{
    const int tid = (int) threadIdx.x;
    state_t &st = sh.st;
    const int spl = st.spl, w = st.imagewidth, bw = st.bandwidth;
    if (tid == 0) sh.ph_inc = line_begin(st, srate, sh.rec);
    __syncthreads();
    // ---- DemodulateData (:285-334)
    if (!(sh.ang_n >= spl && sh.ang_ph_inc == sh.ph_inc)) {
        if (tid == 0) {
            double f = 0;
            const double ph_inc = sh.ph_inc;
            for (int i = 0; i < spl; i++) { d->ang[i] = mix_angle(f); f = next_f(f, ph_inc); }
        }
        __syncthreads();
        if (tid == 0) { sh.ang_n = spl; sh.ang_ph_inc = sh.ph_inc; }
    }
    float *xi = sh.f, *xq = xi + FX_CHUNK + FX_HIST, *In = xq + FX_CHUNK + FX_HIST, *Qn = In + FX_CHUNK + FX_HIST;      // In[0], Qn[0]: Iprev, Qprev
    const float scale = demod_scale(st.nom, st.deviation);
    if (tid < FX_HIST) { xi[FX_HIST - 1 - tid] = st.hist[0][tid]; xq[FX_HIST - 1 - tid] = st.hist[1][tid]; }
    if (tid == 0) { In[0] = st.Iprev; Qn[0] = st.Qprev; }
    float h16i = st.hist[0][FX_HIST], h16q = st.hist[1][FX_HIST];      // the product 17 back: only the state keeps it
    __syncthreads();
    int n = 0;
    for (int c0 = 0; c0 < spl; c0 += FX_CHUNK) {
        n = spl - c0 < FX_CHUNK ? spl - c0 : FX_CHUNK;
        for (int j = tid; j < n; j += FX_THREADS) mix(d->samples[c0 + j], d->ang[c0 + j], &xi[FX_HIST + j], &xq[FX_HIST + j]);
        __syncthreads();
        for (int j = tid; j < n; j += FX_THREADS) {
            float I = fir17(bw, &xi[FX_HIST + j]), Q = fir17(bw, &xq[FX_HIST + j]);
            normalise(&I, &Q);
            In[1 + j] = I; Qn[1 + j] = Q;
        }
        __syncthreads();
        for (int j = tid; j < n; j += FX_THREADS) sh.demod[c0 + j] = pixel_of(In[1 + j], Qn[1 + j], In[j], Qn[j], scale);
        // what the next chunk (or the next line) starts from: the last 16 products, the one before them, the last I and Q
        float ci = 0, cq = 0, pi = 0, pq = 0;
        if (tid < FX_HIST) { ci = xi[n + tid]; cq = xq[n + tid]; }
        if (tid == 0) { pi = In[n]; pq = Qn[n]; }
        if (tid == 0) { h16i = xi[n - 1]; h16q = xq[n - 1]; }          // window index FX_HIST + (n - 1) - 16
        __syncthreads();
        if (tid < FX_HIST) { xi[tid] = ci; xq[tid] = cq; }
        if (tid == 0) { In[0] = pi; Qn[0] = pq; }
        __syncthreads();
    }
    if (tid == 0) {
        for (int k = 0; k < FX_HIST; k++) { st.hist[0][k] = xi[FX_HIST - 1 - k]; st.hist[1][k] = xq[FX_HIST - 1 - k]; }
        st.hist[0][FX_HIST] = h16i; st.hist[1][FX_HIST] = h16q;
        st.Iprev = In[0]; st.Qprev = Qn[0];
        st.fir_count = (st.fir_count + spl) % TAPS;
    }
    for (int i = tid; i < spl; i += FX_THREADS) d->demod[i] = sh.demod[i];
    // ---- DetectLineType (:117-129)
    if (!st.skip_header_detection) {
        const int len = det_len(spl);
        const float k0 = fourier_k(START_HZ, st.lpm, spl), k1 = fourier_k(STOP_HZ, st.lpm, spl);
        float *t = sh.f;
        float acc = 0;
        for (int c0 = 0; c0 < len; c0 += FX_CHUNK) {
            const int m = len - c0 < FX_CHUNK ? len - c0 : FX_CHUNK;
            __syncthreads();
            for (int j = tid; j < m; j += FX_THREADS) {
                const uint8_t b = sh.demod[c0 + j];
                t[j] = fourier_term(b, k0, c0 + j, 0);
                t[FX_CHUNK + j] = fourier_term(b, k0, c0 + j, 1);
                t[2 * FX_CHUNK + j] = fourier_term(b, k1, c0 + j, 0);
                t[3 * FX_CHUNK + j] = fourier_term(b, k1, c0 + j, 1);
            }
            __syncthreads();
            if ((tid & 63) == 0) {
                const float *mine = t + (tid >> 6) * FX_CHUNK;
                for (int j = 0; j < m; j++) acc += mine[j];
            }
        }
        if ((tid & 63) == 0) sh.acc[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) sh.type = detect_type(fourier_det(sh.acc[0], sh.acc[1], len), fourier_det(sh.acc[2], sh.acc[3], len));
    } else if (tid == 0) sh.type = IMAGE;
    __syncthreads();
    // ---- :178-229
    if (tid == 0) {
        sh.rec.phasing_pos = -1;
        sh.need = machine_pre(st, sh.type, sh.rec) ? 1 : 0;
    }
    __syncthreads();
    if (sh.need) {
        const int nw = wedge_n(spl), incr = wedge_incr(spl, w);
        long long key = 0x7fffffffffffffffLL;
        for (long long i = (long long) tid * incr; i < spl; i += (long long) FX_THREADS * incr) {
            const long long k = ((long long) wedge_total(sh.demod, spl, nw, (int) i) << 32) | i;
            if (k < key) key = k;
        }
        sh.red[tid] = key;
        __syncthreads();
        for (int m = FX_THREADS / 2; m >= 1; m >>= 1) {
            if (tid < m && sh.red[tid + m] < sh.red[tid]) sh.red[tid] = sh.red[tid + m];
            __syncthreads();
        }
        if (tid == 0) sh.rec.phasing_pos = st.phasingPos[st.phasingLinesLeft - 1] = phasing_result((int) (sh.red[0] & 0xffffffffLL), nw, spl);
        __syncthreads();
    }
    // ---- :231-280
    if (tid == 0) {
        const int type = sh.type;
        sh.counted = machine_post(st, type, sh.rec) ? 1 : 0;
        sh.decode = sh.counted && !st.autostopped;
        sh.emit = sh.blend = 0;
        if (sh.decode) {
            bool blend;
            sh.emit = blend_decide(st, &blend, &sh.next, &sh.prevBlend) ? 1 : 0;
            sh.blend = blend ? 1 : 0;
            if (sh.emit && sh.nrows >= max_lines) { sh.emit = 0; sh.overflow = 1; }
        }
    }
    __syncthreads();
    if (sh.counted) {
        if (sh.decode) {
            uint8_t *row = rows + (size_t) sh.nrows * row_stride;
            const bool emit = sh.emit != 0, blend = sh.blend != 0, debug = st.debug != 0;
            const double next = sh.next, prevBlend = sh.prevBlend;
            for (int i = tid; i < w; i += FX_THREADS) {
                const uint8_t img = pixel_avg(sh.demod, spl, w, i);
                uint8_t o = d->out[i];
                if (blend) { o = blend_pixel(img, d->prev[i], next, prevBlend); d->out[i] = o; }
                d->prev[i] = img;
                if (emit) row[1 + i] = debug ? img : o;
            }
            if (tid == 0 && emit) { row[0] = MSG_DRAW; sh.rec.flags |= F_ROW_SENT; }
        } else {
            for (int i = tid; i < w; i += FX_THREADS) d->prev[i] = 0;     // counted, not decoded: DEFINED as zeros
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (sh.emit) sh.nrows++;
        if (sh.counted) machine_tail(st, sh.rec);
        rec_finish(st, sh.type, sh.rec);
        if (sh.nrec < max_lines) {
            kg_fax_rec *o = recs + sh.nrec;
            const rec_t &r = sh.rec;
            o->blk = r.blk; o->off = r.off; o->type = r.type; o->typecount = r.typecount; o->imageline = r.imageline; o->phasingLinesLeft = r.phasingLinesLeft;
            o->skip = r.skip; o->phasing_pos = r.phasing_pos; o->flags = r.flags; o->phasingSkipData = r.phasingSkipData; o->ten_pct = r.ten_pct;
            o->ninety_pct = r.ninety_pct;
            sh.nrec++;
        } else sh.overflow = 1;
        st.samp_idx = 0;
    }
    __syncthreads();
}

// entry e: rows at rows + e * max_lines * row_stride, records at recs + e * max_lines, counts[4 e ..]: rows, records, overflow, 0
__global__ __launch_bounds__(FX_THREADS) void fax_push_kernel(const fx_entry *__restrict__ entries, const int16_t *__restrict__ in, uint8_t *rows, size_t row_stride,
                                                              kg_fax_rec *recs, int32_t *counts, fx_dev *dev)
{
    __shared__ fx_shared sh;
    const fx_entry e = entries[blockIdx.x];
    const int tid = (int) threadIdx.x;
    if (!(e.flags & E_STARTED)) {
        if (tid < 4) counts[4 * blockIdx.x + tid] = 0;
        return;
    }
    fx_dev *d = dev + e.conn;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&d->s);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&sh.st);
        for (int i = tid; i < (int) (sizeof(state_t) / 4); i += FX_THREADS) dst[i] = src[i];
    }
    if (tid == 0) { sh.ang_n = d->ang_n; sh.ang_ph_inc = d->ang_ph_inc; sh.nrows = sh.nrec = sh.overflow = 0; }
    __syncthreads();
    state_t &st = sh.st;
    rows += (size_t) blockIdx.x * (size_t) e.max_lines * row_stride;
    recs += (size_t) blockIdx.x * (size_t) e.max_lines;
    for (int b = 0; b < e.nblk; b++) {
        if (tid == 0) {
            int front;
            sh.nsamps = block_head(st, b == 0 ? e.shift : 0.0f, &front);
            sh.front = front;
            sh.i = 0;
        }
        __syncthreads();
        const int16_t *blk = in + e.in_off + (int64_t) b * BLK + sh.front;
        const int nsamps = sh.nsamps;
        for (;;) {
            const int i_now = sh.i;
            __syncthreads();
            if (i_now >= nsamps) break;
            if (tid == 0) {                                             // :427-432, at most FX_PICKS picks at a time
                int np = 0, i = i_now, idx = st.samp_idx;             // the chain in registers: one LDS store an iteration
                const int spl = st.spl;
                const double ratio = st.ratio;
                double fi = st.fi;
                sh.idx0 = idx;
                while (i < nsamps && idx < spl && np < FX_PICKS) {
                    sh.pick[np++] = (uint16_t) i;
                    idx++;
                    fi += ratio;
                    i = (int) trunc(fi);
                }
                st.samp_idx = idx; st.fi = fi;
                sh.i = i; sh.npick = np;
                sh.line = idx == spl;
            }
            __syncthreads();
            const int np = sh.npick, idx0 = sh.idx0;
            for (int k = tid; k < np; k += FX_THREADS) d->samples[idx0 + k] = blk[sh.pick[k]];
            __syncthreads();
            if (sh.line) {
                if (tid == 0) {
                    rec_t z = {};
                    z.blk = b; z.off = sh.i;
                    sh.rec = z;
                }
                fx_line(sh, d, e.srate, rows, row_stride, recs, e.max_lines);
            }
        }
        if (tid == 0) st.fi -= nsamps;
        __syncthreads();
    }
    {
        uint32_t *dst = reinterpret_cast<uint32_t *>(&d->s);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&sh.st);
        for (int i = tid; i < (int) (sizeof(state_t) / 4); i += FX_THREADS) dst[i] = src[i];
    }
    if (tid == 0) {
        d->ang_n = sh.ang_n; d->ang_ph_inc = sh.ang_ph_inc;
        counts[4 * blockIdx.x] = sh.nrows; counts[4 * blockIdx.x + 1] = sh.nrec; counts[4 * blockIdx.x + 2] = sh.overflow; counts[4 * blockIdx.x + 3] = 0;
    }
}

struct fx_conn {                                // what the commands alone decide
    int configured, started, spl, imagewidth;
    double nom;
    float shift;                                // fax_t::shift (fax.cpp:28): the next pushed block takes it
};

struct kg_fax {
    kg_ctx *ctx;
    int nconn;
    std::vector<fx_conn> c;
    kg_dbuf<fx_dev> d_state;                    // [nconn]
};

// The checks of a push and its table.  took: the started connections of the list with blocks (their pending shift goes with the push).
static int fx_table(kg_fax *q, const int32_t *conns, int nconn, const int32_t *nblk, const int64_t *in_off, size_t stride, const double *srate, size_t row_stride,
                    int max_lines, std::vector<fx_entry> &tab, std::vector<int> &took, const char *who)
{
    KG_REQUIRE(nconn >= 1 && nconn <= q->nconn, KG_ERR_INVALID, "%s: nconn %d (1..%d)", who, nconn, q->nconn);
    KG_REQUIRE(max_lines >= 0, KG_ERR_INVALID, "%s: max_lines %d", who, max_lines);
    std::vector<char> listed((size_t) q->nconn, 0);
    for (int i = 0; i < nconn; i++) {
        const int c = conns[i];
        KG_TRY(kg_ext_list_entry(who, listed, nconn, i, c, nblk[i], FX_MAX_BLK, "stride", stride, BLK, in_off != nullptr, "sample offset", in_off ? in_off[i] : 0));
        const fx_conn &k = q->c[c];
        fx_entry e;
        memset(&e, 0, sizeof e);
        e.conn = c; e.nblk = nblk[i]; e.max_lines = max_lines;
        e.in_off = in_off ? in_off[i] : (int64_t) ((size_t) i * stride);
        if (k.started && nblk[i] > 0) {                                // fax_task is not woken for anybody else: the samples go nowhere
            KG_REQUIRE(srate[i] >= k.nom / 2 && srate[i] <= k.nom * 2, KG_ERR_INVALID, "%s: sample rate %g of connection %d (nominal %g: %g .. %g)", who, srate[i], c,
                       k.nom, k.nom / 2, k.nom * 2);
            KG_REQUIRE(max_lines >= lines_bound(k.spl, nblk[i]), KG_ERR_INVALID, "%s: max_lines %d; %d blocks of connection %d can complete %d lines", who, max_lines,
                       nblk[i], c, lines_bound(k.spl, nblk[i]));
            KG_REQUIRE(row_stride >= (size_t) k.imagewidth + 1, KG_ERR_INVALID, "%s: row_stride %zu; a row of connection %d has %d bytes", who, row_stride, c,
                       k.imagewidth + 1);
            e.flags = E_STARTED; e.srate = srate[i]; e.shift = k.shift;
            took.push_back(c);
        }
        tab.push_back(e);
    }
    return KG_OK;
}

// kg_fax_push on device memory, samples and outputs alike, with entry i's samples at in_off[i] samples from d_s16 (null: i * stride).  Enqueue only.
int kg_fax_push_at_(kg_fax *q, const int32_t *conns, int nconn, const int32_t *nblk, const int64_t *in_off, const int16_t *d_s16, size_t stride, const double *srate,
                    uint8_t *d_rows, size_t row_stride, kg_fax_rec *d_recs, int max_lines, int32_t *d_counts)
{
    KG_REQUIRE(q && conns && nblk && d_s16 && srate && d_rows && d_recs && d_counts, KG_ERR_INVALID, "kg_fax_push: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_REQUIRE(KG_ALIGNED(d_s16, 2) && KG_ALIGNED(d_recs, 4) && KG_ALIGNED(d_counts, 4), KG_ERR_INVALID, "kg_fax_push: the samples must be 2-byte aligned, records and counts 4-byte aligned");
    std::vector<fx_entry> tab;
    std::vector<int> took;
    KG_TRY(fx_table(q, conns, nconn, nblk, in_off, stride, srate, row_stride, max_lines, tab, took, "kg_fax_push"));
    void *d_tab = nullptr;
    if ((rc = kg_ctx_stage(q->ctx, tab.data(), sizeof(fx_entry) * tab.size(), &d_tab))) return rc;
    KG_PLAN_ONLY(q->ctx);
    hipLaunchKernelGGL(fax_push_kernel, dim3((unsigned) tab.size()), dim3(FX_THREADS), 0, q->ctx->stream, (const fx_entry *) d_tab, d_s16, d_rows, row_stride, d_recs,
                       d_counts, q->d_state.p);
    KG_HIP(hipGetLastError());
    for (int c : took) q->c[c].shift = 0;                              // commit: the enqueue succeeded (fax.cpp:88)
    return KG_OK;
}

// what the table of a push over nconn connections takes (and its alignment)
size_t kg_fax_table_bytes_(size_t nconn) { return 64 + nconn * sizeof(fx_entry); }

// a fresh object for the connection (a receiver joined or left): zeroed, as the static m_FaxDecoder[] begins.  Enqueue only.
int kg_fax_reset_(kg_fax *q, int conn)
{
    KG_REQUIRE(q != nullptr && conn >= 0 && conn < q->nconn, KG_ERR_INVALID, "kg_fax: connection %d", conn);
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_HIP(hipMemsetAsync(q->d_state.p + conn, 0, sizeof(fx_dev), q->ctx->stream));
    memset(&q->c[conn], 0, sizeof q->c[conn]);
    return KG_OK;
}

extern "C" {

int kg_fax_create(kg_ctx *ctx, int nconn, kg_fax **out)
{
    return kg_ext_create(ctx, nconn, FX_MAX_CONNS, "kg_fax_create", "nconn", out, [=](kg_fax *q) {
        q->nconn = nconn;
        q->c.resize(nconn);
        for (fx_conn &c : q->c) memset(&c, 0, sizeof c);
        KG_TRY(q->d_state.alloc((size_t) nconn, "kg_fax_create: connection state"));
        return kg_ext_zero(ctx, q->d_state.p, (size_t) nconn, "kg_fax_create");
    });
}

void kg_fax_destroy(kg_fax *q) { kg_drain_delete(q); }

int kg_fax_start(kg_fax *q, int conn, int lpm, int imagewidth, int carrier, int deviation, int bandwidth, int include_headers, int phasing, int autostop, int debug,
                 double nom_rate, double srate)
{
    KG_EXT_INDEX("kg_fax_start", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    int spl = 0;
    const int bad = start_check(lpm, imagewidth, deviation, bandwidth, nom_rate, srate, &spl);
    KG_REQUIRE(bad != REFUSED_LPM, KG_ERR_INVALID, "kg_fax_start: lpm %d (1 or more)", lpm);
    KG_REQUIRE(bad != REFUSED_DEVIATION, KG_ERR_INVALID, "kg_fax_start: deviation 0 (the reference divides by it)");
    KG_REQUIRE(bad != REFUSED_BANDWIDTH, KG_ERR_INVALID, "kg_fax_start: bandwidth %d (0 narrow, 1 middle, 2 wide)", bandwidth);
    KG_REQUIRE(bad != REFUSED_WIDTH, KG_ERR_INVALID, "kg_fax_start: imagewidth %d (1 or more)", imagewidth);
    KG_REQUIRE(bad != REFUSED_RATE, KG_ERR_INVALID, "kg_fax_start: nominal rate %g (1 .. 1e6), sample rate %g (half to twice the nominal)", nom_rate, srate);
    KG_REQUIRE(bad != REFUSED_SPL_MAX, KG_ERR_INVALID, "kg_fax_start: %g samples a line at %d lpm and %g Hz (at most %d)", nom_rate * 60.0 / lpm, lpm, nom_rate, MAX_SPL);
    KG_REQUIRE(bad != REFUSED_SPL_WIDTH, KG_ERR_INVALID, "kg_fax_start: %d samples a line below the imagewidth %d (the reference's phasing loop never ends)", spl,
               imagewidth);
    KG_REQUIRE(bad == 0, KG_ERR_INVALID, "kg_fax_start: refused (%d)", bad);
    fx_cfg c = {lpm, imagewidth, carrier, deviation, bandwidth, include_headers, phasing, autostop, debug, 0, nom_rate, srate};
    KG_PLAN_ONLY(q->ctx);
    hipLaunchKernelGGL(fax_start_kernel, dim3(1), dim3(FX_THREADS), 0, q->ctx->stream, q->d_state.p, conn, c);
    KG_HIP(hipGetLastError());
    fx_conn &k = q->c[conn];
    k.configured = 1; k.started = 1; k.spl = spl; k.imagewidth = imagewidth; k.nom = nom_rate;
    return KG_OK;
}

int kg_fax_set_shift(kg_fax *q, int conn, float shift)
{
    KG_EXT_INDEX("kg_fax_set_shift", q, conn, q->nconn, "connection");
    KG_REQUIRE(shift_ok(shift), KG_ERR_INVALID, "kg_fax_set_shift: shift %g (0 .. 1: a negative skip walks the sample pointer backwards)", (double) shift);
    q->c[conn].shift = shift;
    return KG_OK;
}

int kg_fax_stop(kg_fax *q, int conn)
{
    KG_EXT_INDEX("kg_fax_stop", q, conn, q->nconn, "connection");
    q->c[conn].started = 0;                     // fax_close (fax.cpp:94-107): the task goes, fax_t is cleared; the decoder stays
    q->c[conn].shift = 0;
    return KG_OK;
}

int kg_fax_max_lines(kg_fax *q, const int32_t *conns, int nconn, const int32_t *nblk, int32_t *max_lines_out, int32_t *max_width)
{
    KG_REQUIRE(q && conns && nblk && nconn >= 1, KG_ERR_INVALID, "kg_fax_max_lines: bad argument");
    int ml = 0, mw = 0;
    for (int i = 0; i < nconn; i++) {
        KG_REQUIRE(conns[i] >= 0 && conns[i] < q->nconn && nblk[i] >= 0, KG_ERR_INVALID, "kg_fax_max_lines: entry %d", i);
        const fx_conn &k = q->c[conns[i]];
        if (!k.started || nblk[i] == 0) continue;
        const int m = lines_bound(k.spl, nblk[i]);
        if (m > ml) ml = m;
        if (k.imagewidth > mw) mw = k.imagewidth;
    }
    if (max_lines_out) *max_lines_out = ml;
    if (max_width) *max_width = mw;
    return KG_OK;
}

int kg_fax_push(kg_fax *q, const int32_t *conns, int nconn, const int32_t *nblk, const int16_t *s16, size_t stride, const double *srate, uint8_t *rows,
                size_t row_stride, kg_fax_rec *recs, int max_lines, int32_t *counts)
{
    KG_REQUIRE(q && conns && nblk && s16 && srate && rows && recs && counts, KG_ERR_INVALID, "kg_fax_push: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    {   // checked ahead of the first copy: a push that will be refused enqueues nothing here either
        std::vector<fx_entry> tab;
        std::vector<int> took;
        KG_TRY(fx_table(q, conns, nconn, nblk, nullptr, stride, srate, row_stride, max_lines, tab, took, "kg_fax_push"));
    }
    size_t last = 0;
    for (int i = 0; i < nconn; i++)
        if (nblk[i] > 0) last = (size_t) i * stride + (size_t) BLK * nblk[i];
    const size_t nrow_bytes = (size_t) nconn * (size_t) max_lines * row_stride, nrec = (size_t) nconn * (size_t) max_lines;
    int16_t *d_s16 = nullptr;
    uint8_t *d_rows = nullptr;
    kg_fax_rec *d_recs = nullptr;
    int32_t *d_counts = nullptr;
    hipStream_t s = q->ctx->stream;
    kg_scope tmp(q->ctx);                               // the caller's arrays and the temporaries are in use until it has drained the stream
    KG_TRY(tmp.alloc(&d_s16, last ? last : 1, "kg_fax_push: samples"));
    KG_TRY(tmp.alloc(&d_rows, nrow_bytes ? nrow_bytes : 1, "kg_fax_push: rows"));
    KG_TRY(tmp.alloc(&d_recs, nrec ? nrec : 1, "kg_fax_push: records"));
    KG_TRY(tmp.alloc(&d_counts, (size_t) 4 * nconn, "kg_fax_push: counts"));
    for (int i = 0; i < nconn; i++)
        if (nblk[i] > 0)
            KG_HIP(hipMemcpyAsync(d_s16 + (size_t) i * stride, s16 + (size_t) i * stride, sizeof(int16_t) * BLK * (size_t) nblk[i], hipMemcpyHostToDevice, s));
    KG_TRY(kg_fax_push_at_(q, conns, nconn, nblk, nullptr, d_s16, stride, srate, d_rows, row_stride, d_recs, max_lines, d_counts));
    KG_HIP(hipMemcpyAsync(counts, d_counts, sizeof(int32_t) * 4 * (size_t) nconn, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < nconn; i++) {                   // the rows and records the device counted, nothing else of the caller's arrays
        const size_t nr = (size_t) counts[4 * i], nl = (size_t) counts[4 * i + 1];
        if (nr) KG_HIP(hipMemcpyAsync(rows + (size_t) i * max_lines * row_stride, d_rows + (size_t) i * max_lines * row_stride, nr * row_stride, hipMemcpyDeviceToHost, s));
        if (nl) KG_HIP(hipMemcpyAsync(recs + (size_t) i * max_lines, d_recs + (size_t) i * max_lines, sizeof(kg_fax_rec) * nl, hipMemcpyDeviceToHost, s));
    }
    KG_HIP(hipStreamSynchronize(s));
    return KG_OK;                                       // tmp drains the stream
}

int kg_fax_state(kg_fax *q, int conn, kg_fax_info *info, int16_t *samples, uint8_t *demod, uint8_t *prev, uint8_t *out)
{
    KG_EXT_INDEX("kg_fax_state", q, conn, q->nconn, "connection");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const fx_dev *d = q->d_state.p + conn;
    hipStream_t s = q->ctx->stream;
    state_t st;
    KG_HIP(hipMemcpyAsync(&st, &d->s, sizeof st, hipMemcpyDeviceToHost, s));
    if (samples) KG_HIP(hipMemcpyAsync(samples, d->samples, sizeof d->samples, hipMemcpyDeviceToHost, s));
    if (demod) KG_HIP(hipMemcpyAsync(demod, d->demod, MAX_SPL, hipMemcpyDeviceToHost, s));
    if (prev) KG_HIP(hipMemcpyAsync(prev, d->prev, MAX_SPL, hipMemcpyDeviceToHost, s));
    if (out) KG_HIP(hipMemcpyAsync(out, d->out, MAX_SPL, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    if (prev && st.imageline == 0) memset(prev, 0, MAX_SPL);           // no line counted yet: the reference has no previous line
    if (info) {
        memset(info, 0, sizeof *info);
        info->nom = st.nom; info->frac = st.frac; info->frac_prev = st.frac_prev; info->ratio = st.ratio; info->fi = st.fi; info->lineIncrFrac = st.lineIncrFrac;
        info->lineIncrAcc = st.lineIncrAcc; info->lineBlend = st.lineBlend; info->carrier = st.carrier; info->deviation = st.deviation;
        info->lpm = st.lpm; info->imagewidth = st.imagewidth; info->bandwidth = st.bandwidth; info->include_headers = st.include_headers;
        info->use_phasing = st.use_phasing; info->autostop = st.autostop; info->autostopped = st.autostopped; info->debug = st.debug;
        info->skip_header_detection = st.skip_header_detection; info->spl = st.spl; info->skip = st.skip; info->samp_idx = st.samp_idx; info->lasttype = st.lasttype;
        info->typecount = st.typecount; info->imageline = st.imageline; info->phasingLinesLeft = st.phasingLinesLeft; info->phasingSkipData = st.phasingSkipData;
        info->have_phasing = st.have_phasing;
        fir_circular(st, info->fir, &info->fir_current);
        info->started = q->c[conn].started;
        info->Iprev = st.Iprev; info->Qprev = st.Qprev;
        memcpy(info->phasingPos, st.phasingPos, sizeof info->phasingPos);
        info->shift = q->c[conn].shift;
    }
    return KG_OK;
}

}  // extern "C"
