// kg_iqd.hip -- the IQ display extension (extensions/IQ_display/iq_display.cpp; csrc/kg_iqd.h is the one definition of its arithmetic).
//
// The schedule of display_data (:71-111: ring positions, rows, maN, nsamp) depends on no sample, so the host walks it per call and hands
// the kernel a table: per listed channel a group {channel, its blocks' range in the op list, what the commands left: draw, display
// mode, exponent, MSK, points, gain, the PLLs' coefficients}, per block an op {where its samples are, instance, ring position and maN
// at its start, where its first row and its status record go}.  ONE launch per call: one workgroup of ONE wave64 per listed channel,
// the channel's blocks in order.  Per sample the work is a chain, but only a thin part of it is; per block of up to 512 samples:
//   A  s * s, or the repeated-squaring power, of every sample: state-free, lane-parallel (8 samples a lane), into LDS;
//   B  pll::update over the block -- fmodf, sincos, one complex multiply, atan2f, the loop filter: the serial spine, on ONE lane;
//      under MSK the two PLLs are independent given A and walk in two lanes at once.  The phase of every sample goes to LDS;
//   C  the recovered carrier (sincos), multiply or replace, hypotf: lane-parallel;
//   D  cma.re, cma.im and ama: three independent recurrences of a few float operations a sample, in THREE lanes at once; the ama behind
//      every sample goes to LDS (auto gain scales a sample with it);
//   E  to_u1, plot / map / iq and the rows, lane-parallel lap by lap: within a lap of the ring every sample has a place of its own;
//      a lap's row is copied (16 bytes a lane and pass where the row's place allows it) behind a barrier, and a second barrier keeps
//      the next lap from overwriting what the copy still reads.
// With the PLL off A to C's PLL part falls away.  Nothing is reassociated.  One wave a workgroup: a barrier costs a wait for the
// wave's own memory operations, and 14 channels land on 14 compute units.
#include "kg_ext.h"
#include "kg_iqd.h"

using namespace kg_iqd_cf;

static_assert(RING == KG_IQD_RING && MAX_NS == KG_IQD_MAX_NS && POINTS == KG_IQD_POINTS && DENSITY == KG_IQD_DENSITY, "constants");
static_assert(sizeof(kg_iqd_status) == 24 && sizeof(status_t) == 24 && offsetof(kg_iqd_status, df) == offsetof(status_t, df) &&
              offsetof(kg_iqd_status, phase) == offsetof(status_t, phase), "kg_iqd_status layout");
static_assert(sizeof(kg_iqd_row) == 32 && sizeof(kg_iqd_info) == 164, "kg_iqd_row / kg_iqd_info layout");

enum { IQ_LANES = 64, IQ_PER_LANE = MAX_NS / IQ_LANES };
enum { IQ_MAX_CHANS = 1024, IQ_MAX_LIST = 4096, IQ_MAX_BLK = 4096, IQ_MAX_OPS = 8192 };
enum { Z_ALL = 1, Z_MA = 2, Z_PLL = 4 };
// dyn: what the samples decide
enum { DYN_CMA_RE = 0, DYN_CMA_IM = 1, DYN_AMA = 2, DYN_PLL = 4, DYN_N = 16 };          // DYN_PLL + 3 k: df, phase, ud of PLL k

struct iq_dev {                                 // one channel: _iq, _plot, _map (416 KiB) and the scalars the samples decide
    float2 iq[NCH][RING];
    uchar4 plot[NCH][RING];                     // old.re, old.im, new.re, new.im
    uchar2 map[RING];
    float dyn[DYN_N];
};
static_assert(sizeof(iq_dev) == 416 * 1024 + 64, "device state");

struct iq_group {
    int32_t ch, first, nops, flags, draw, dmode, exponent, msk, points, cap, ns, pad0;
    float gain, fs, pad1[2];
    float pll[3][4];                            // fc, b0, b1
};
struct iq_op { int64_t in_off, row_off; int32_t inst, ring0, maN0, status; };      // in_off: complex samples from d_iq
static_assert(sizeof(iq_group) == 112 && sizeof(iq_op) == 32, "table layout");

// n bytes (even) from src (16-byte aligned) to dst (2-byte aligned)
__device__ __forceinline__ void row_copy(uint8_t *dst, const uint8_t *src, int n, int lane)
{
    if ((((uintptr_t) dst | (uintptr_t) n) & 15) == 0) {
        const uint4 *s = reinterpret_cast<const uint4 *>(src);
        uint4 *d = reinterpret_cast<uint4 *>(dst);
        for (int i = lane; i < n / 16; i += IQ_LANES) d[i] = s[i];
    } else {
        const unsigned short *s = reinterpret_cast<const unsigned short *>(src);
        unsigned short *d = reinterpret_cast<unsigned short *>(dst);
        for (int i = lane; i < n / 2; i += IQ_LANES) d[i] = s[i];
    }
}

__global__ __launch_bounds__(IQ_LANES) void iqd_kernel(const iq_group *__restrict__ groups, const iq_op *__restrict__ ops, const float2 *__restrict__ in,
                                                       uint8_t *rows, status_t *__restrict__ status, iq_dev *dev)
{
    __shared__ float2 s_in[MAX_NS], s_pw[MAX_NS];
    __shared__ float s_ph[2][MAX_NS], s_v[3][MAX_NS], s_ama[MAX_NS], s_dyn[DYN_N];
    const iq_group g = groups[blockIdx.x];
    const int lane = (int) threadIdx.x, ns = g.ns;
    iq_dev *d = dev + g.ch;
    if (g.flags & Z_ALL) {                                                  // a fresh object: every array of it is zero
        uint4 *p = reinterpret_cast<uint4 *>(d);
        for (int i = lane; i < (int) (sizeof(iq_dev) / 16); i += IQ_LANES) p[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    if (lane < DYN_N) {
        float v = d->dyn[lane];
        if ((g.flags & Z_MA) && lane < DYN_PLL) v = 0.0f;
        if ((g.flags & Z_PLL) && lane >= DYN_PLL) v = 0.0f;
        s_dyn[lane] = v;
    }
    __syncthreads();
    const bool on = g.draw == POINTS || g.draw == DENSITY, pll_on = g.exponent != 0;
    for (int k = 0; k < g.nops; k++) {
        const iq_op op = ops[g.first + k];
        if (on) {
            const float2 *src = in + op.in_off;
#pragma unroll
            for (int j = 0; j < IQ_PER_LANE; j++) {
                const int i = lane + IQ_LANES * j;
                if (i < ns) {
                    const float2 x = src[i];
                    s_in[i] = x;
                    if (pll_on) {                                               // A
                        cf s; s.re = x.x; s.im = x.y;
                        const cf p = g.msk ? cmul(s, s) : cpow_u(s, (unsigned) g.exponent);
                        s_pw[i] = make_float2(p.re, p.im);
                    }
                }
            }
            __syncthreads();
            if (pll_on) {
                if (lane < (g.msk ? 2 : 1)) {                                   // B
                    const int w = g.msk ? 1 + lane : 0;
                    pll_t p;
                    const float *co = groups[blockIdx.x].pll[w];               // (not g.pll[w]: a lane-dependent index would put g in scratch)
                    p.fs = g.fs; p.fc = co[0]; p.b0 = co[1]; p.b1 = co[2];
                    p.df = s_dyn[DYN_PLL + 3 * w]; p.phase = s_dyn[DYN_PLL + 3 * w + 1]; p.ud = s_dyn[DYN_PLL + 3 * w + 2];
                    for (int i = 0; i < ns; i++) {
                        const float2 x = s_pw[i];
                        cf s; s.re = x.x; s.im = x.y;
                        s_ph[lane][i] = pll_update(p, s);
                    }
                    s_dyn[DYN_PLL + 3 * w] = p.df; s_dyn[DYN_PLL + 3 * w + 1] = p.phase; s_dyn[DYN_PLL + 3 * w + 2] = p.ud;
                }
                __syncthreads();
            }
#pragma unroll
            for (int j = 0; j < IQ_PER_LANE; j++) {                             // C
                const int i = lane + IQ_LANES * j;
                if (i < ns) {
                    const float2 x = s_in[i];
                    cf s; s.re = x.x; s.im = x.y;
                    if (pll_on) {
                        const cf c = g.msk ? carrier_msk(s_ph[1][i], s_ph[0][i]) : carrier_single(s_ph[0][i], g.exponent);
                        s = g.dmode == 0 ? cmul(s, c) : c;
                    }
                    s_v[0][i] = s.re; s_v[1][i] = s.im; s_v[2][i] = hypotf_dbl(s.re, s.im);
                }
            }
            __syncthreads();
            if (lane < 3) {                                                     // D
                float acc = s_dyn[lane];
                for (int i = 0; i < ns; i++) {
                    acc = ma_step(acc, s_v[lane][i], ma_count(op.maN0, i, g.cap));
                    if (lane == 2) s_ama[i] = acc;
                }
                s_dyn[lane] = acc;
            }
            __syncthreads();
            // E: lap by lap
            const int ch = op.inst, P = g.points;
            const float fixed = scale_fixed(g.gain, ch);
            const bool autog = g.gain == 0.0f;
            const int rlen = g.draw == POINTS ? P * 4 : P * 2;
            uint8_t *row = rows + op.row_off;
            int r = op.ring0;
            for (int done = 0; done < ns;) {
                const int room = P - r > 1 ? P - r : 1;
                const int lap = ns - done < room ? ns - done : room;
                for (int i = lane; i < lap; i += IQ_LANES) {
                    const int s = done + i, pos = r + i;
                    const float sc = autog ? scale_auto(s_ama[s]) : fixed;
                    const float re = s_v[0][s], im = s_v[1][s];
                    if (g.draw == POINTS) {
                        const float2 old = d->iq[ch][pos];
                        d->plot[ch][pos] = make_uchar4(u1(old.x, sc), u1(old.y, sc), u1(re, sc), u1(im, sc));
                        d->iq[ch][pos] = make_float2(re, im);
                    } else {
                        d->map[pos] = make_uchar2(u1(re, sc), u1(im, sc));
                    }
                }
                done += lap; r += lap;
                __syncthreads();
                if (r >= P) {
                    row_copy(row, g.draw == POINTS ? reinterpret_cast<const uint8_t *>(d->plot[ch]) : reinterpret_cast<const uint8_t *>(d->map), rlen, lane);
                    row += rlen;
                    r = 0;
                    __syncthreads();
                }
            }
        }
        if (lane == 0)
            status[op.status] = status_of(s_dyn[DYN_CMA_RE], s_dyn[DYN_CMA_IM], g.exponent, g.msk, s_dyn[DYN_PLL], s_dyn[DYN_PLL + 1], s_dyn[DYN_PLL + 3],
                                          s_dyn[DYN_PLL + 4], s_dyn[DYN_PLL + 6], s_dyn[DYN_PLL + 7]);
        __syncthreads();
    }
    if (lane < DYN_N) d->dyn[lane] = s_dyn[lane];
}

// ---- hypotf / fmodf over two arrays: what tests/test_iqd_gpu.py holds to the host's libm
__global__ void iqd_math_kernel(int fn, const float *__restrict__ a, const float *__restrict__ b, size_t n, float *__restrict__ out)
{
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
        out[i] = fn == KG_IQD_MATH_HYPOTF ? hypotf_dbl(a[i], b[i]) : fmodf_exact(a[i], b[i]);
}

struct iq_chan {
    state_t st;                                 // the samples' part of it (cma, ama, the PLLs' df / phase / ud) lives on the device
    int zflags;                                 // Z_*: what the channel's next block is to zero first
};

struct kg_iqd {
    kg_ctx *ctx;
    int nchan;
    std::vector<iq_chan> ch;
    kg_dbuf<iq_dev> d_state;                    // [nchan]
};

struct iq_plan {
    std::vector<iq_chan> ch;                    // copies of the listed channels, in order of first appearance
    std::vector<int> slot, chan;
    std::vector<std::vector<iq_op>> ops;
    std::vector<kg_iqd_row> rows;
    std::vector<int32_t> sent;                  // per block of the call
    size_t row_bytes = 0;
};

static int iq_walk(kg_iqd *q, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const int32_t *iq_row, int ns, size_t iq_stride, size_t rows_cap,
                   size_t status_cap, int max_rows, bool want_rows, iq_plan &p, const char *who)
{
    KG_REQUIRE(nch >= 1 && nch <= IQ_MAX_LIST, KG_ERR_INVALID, "%s: nch %d (1..%d)", who, nch, IQ_MAX_LIST);
    KG_REQUIRE(ns >= 1 && ns <= MAX_NS, KG_ERR_INVALID, "%s: ns %d (1..%d)", who, ns, MAX_NS);
    KG_REQUIRE(max_rows >= 0, KG_ERR_INVALID, "%s: max_rows %d", who, max_rows);
    p.slot.assign(q->nchan, -1);
    int32_t samp[MAX_NS];
    size_t nblocks = 0;
    for (int i = 0; i < nch; i++) {
        const int c = chans[i];
        KG_REQUIRE(c >= 0 && c < q->nchan, KG_ERR_INVALID, "%s: chans[%d] = %d of %d", who, i, c, q->nchan);
        KG_REQUIRE(nblk[i] >= 0 && nblk[i] <= IQ_MAX_BLK, KG_ERR_INVALID, "%s: nblk[%d] = %d (0..%d)", who, i, nblk[i], IQ_MAX_BLK);
        KG_REQUIRE(inst[i] == 0 || inst[i] == 1, KG_ERR_INVALID, "%s: inst[%d] = %d (0 or 1)", who, i, inst[i]);
        KG_REQUIRE(nblk[i] <= 0 || nch == 1 || iq_stride >= (size_t) ns * nblk[i], KG_ERR_INVALID, "%s: iq_stride %zu below the %d blocks of entry %d", who,
                   iq_stride, nblk[i], i);
        KG_REQUIRE(!iq_row || iq_row[i] >= 0, KG_ERR_INVALID, "%s: sample row %d of entry %d", who, iq_row ? iq_row[i] : 0, i);
        KG_REQUIRE(q->ch[c].st.inited, KG_ERR_STATE, "%s: channel %d was never initialised (kg_iqd_init)", who, c);
        KG_REQUIRE(q->ch[c].st.rate_set, KG_ERR_STATE, "%s: channel %d has no sample rate (kg_iqd_set_run)", who, c);
        if (p.slot[c] < 0) {
            p.slot[c] = (int) p.ch.size();
            p.ch.push_back(q->ch[c]);
            p.chan.push_back(c);
            p.ops.emplace_back();
        }
        iq_chan &w = p.ch[p.slot[c]];
        for (int b = 0; b < nblk[i]; b++) {
            KG_REQUIRE(nblocks < IQ_MAX_OPS && nblocks < status_cap, KG_ERR_INVALID, "%s: more blocks than status records (%zu) or than %d", who, status_cap,
                       IQ_MAX_OPS);
            iq_op op = {(int64_t) ((size_t) (iq_row ? iq_row[i] : i) * iq_stride + (size_t) ns * b), (int64_t) p.row_bytes, inst[i], w.st.ring[inst[i]], w.st.maN, (int32_t) nblocks};
            const int cmd = row_cmd(w.st, inst[i]), len = row_len(w.st);
            int sent = 0;
            const int n = block_sched(w.st, inst[i], ns, samp, &sent);
            KG_REQUIRE(p.row_bytes + (size_t) n * len <= rows_cap, KG_ERR_INVALID, "%s: more row bytes than the capacity %zu", who, rows_cap);
            KG_REQUIRE(!want_rows || p.rows.size() + n <= (size_t) max_rows, KG_ERR_INVALID, "%s: more rows than max_rows = %d", who, max_rows);
            for (int r = 0; r < n; r++) {
                p.rows.push_back(kg_iqd_row{c, i, b, samp[r], cmd, len, (int64_t) p.row_bytes});
                p.row_bytes += len;
            }
            p.ops[p.slot[c]].push_back(op);
            p.sent.push_back(sent);
            nblocks++;
        }
    }
    return KG_OK;
}

extern "C" {

int kg_iqd_create(kg_ctx *ctx, int nchan, kg_iqd **out)
{
    return kg_ext_create(ctx, nchan, IQ_MAX_CHANS, "kg_iqd_create", "nchan", out, [=](kg_iqd *q) {
        q->nchan = nchan;
        q->ch.resize(nchan);
        for (iq_chan &c : q->ch) { memset(&c.st, 0, sizeof c.st); c.zflags = Z_ALL; }      // Z_ALL: the device state needs no zeroing here
        return q->d_state.alloc((size_t) nchan, "kg_iqd_create: channel state");
    });
}

void kg_iqd_destroy(kg_iqd *q) { kg_drain_delete(q); }

#define IQ_INITED(who)                                                                               \
    KG_EXT_INDEX(who, q, ch, q->nchan, "channel");                                                    \
    KG_REQUIRE(q->ch[ch].st.inited, KG_ERR_STATE, who ": channel %d was never initialised (kg_iqd_init)", ch)

int kg_iqd_init(kg_iqd *q, int ch)
{
    KG_EXT_INDEX("kg_iqd_init", q, ch, q->nchan, "channel");
    fresh(q->ch[ch].st);
    q->ch[ch].zflags = Z_ALL;
    return KG_OK;
}

int kg_iqd_set_run(kg_iqd *q, int ch, int run, double rate)
{
    IQ_INITED("kg_iqd_set_run");
    KG_REQUIRE(cmd_run(q->ch[ch].st, run, rate) == 0, KG_ERR_INVALID, "kg_iqd_set_run: sample rate %g (1 .. 1e9)", rate);
    if (run) q->ch[ch].zflags |= Z_PLL;
    return KG_OK;
}

int kg_iqd_set_gain(kg_iqd *q, int ch, int gain)
{
    IQ_INITED("kg_iqd_set_gain");
    cmd_gain(q->ch[ch].st, gain);
    return KG_OK;
}

int kg_iqd_set_points(kg_iqd *q, int ch, int points)
{
    IQ_INITED("kg_iqd_set_points");
    KG_REQUIRE(cmd_points(q->ch[ch].st, points) == 0, KG_ERR_INVALID, "kg_iqd_set_points: points %d (1..%d)", points, RING);
    return KG_OK;
}

int kg_iqd_set_pll_mode(kg_iqd *q, int ch, int pll_mode, int arg)
{
    IQ_INITED("kg_iqd_set_pll_mode");
    KG_REQUIRE(cmd_pll_mode(q->ch[ch].st, pll_mode, arg) == 0, KG_ERR_INVALID, "kg_iqd_set_pll_mode: a negative exponent (%d) is not ported", arg);
    q->ch[ch].zflags |= Z_PLL;
    return KG_OK;
}

int kg_iqd_set_pll_bandwidth(kg_iqd *q, int ch, float bandwidth)
{
    IQ_INITED("kg_iqd_set_pll_bandwidth");
    cmd_pll_bandwidth(q->ch[ch].st, bandwidth);
    q->ch[ch].zflags |= Z_PLL;
    return KG_OK;
}

int kg_iqd_set_draw(kg_iqd *q, int ch, int draw)
{
    IQ_INITED("kg_iqd_set_draw");
    cmd_draw(q->ch[ch].st, draw);
    return KG_OK;
}

int kg_iqd_set_display_mode(kg_iqd *q, int ch, int display_mode)
{
    IQ_INITED("kg_iqd_set_display_mode");
    cmd_display_mode(q->ch[ch].st, display_mode);
    return KG_OK;
}

int kg_iqd_clear(kg_iqd *q, int ch)
{
    IQ_INITED("kg_iqd_clear");
    cmd_clear(q->ch[ch].st);
    q->ch[ch].zflags |= Z_MA | Z_PLL;
    return KG_OK;
}

int kg_iqd_process_dev(kg_iqd *q, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, int ns, const float *d_iq, size_t iq_stride,
                       uint8_t *d_rows, size_t rows_cap, kg_iqd_status *d_status, size_t status_cap, kg_iqd_row *row_map, int max_rows,
                       int32_t *status_sent)
{
    return kg_iqd_process_rows_(q, chans, nch, nblk, inst, nullptr, ns, d_iq, iq_stride, d_rows, rows_cap, d_status, status_cap, row_map, max_rows, status_sent);
}

}  // extern "C"

// kg_iqd_process_dev with the samples placed by the caller: entry i's blocks from d_iq + 2 * iq_row[i] * iq_stride on (null: row i)
int kg_iqd_process_rows_(kg_iqd *q, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const int32_t *iq_row, int ns, const float *d_iq,
                         size_t iq_stride, uint8_t *d_rows, size_t rows_cap, kg_iqd_status *d_status, size_t status_cap, kg_iqd_row *row_map, int max_rows,
                         int32_t *status_sent)
{
    KG_REQUIRE(q && chans && nblk && inst && d_iq && d_rows && d_status, KG_ERR_INVALID, "kg_iqd_process_dev: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_REQUIRE(KG_ALIGNED(d_iq, 8) && KG_ALIGNED(d_rows, 16) && KG_ALIGNED(d_status, 8), KG_ERR_INVALID,
               "kg_iqd_process_dev: d_iq and d_status must be 8-byte aligned, d_rows 16-byte aligned");
    iq_plan p;
    KG_TRY(iq_walk(q, chans, nch, nblk, inst, iq_row, ns, iq_stride, rows_cap, status_cap, max_rows, row_map != nullptr, p, "kg_iqd_process_dev"));
    std::vector<int> of_group;
    size_t nops = 0;
    for (size_t k = 0; k < p.ch.size(); k++)
        if (!p.ops[k].empty()) { of_group.push_back((int) k); nops += p.ops[k].size(); }
    if (!of_group.empty()) {
        std::vector<unsigned char> tab(sizeof(iq_group) * of_group.size() + sizeof(iq_op) * nops);
        iq_group *g = reinterpret_cast<iq_group *>(tab.data());
        iq_op *o = reinterpret_cast<iq_op *>(tab.data() + sizeof(iq_group) * of_group.size());
        int32_t first = 0;
        for (size_t j = 0; j < of_group.size(); j++) {
            const int k = of_group[j];
            const state_t &st = q->ch[p.chan[k]].st;                     // the commands' part: what it was when the call began
            iq_group &e = g[j];
            memset(&e, 0, sizeof e);
            e.ch = p.chan[k]; e.first = first; e.nops = (int32_t) p.ops[k].size(); e.flags = q->ch[p.chan[k]].zflags;
            e.draw = st.draw; e.dmode = st.display_mode; e.exponent = st.exponent; e.msk = st.msk_mode; e.points = st.points; e.cap = ma_cap(st);
            e.ns = ns; e.gain = st.gain; e.fs = st.fs;
            for (int w = 0; w < 3; w++) { e.pll[w][0] = st.pll[w].fc; e.pll[w][1] = st.pll[w].b0; e.pll[w][2] = st.pll[w].b1; }
            memcpy(o + first, p.ops[k].data(), sizeof(iq_op) * p.ops[k].size());
            first += (int32_t) p.ops[k].size();
        }
        void *d_tab = nullptr;
        if ((rc = kg_ctx_stage(q->ctx, tab.data(), tab.size(), &d_tab))) return rc;
        KG_PLAN_ONLY(q->ctx);
        hipLaunchKernelGGL(iqd_kernel, dim3((unsigned) of_group.size()), dim3(IQ_LANES), 0, q->ctx->stream, (const iq_group *) d_tab,
                           (const iq_op *) ((const unsigned char *) d_tab + sizeof(iq_group) * of_group.size()), (const float2 *) d_iq, d_rows,
                           (status_t *) d_status, q->d_state.p);
        KG_HIP(hipGetLastError());
    } else {
        KG_PLAN_ONLY(q->ctx);
    }
    for (size_t k = 0; k < p.ch.size(); k++)                             // commit: the schedule advanced, the zeroing is enqueued
        if (!p.ops[k].empty()) { q->ch[p.chan[k]] = p.ch[k]; q->ch[p.chan[k]].zflags = 0; }
    if (row_map && !p.rows.empty()) memcpy(row_map, p.rows.data(), sizeof(kg_iqd_row) * p.rows.size());
    if (status_sent && !p.sent.empty()) memcpy(status_sent, p.sent.data(), sizeof(int32_t) * p.sent.size());
    return (int) p.rows.size();
}

extern "C" {

int kg_iqd_process(kg_iqd *q, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, int ns, const float *iq, size_t iq_stride,
                   uint8_t *rows, size_t rows_cap, kg_iqd_status *status, size_t status_cap, kg_iqd_row *row_map, int max_rows, int32_t *status_sent)
{
    KG_REQUIRE(q && chans && nblk && inst && iq && rows && status && row_map, KG_ERR_INVALID, "kg_iqd_process: null argument");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    KG_REQUIRE(nch >= 1 && nch <= IQ_MAX_LIST && ns >= 1 && ns <= MAX_NS, KG_ERR_INVALID, "kg_iqd_process: nch %d (1..%d), ns %d (1..%d)", nch, IQ_MAX_LIST, ns,
               MAX_NS);
    size_t last = 0, nblocks = 0;
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(nblk[i] >= 0 && nblk[i] <= IQ_MAX_BLK, KG_ERR_INVALID, "kg_iqd_process: nblk[%d] = %d (0..%d)", i, nblk[i], IQ_MAX_BLK);
        KG_REQUIRE(nblk[i] <= 0 || nch == 1 || iq_stride >= (size_t) ns * nblk[i], KG_ERR_INVALID, "kg_iqd_process: iq_stride %zu below the %d blocks of entry %d",
                   iq_stride, nblk[i], i);
        if (nblk[i] > 0) last = (size_t) i * iq_stride + (size_t) ns * nblk[i];
        nblocks += (size_t) nblk[i];
    }
    KG_REQUIRE(nblocks <= status_cap, KG_ERR_INVALID, "kg_iqd_process: %zu blocks, %zu status records", nblocks, status_cap);
    {   // the schedule is walked (on copies) ahead of the first copy: a call that will be refused enqueues nothing here either
        iq_plan p;
        KG_TRY(iq_walk(q, chans, nch, nblk, inst, nullptr, ns, iq_stride, rows_cap, nblocks, max_rows, true, p, "kg_iqd_process"));
    }
    float *d_iq = nullptr;
    uint8_t *d_rows = nullptr;
    kg_iqd_status *d_status = nullptr;
    hipStream_t s = q->ctx->stream;
    kg_scope tmp(q->ctx);                               // the caller's arrays and the temporaries are in use until it has drained the stream
    KG_TRY(tmp.alloc(&d_iq, 2 * (last ? last : 1), "kg_iqd_process: samples"));
    KG_TRY(tmp.alloc(&d_rows, rows_cap ? rows_cap : 1, "kg_iqd_process: rows"));
    KG_TRY(tmp.alloc(&d_status, nblocks ? nblocks : 1, "kg_iqd_process: status"));
    for (int i = 0; i < nch; i++)
        if (nblk[i] > 0)
            KG_HIP(hipMemcpyAsync(d_iq + 2 * (size_t) i * iq_stride, iq + 2 * (size_t) i * iq_stride, sizeof(float) * 2 * ns * (size_t) nblk[i],
                                  hipMemcpyHostToDevice, s));
    const int n = kg_iqd_process_dev(q, chans, nch, nblk, inst, ns, d_iq, iq_stride, d_rows, rows_cap, d_status, nblocks, row_map, max_rows, status_sent);
    if (n < 0) return n;
    size_t bytes = 0;
    for (int r = 0; r < n; r++) bytes = (size_t) row_map[r].off + (size_t) row_map[r].len;
    if (bytes) KG_HIP(hipMemcpyAsync(rows, d_rows, bytes, hipMemcpyDeviceToHost, s));
    if (nblocks) KG_HIP(hipMemcpyAsync(status, d_status, sizeof(kg_iqd_status) * nblocks, hipMemcpyDeviceToHost, s));
    return n;                                           // tmp drains the stream
}

int kg_iqd_state(kg_iqd *q, int ch, kg_iqd_info *info, float *iq, uint8_t *plot, uint8_t *map)
{
    KG_EXT_INDEX("kg_iqd_state", q, ch, q->nchan, "channel");
    int rc = kg_ctx_use(q->ctx);
    if (rc) return rc;
    const iq_chan &c = q->ch[ch];
    const iq_dev *d = q->d_state.p + ch;
    hipStream_t s = q->ctx->stream;
    float dyn[DYN_N];
    memset(dyn, 0, sizeof dyn);
    const bool zero = (c.zflags & Z_ALL) != 0;          // a fresh object whose zeroing waits for the channel's next block
    if (!zero) KG_HIP(hipMemcpyAsync(dyn, d->dyn, sizeof dyn, hipMemcpyDeviceToHost, s));
    if (iq) {
        if (zero) memset(iq, 0, sizeof d->iq);
        else KG_HIP(hipMemcpyAsync(iq, d->iq, sizeof d->iq, hipMemcpyDeviceToHost, s));
    }
    if (plot) {
        if (zero) memset(plot, 0, sizeof d->plot);
        else KG_HIP(hipMemcpyAsync(plot, d->plot, sizeof d->plot, hipMemcpyDeviceToHost, s));
    }
    if (map) {
        if (zero) memset(map, 0, sizeof d->map);
        else KG_HIP(hipMemcpyAsync(map, d->map, sizeof d->map, hipMemcpyDeviceToHost, s));
    }
    KG_HIP(hipStreamSynchronize(s));
    if (c.zflags & Z_MA) dyn[DYN_CMA_RE] = dyn[DYN_CMA_IM] = dyn[DYN_AMA] = 0;
    if (c.zflags & Z_PLL) memset(dyn + DYN_PLL, 0, sizeof(float) * 9);
    if (info) {
        const state_t &e = c.st;
        memset(info, 0, sizeof *info);
        info->inited = e.inited; info->run = e.run; info->points = e.points; info->nsamp = e.nsamp; info->exponent = e.exponent;
        info->msk_mode = e.msk_mode; info->msk_baud = e.msk_baud; info->draw = e.draw; info->display_mode = e.display_mode; info->maN = e.maN;
        info->maNsend = e.maNsend; info->ring[0] = e.ring[0]; info->ring[1] = e.ring[1];
        info->gain = e.gain; info->fs = e.fs; info->pll_bandwidth = e.pll_bandwidth;
        info->cmaI = dyn[DYN_CMA_RE]; info->cmaQ = dyn[DYN_CMA_IM]; info->ama = dyn[DYN_AMA];
        for (int w = 0; w < 3; w++) {
            float *o = info->pll[w];
            o[0] = e.pll[w].fs; o[1] = e.pll[w].fc; o[2] = dyn[DYN_PLL + 3 * w]; o[3] = dyn[DYN_PLL + 3 * w + 1]; o[4] = e.pll[w].b0; o[5] = e.pll[w].b1;
            o[6] = dyn[DYN_PLL + 3 * w + 2];
        }
    }
    return KG_OK;
}

int kg_iqd_math_dev(kg_ctx *ctx, int fn, const float *d_a, const float *d_b, size_t n, float *d_out)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(d_a && d_b && d_out && n >= 1 && KG_ALIGNED(d_a, 4) && KG_ALIGNED(d_b, 4) && KG_ALIGNED(d_out, 4), KG_ERR_INVALID, "kg_iqd_math_dev: bad argument");
    KG_REQUIRE(fn == KG_IQD_MATH_HYPOTF || fn == KG_IQD_MATH_FMODF, KG_ERR_INVALID, "kg_iqd_math_dev: unknown function %d", fn);
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(iqd_math_kernel, dim3((unsigned) (blocks < 16384 ? blocks : 16384)), dim3(256), 0, ctx->stream, fn, d_a, d_b, n, d_out);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

}  // extern "C"
