// kg_ft8.hip -- the FT8 / FT4 extension, stage 1 (extensions/FT8/, ft8_lib; csrc/kg_ft8.h is the one definition of its arithmetic and
// schedule).
//
// The schedule of decode_ft8_samples (decode_ft8.c:503-559) depends on no sample, so the host walks a push callback by callback
// (sched_callback of kg_ft8.h) and hands the kernels ONE table: the copy runs, the (block, time_sub) transforms due, the slots that end.
// A connection keeps, per slot parity, (previous tail || this slot's samples) as floats and the waterfall bytes; a slot that ends leaves
// its tail -- last_frame, which survives monitor_reset -- at the head of the other parity's samples, where the next slot finds it.  So
// every analysis frame is nfft consecutive floats of one buffer, and every transform of a push is independent of the others.
//   copy     a workgroup per run: int16 / 32768.0f (:533);
//   tail     a workgroup per ending slot: its last nfft samples to the other parity;
//   monitor  a workgroup per (connection, block, time_sub): the windowed frame is staged in LDS as nfft / 2 complex values (even, odd),
//            a half-length Stockham transform runs through two LDS tiles -- passes of radix 4, 2, 3 and 5 (1920 = 4 4 4 2 3 5,
//            576 = 4 4 4 3 3), the twiddles read from an exact table of W_nfft made on the host in double --, then the split to the real
//            transform for the freq_osr * num_bins kept bins ALONE, the chain mag2 -> dB -> byte of monitor.c:180-192, and the maximum
//            of db over the workgroup (a float maximum is order-free: max_mag is exact given equal db);
// and behind the monitor launch of a push that ends a slot, with no host read between them:
//   score    a workgroup per (slot, time_sub, freq_sub, time_offset): the 21 (16) rows of Costas blocks it touches go to LDS, a lane a
//            freq_offset (decode.c:63-190);
//   select   a workgroup per slot: the hypotheses with score >= min_score are compacted in scan order by a prefix sum, then ONE lane
//            runs the twin's heap (heap_of_list: ftx_find_candidates' loop body and heap sort, :214-251) and writes the candidates;
//   like     a workgroup per candidate, a lane per data symbol; lane 0 forms sum and sum2 in index order (:312-318: no tree).
#include "kg_ext.h"
#include "kg_fft.h"
#include "kg_ft8.h"

using namespace kg_ft8_cf;

static_assert(sizeof(kg_ft8_ev) == 32 && sizeof(kg_ft8_cand) == 20 && sizeof(kg_ft8_slot) == 32 + 20 * 140 + 4 * 140 * 174 && sizeof(kg_ft8_info) == 88, "kg_ft8_* layout");
static_assert(KG_FT8_MAX_CAND == MAX_CAND && KG_FT8_MIN_SCORE == MIN_SCORE && KG_FT8_LDPC_N == LDPC_N && KG_FT8_MAX_NS == MAX_NS && KG_FT8_MAX_NFFT == MAX_NFFT &&
              KG_FT8_PROTO_FT8 == PROTO_FT8 && KG_FT8_PROTO_FT4 == PROTO_FT4 && KG_FT8_EV_SLOT_START == EV_SLOT_START && KG_FT8_EV_DECODE == EV_DECODE, "constants");
static_assert(sizeof(cand_t) == 8, "ftx_candidate_t");

enum { F8_THREADS = 256, F8_MAX_CONNS = 64, F8_MAX_CB = 4096, F8_MAX_PASS = 8, F8_LIKE_THREADS = 128, F8_COPY_CHUNK = 2048, F8_COPY_MAX_Y = 32 };
enum { F8_SLOT_SAMPLES = 92 * 1920 + MAX_NS, F8_SAMP = MAX_NFFT + F8_SLOT_SAMPLES };      // floats of one parity: tail, slot, the last callback's surplus
enum { F8_WF = KG_FT8_MAX_WF + 12, F8_NWF = 3, F8_WG = 2 * MAX_BLOCKS, F8_NHYP = 4 * NTO * 474 };        // F8_NWF: two parities and the load path's own
static_assert(F8_WF % 16 == 0 && F8_NHYP < 65536, "shapes");

struct f8_cfgs { cfg_t c[2]; int32_t npass[2], radix[2][F8_MAX_PASS]; };
struct f8_copy { int32_t conn, parity, dst, n; int64_t src; };
struct f8_tail { int32_t conn, parity, src, n; };
struct f8_blk { int32_t conn, parity, block, time_sub, protocol, start, pad[2]; };
struct f8_end { int32_t conn, which, num_blocks, protocol, num_candidates, min_score, out, slot, have_max, pad[3]; };
static_assert(sizeof(f8_copy) == 24 && sizeof(f8_tail) == 16 && sizeof(f8_blk) == 32 && sizeof(f8_end) == 48, "table layout");

__device__ __constant__ const unsigned char f8_costas8[7] = KG_FT8_COSTAS;
__device__ __constant__ const unsigned char f8_costas4[4][4] = KG_FT4_COSTAS;
__device__ __constant__ const unsigned char f8_gray8[8] = KG_FT8_GRAY;
__device__ __constant__ const unsigned char f8_gray4[4] = KG_FT4_GRAY;

__global__ __launch_bounds__(F8_THREADS) void ft8_copy_kernel(const f8_copy *__restrict__ tab, const int16_t *__restrict__ in, float *samp)
{
    const f8_copy e = tab[blockIdx.x];
    float *dst = samp + ((size_t) e.conn * 2 + e.parity) * F8_SAMP + MAX_NFFT + e.dst;
    // grid.y workgroups share a run: chunk after chunk of F8_COPY_CHUNK samples, so that a push that carries a whole slot is not one workgroup's
    for (int c0 = (int) blockIdx.y * F8_COPY_CHUNK; c0 < e.n; c0 += (int) gridDim.y * F8_COPY_CHUNK) {
        const int c1 = c0 + F8_COPY_CHUNK < e.n ? c0 + F8_COPY_CHUNK : e.n;
        for (int t = c0 + (int) threadIdx.x; t < c1; t += F8_THREADS) dst[t] = sample_of(in[e.src + t]);
    }
}

__global__ __launch_bounds__(F8_THREADS) void ft8_tail_kernel(const f8_tail *__restrict__ tab, float *samp)
{
    const f8_tail e = tab[blockIdx.x];
    const float *src = samp + ((size_t) e.conn * 2 + e.parity) * F8_SAMP + e.src;           // e.src: in buffer coordinates, the slot's samples begin at MAX_NFFT
    float *dst = samp + ((size_t) e.conn * 2 + (e.parity ^ 1)) * F8_SAMP + (MAX_NFFT - e.n);
    for (int t = (int) threadIdx.x; t < e.n; t += F8_THREADS) dst[t] = src[t];
}

// forward butterflies (exp(-i ...)); kg_addj / kg_subj are kg_fft.h's a + jb, a - jb
KG_DEV void f8_dft2(cf *v) { const cf a = v[0], b = v[1]; v[0] = a + b; v[1] = a - b; }
KG_DEV void f8_dft3(cf *v)
{
    const cf t = v[1] + v[2], m = v[0] - kg_scale(t, 0.5f), s = kg_scale(v[1] - v[2], 0.86602540378443864676f);
    v[0] = v[0] + t; v[1] = kg_subj(m, s); v[2] = kg_addj(m, s);
}
KG_DEV void f8_dft4(cf *v)
{
    const cf a = v[0] + v[2], b = v[0] - v[2], c = v[1] + v[3], d = v[1] - v[3];
    v[0] = a + c; v[1] = kg_subj(b, d); v[2] = a - c; v[3] = kg_addj(b, d);
}
KG_DEV void f8_dft5(cf *v)
{
    const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f, s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
    const cf a1 = v[1] + v[4], a2 = v[2] + v[3], b1 = v[1] - v[4], b2 = v[2] - v[3];
    const cf p = v[0] + kg_scale(a1, c1) + kg_scale(a2, c2), q = v[0] + kg_scale(a1, c2) + kg_scale(a2, c1);
    const cf u = kg_scale(b1, s1) + kg_scale(b2, s2), w = kg_scale(b1, s2) - kg_scale(b2, s1);
    v[0] = v[0] + a1 + a2; v[1] = kg_subj(p, u); v[4] = kg_addj(p, u); v[2] = kg_subj(q, w); v[3] = kg_addj(q, w);
}
// one Stockham pass of radix R over n points whose earlier passes' radices multiply to ns; tw: W_(2n)^k, k < 2n
template <int R> KG_DEV void f8_pass(const float2 *src, float2 *dst, const float2 *__restrict__ tw, int n, int ns, int tid)
{
    const int m = n / R, step = 2 * (n / (ns * R));
    for (int j = tid; j < m; j += F8_THREADS) {
        const int k = j % ns;
        cf v[R];
        v[0] = kg_ld(&src[j]);
#pragma unroll
        for (int r = 1; r < R; r++) v[r] = kg_cmul(kg_ld(&src[j + r * m]), kg_ld(&tw[r * k * step]));
        if (R == 2) f8_dft2(v); else if (R == 3) f8_dft3(v); else if (R == 4) f8_dft4(v); else f8_dft5(v);
        const int j0 = (j / ns) * ns * R + k;
#pragma unroll
        for (int r = 0; r < R; r++) kg_st(&dst[j0 + r * ns], v[r]);
    }
}

__global__ __launch_bounds__(F8_THREADS) void ft8_monitor_kernel(const f8_blk *__restrict__ tab, const f8_cfgs cf2, const float *__restrict__ samp, const float *__restrict__ window,
                                                                 const float2 *__restrict__ twid, uint8_t *wf, float *wgmax)
{
    __shared__ float2 s_a[MAX_NFFT / 2], s_b[MAX_NFFT / 2];
    __shared__ float s_max[F8_THREADS];
    const f8_blk e = tab[blockIdx.x];
    const cfg_t &c = cf2.c[e.protocol];
    const int tid = (int) threadIdx.x, n = c.nfft / 2;
    const float *x = samp + ((size_t) e.conn * 2 + e.parity) * F8_SAMP + (MAX_NFFT - c.nfft) + e.start;     // e.start: the frame's start counted from the tail's first sample
    const float *win = window + e.protocol * MAX_NFFT;
    const float2 *tw = twid + e.protocol * MAX_NFFT;
    for (int t = tid; t < n; t += F8_THREADS) kg_st(&s_a[t], cf{windowed(win[2 * t], x[2 * t]), windowed(win[2 * t + 1], x[2 * t + 1])});      // monitor.c:168-171
    __syncthreads();
    float2 *src = s_a, *dst = s_b;
    int ns = 1;
    for (int p = 0; p < cf2.npass[e.protocol]; p++) {
        const int r = cf2.radix[e.protocol][p];
        if (r == 4) f8_pass<4>(src, dst, tw, n, ns, tid);
        else if (r == 2) f8_pass<2>(src, dst, tw, n, ns, tid);
        else if (r == 3) f8_pass<3>(src, dst, tw, n, ns, tid);
        else f8_pass<5>(src, dst, tw, n, ns, tid);
        ns *= r;
        __syncthreads();
        float2 *sw = src; src = dst; dst = sw;
    }
    // the split: X[k] = (Z[k] + conj Z[n-k]) / 2 - j W^k (Z[k] - conj Z[n-k]) / 2, for the kept bins alone (monitor.c:175-199)
    uint8_t *out = wf + ((size_t) e.conn * F8_NWF + e.parity) * F8_WF + (size_t) (e.block * TIME_OSR + e.time_sub) * FREQ_OSR * c.num_bins;
    float mx = -INFINITY;
    for (int idx = tid; idx < FREQ_OSR * c.num_bins; idx += F8_THREADS) {
        const int freq_sub = idx / c.num_bins, bin = idx - freq_sub * c.num_bins;
        const int k = src_bin_of(c.min_bin, bin, freq_sub);             // 0 < k < n for every kept bin (checked at create)
        const cf a = kg_ld(&src[k]), zb = kg_ld(&src[n - k]);
        const cf b = cf{zb.x, -zb.y};
        const cf ev = kg_scale(a + b, 0.5f), od = kg_scale(a - b, 0.5f);
        const cf wo = kg_cmul(od, kg_ld(&tw[k]));
        const cf X = kg_subj(ev, wo);
        const float db = db_of(X.x, X.y);
        out[idx] = byte_of(db);
        mx = db > mx ? db : mx;
    }
    s_max[tid] = mx;
    __syncthreads();
    for (int m = F8_THREADS / 2; m >= 1; m >>= 1) {
        if (tid < m) s_max[tid] = s_max[tid + m] > s_max[tid] ? s_max[tid + m] : s_max[tid];
        __syncthreads();
    }
    if (tid == 0) wgmax[((size_t) e.conn * 2 + e.parity) * F8_WG + e.block * TIME_OSR + e.time_sub] = s_max[0];
}

__global__ __launch_bounds__(F8_THREADS) void ft8_score_kernel(const f8_end *__restrict__ tab, const f8_cfgs cf2, const uint8_t *__restrict__ wf, int16_t *scores)
{
    __shared__ unsigned char s_rows[MAX_SYNC_ROWS][MAX_BINS + 3];
    const f8_end e = tab[blockIdx.y];
    const cfg_t &c = cf2.c[e.protocol];
    const int tid = (int) threadIdx.x;
    const int g = (int) blockIdx.x, to_i = g % NTO, freq_sub = (g / NTO) % FREQ_OSR, time_sub = g / (NTO * FREQ_OSR);
    const int time_offset = TO_MIN + to_i;
    const int ft4 = e.protocol == PROTO_FT4, LEN = ft4 ? (int) FT4_LENGTH_SYNC : (int) FT8_LENGTH_SYNC, NUM = ft4 ? (int) FT4_NUM_SYNC : (int) FT8_NUM_SYNC;
    const uint8_t *mag = wf + ((size_t) e.conn * F8_NWF + e.which) * F8_WF;
    for (int r = 0; r < NUM * LEN; r++) {
        const int block_abs = time_offset + sync_block(e.protocol, r / LEN, r % LEN);
        const bool in = block_abs >= 0 && block_abs < e.num_blocks;
        for (int b = tid; b < c.num_bins; b += F8_THREADS) s_rows[r][b] = in ? mag[mag_index(c, block_abs, time_sub, freq_sub, b)] : (unsigned char) 0;
    }
    __syncthreads();
    const int nfo = num_freq_offsets(c);
    const unsigned char *costas = ft4 ? &f8_costas4[0][0] : f8_costas8;
    for (int fo = tid; fo < nfo; fo += F8_THREADS) {
        const int score = sync_score(e.protocol, time_offset, e.num_blocks, costas, [&](int m, int k, int f) { return s_rows[m * LEN + k][fo + f]; });
        scores[(size_t) e.conn * F8_NHYP + (size_t) g * nfo + fo] = (int16_t) score;        // g * nfo + fo: the hypothesis in scan order (hyp_of)
    }
}

__global__ __launch_bounds__(F8_THREADS) void ft8_select_kernel(const f8_end *__restrict__ tab, const f8_cfgs cf2, const int16_t *__restrict__ scores, uint32_t *lists,
                                                                const float *__restrict__ wgmax, kg_ft8_slot *slots, float snr_adj)
{
    __shared__ int s_cnt[F8_THREADS + 1];
    __shared__ cand_t s_heap[MAX_CAND];
    __shared__ float s_max[F8_THREADS];
    const f8_end e = tab[blockIdx.x];
    const cfg_t &c = cf2.c[e.protocol];
    const int tid = (int) threadIdx.x, nh = num_hyp(c);
    const int16_t *sc = scores + (size_t) e.conn * F8_NHYP;
    uint32_t *list = lists + (size_t) e.conn * F8_NHYP;
    const int per = (nh + F8_THREADS - 1) / F8_THREADS, h0 = tid * per, h1 = h0 + per < nh ? h0 + per : nh;
    int cnt = 0;
    for (int h = h0; h < h1; h++) cnt += sc[h] >= e.min_score;
    s_cnt[tid + 1] = cnt;
    if (tid == 0) s_cnt[0] = 0;
    __syncthreads();
    if (tid == 0) for (int t = 1; t <= F8_THREADS; t++) s_cnt[t] += s_cnt[t - 1];          // 256 additions: the prefix sum over the grid
    __syncthreads();
    int at = s_cnt[tid];
    for (int h = h0; h < h1; h++)
        if (sc[h] >= e.min_score) list[at++] = pass_entry(h, sc[h]);
    float mx = -120.0f;                                                 // monitor.c:112, :137, :196-197
    if (e.have_max)
        for (int t = tid; t < e.num_blocks * TIME_OSR; t += F8_THREADS) {
            const float v = wgmax[((size_t) e.conn * 2 + e.which) * F8_WG + t];
            mx = v > mx ? v : mx;
        }
    s_max[tid] = mx;
    __syncthreads();                                                    // the list is this workgroup's own: visible to lane 0 behind the barrier
    for (int m = F8_THREADS / 2; m >= 1; m >>= 1) {
        if (tid < m) s_max[tid] = s_max[tid + m] > s_max[tid] ? s_max[tid + m] : s_max[tid];
        __syncthreads();
    }
    if (tid != 0) return;
    kg_ft8_slot *o = slots + e.out;
    const int ncand = heap_of_list(c, list, s_cnt[F8_THREADS], e.num_candidates, s_heap);
    o->conn = e.conn; o->due = 1; o->ncand = ncand; o->num_blocks = e.num_blocks; o->protocol = e.protocol; o->slot = e.slot; o->max_mag = s_max[0]; o->pad = 0;
    for (int i = 0; i < ncand; i++) {
        const cand_t x = s_heap[i];
        kg_ft8_cand r = {x.score, x.time_offset, x.freq_offset, x.time_sub, x.freq_sub, freq_hz_of(c, x), time_sec_of(c, x), snr_of(x, snr_adj)};
        o->cand[i] = r;
    }
}

__global__ __launch_bounds__(F8_LIKE_THREADS) void ft8_like_kernel(const f8_end *__restrict__ tab, const f8_cfgs cf2, const uint8_t *__restrict__ wf, kg_ft8_slot *slots)
{
    __shared__ float s_log[LDPC_N + 2];
    __shared__ float s_nf;
    const f8_end e = tab[blockIdx.y];
    kg_ft8_slot *o = slots + e.out;
    const int ci = (int) blockIdx.x, tid = (int) threadIdx.x;
    if (ci >= o->ncand) return;                                         // the whole workgroup
    const cfg_t &c = cf2.c[e.protocol];
    const kg_ft8_cand x = o->cand[ci];
    const uint8_t *mag = wf + ((size_t) e.conn * F8_NWF + e.which) * F8_WF;
    const int per = e.protocol == PROTO_FT4 ? 2 : 3;
    if (tid < num_data_syms(e.protocol)) {
        const int block = x.time_offset + sym_idx_of(e.protocol, tid);
        float *logl = s_log + per * tid;
        if ((block < 0) || (block >= e.num_blocks)) { for (int j = 0; j < per; j++) logl[j] = 0; }
        else extract_symbol(e.protocol, e.protocol == PROTO_FT4 ? f8_gray4 : f8_gray8, [&](int f) { return mag[mag_index(c, block, x.time_sub, x.freq_sub, x.freq_offset + f)]; }, logl);
    }
    __syncthreads();
    if (tid == 0) s_nf = norm_factor_of(s_log);
    __syncthreads();
    for (int i = tid; i < LDPC_N; i += F8_LIKE_THREADS) o->log174[ci][i] = s_log[i] * s_nf;
}

struct f8_conn { state_t st; int32_t last_blocks = 0; };

struct kg_ft8 {
    kg_ctx *ctx;
    int nconn;
    float snr_adj;
    f8_cfgs cfgs;
    std::vector<f8_conn> c;
    kg_dbuf<float> d_samp;                      // [nconn][2][F8_SAMP]
    kg_dbuf<uint8_t> d_wf;                      // [nconn][3][F8_WF]
    kg_dbuf<float> d_wgmax;                     // [nconn][2][F8_WG]
    kg_dbuf<int16_t> d_scores;                  // [nconn][F8_NHYP]
    kg_dbuf<uint32_t> d_lists;                  // [nconn][F8_NHYP]
    kg_dbuf<float> d_window;                    // [2][MAX_NFFT], monitor.c:66-74
    kg_dbuf<float2> d_twid;                     // [2][MAX_NFFT]: exp(-2 pi i k / nfft), rounded from double
};

struct f8_plan {
    std::vector<int> conn;                      // the connections of the list, in list order
    std::vector<state_t> st;                    // their states behind the push
    std::vector<int32_t> last_blocks;
    std::vector<f8_copy> copies;
    std::vector<f8_tail> tails;
    std::vector<f8_blk> blks;
    std::vector<f8_end> ends;
    std::vector<kg_ft8_ev> evs;
};

static int f8_walk(kg_ft8 *q, const int32_t *conns, int nconn, const int32_t *ncb, const int64_t *in_off, int ns, size_t sample_stride, const double *times, size_t time_stride, int max_events,
                   int max_slots, f8_plan &p, const char *who)
{
    KG_REQUIRE(nconn >= 1 && nconn <= q->nconn, KG_ERR_INVALID, "%s: nconn %d (1..%d)", who, nconn, q->nconn);
    KG_REQUIRE(ns >= 1 && ns <= MAX_NS, KG_ERR_INVALID, "%s: ns %d (1..%d)", who, ns, (int) MAX_NS);
    KG_REQUIRE(max_events >= 0 && max_slots >= 0, KG_ERR_INVALID, "%s: max_events %d, max_slots %d", who, max_events, max_slots);
    std::vector<char> listed((size_t) q->nconn, 0);
    for (int i = 0; i < nconn; i++) {
        const int c = conns[i];
        KG_TRY(kg_ext_list_entry(who, listed, nconn, i, c, ncb[i], F8_MAX_CB, "sample_stride", sample_stride, (size_t) ns, in_off != nullptr, "sample offset", in_off ? (long long) in_off[i] : 0));
        KG_REQUIRE(ncb[i] <= 0 || nconn == 1 || time_stride >= (size_t) ncb[i], KG_ERR_INVALID, "%s: time_stride %zu below the %d callbacks of entry %d", who, time_stride,
                   ncb[i], i);
        KG_REQUIRE(q->c[c].st.inited, KG_ERR_STATE, "%s: connection %d was never initialised (kg_ft8_init)", who, c);
        for (int b = 0; b < ncb[i]; b++)
            KG_REQUIRE(time_ok(times[i * time_stride + b]), KG_ERR_INVALID, "%s: callback %d of entry %d at time %g (finite, 0 .. 2^40)", who, b, i, times[i * time_stride + b]);
        state_t st = q->c[c].st;
        int32_t last_blocks = q->c[c].last_blocks;
        const cfg_t &cf = st.cfg;
        sched_t sp;
        for (int b = 0; b < ncb[i]; b++) sched_callback(st, sp, b, (in_off ? in_off[i] : (int64_t) i * (int64_t) sample_stride) + (int64_t) b * ns, ns, times[i * time_stride + b]);
        KG_REQUIRE(sp.nend <= 1, KG_ERR_INVALID, "%s: entry %d ends %d slots; a push takes at most one (cut it)", who, i, sp.nend);
        for (const op_t &o : sp.ops) {
            if (o.kind == OP_COPY) {
                KG_REQUIRE(o.a + o.n <= F8_SLOT_SAMPLES, KG_ERR_STATE, "%s: entry %d: sample %d of a slot", who, i, o.a + o.n);       // cannot happen: ns <= MAX_NS
                if (!p.copies.empty() && p.copies.back().conn == c && p.copies.back().parity == o.parity && p.copies.back().dst + p.copies.back().n == o.a &&
                    p.copies.back().src + p.copies.back().n == o.src)
                    p.copies.back().n += o.n;
                else p.copies.push_back(f8_copy{c, o.parity, o.a, o.n, o.src});
            } else if (o.kind == OP_BLOCK) {
                for (int t = 0; t < TIME_OSR; t++) p.blks.push_back(f8_blk{c, o.parity, o.a, t, st.protocol, frame_start(cf, (int) o.src, t) + cf.nfft, {0, 0}});
            } else {
                KG_REQUIRE(p.ends.size() < (size_t) max_slots, KG_ERR_INVALID, "%s: more ended slots than max_slots = %d", who, max_slots);
                p.tails.push_back(f8_tail{c, o.parity, MAX_NFFT + o.a * cf.block_size - cf.nfft, cf.nfft});
                p.ends.push_back(f8_end{c, o.parity, o.a, st.protocol, MAX_CAND, MIN_SCORE, (int32_t) p.ends.size(), o.n, 1, {0, 0, 0}});
                last_blocks = o.a;
            }
        }
        for (const ev_t &m : sp.evs) p.evs.push_back(kg_ft8_ev{c, m.cb, m.kind, m.a, m.b, 0, m.t});
        KG_REQUIRE(p.evs.size() <= (size_t) max_events, KG_ERR_INVALID, "%s: more events than max_events = %d", who, max_events);
        p.conn.push_back(c);
        p.st.push_back(st);
        p.last_blocks.push_back(last_blocks);
    }
    return KG_OK;
}

// the slot-end chain of `ne` entries of a staged table, behind whatever the stream holds; d_slots cleared here.  Enqueue only.
static int f8_chain(kg_ft8 *q, const f8_end *d_ends, int ne, kg_ft8_slot *d_slots)
{
    hipStream_t s = q->ctx->stream;
    KG_HIP(hipMemsetAsync(d_slots, 0, sizeof(kg_ft8_slot) * (size_t) ne, s));
    hipLaunchKernelGGL(ft8_score_kernel, dim3(TIME_OSR * FREQ_OSR * NTO, (unsigned) ne), dim3(F8_THREADS), 0, s, d_ends, q->cfgs, (const uint8_t *) q->d_wf.p, q->d_scores.p);
    KG_HIP(hipGetLastError());
    hipLaunchKernelGGL(ft8_select_kernel, dim3((unsigned) ne), dim3(F8_THREADS), 0, s, d_ends, q->cfgs, (const int16_t *) q->d_scores.p, q->d_lists.p,
                       (const float *) q->d_wgmax.p, d_slots, q->snr_adj);
    KG_HIP(hipGetLastError());
    hipLaunchKernelGGL(ft8_like_kernel, dim3(MAX_CAND, (unsigned) ne), dim3(F8_LIKE_THREADS), 0, s, d_ends, q->cfgs, (const uint8_t *) q->d_wf.p, d_slots);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

// A walked push enqueued on device memory, samples and slot records alike: ONE table -- copies, tails, blocks, ends -- staged ahead of the
// first launch.  The commit is the last act.  Enqueue only.
static int f8_enqueue(kg_ft8 *q, f8_plan &p, const int16_t *d_in, kg_ft8_slot *d_slots)
{
    hipStream_t s = q->ctx->stream;
    const size_t nc = sizeof(f8_copy) * p.copies.size(), nt = sizeof(f8_tail) * p.tails.size(), nb = sizeof(f8_blk) * p.blks.size(), ne = sizeof(f8_end) * p.ends.size();
    if (nc + nt + nb + ne) {
        std::vector<unsigned char> tab(nc + nt + nb + ne);
        if (nc) memcpy(tab.data(), p.copies.data(), nc);
        if (nt) memcpy(tab.data() + nc, p.tails.data(), nt);
        if (nb) memcpy(tab.data() + nc + nt, p.blks.data(), nb);
        if (ne) memcpy(tab.data() + nc + nt + nb, p.ends.data(), ne);
        void *d_tab = nullptr;
        KG_TRY(kg_ctx_stage(q->ctx, tab.data(), tab.size(), &d_tab));
        KG_PLAN_ONLY(q->ctx);
        const unsigned char *t = (const unsigned char *) d_tab;
        if (nc) {
            int longest = 0;
            for (const f8_copy &c : p.copies) longest = c.n > longest ? c.n : longest;
            const int ny = (longest + F8_COPY_CHUNK - 1) / F8_COPY_CHUNK;
            hipLaunchKernelGGL(ft8_copy_kernel, dim3((unsigned) p.copies.size(), (unsigned) (ny < 1 ? 1 : ny > F8_COPY_MAX_Y ? F8_COPY_MAX_Y : ny)), dim3(F8_THREADS), 0, s,
                               (const f8_copy *) t, d_in, q->d_samp.p);
            KG_HIP(hipGetLastError());
        }
        if (nt) {
            hipLaunchKernelGGL(ft8_tail_kernel, dim3((unsigned) p.tails.size()), dim3(F8_THREADS), 0, s, (const f8_tail *) (t + nc), q->d_samp.p);
            KG_HIP(hipGetLastError());
        }
        if (nb) {
            hipLaunchKernelGGL(ft8_monitor_kernel, dim3((unsigned) p.blks.size()), dim3(F8_THREADS), 0, s, (const f8_blk *) (t + nc + nt), q->cfgs, (const float *) q->d_samp.p,
                               (const float *) q->d_window.p, (const float2 *) q->d_twid.p, q->d_wf.p, q->d_wgmax.p);
            KG_HIP(hipGetLastError());
        }
        if (ne) KG_TRY(f8_chain(q, (const f8_end *) (t + nc + nt + nb), (int) p.ends.size(), d_slots));
    }
    for (size_t k = 0; k < p.conn.size(); k++) { q->c[p.conn[k]].st = p.st[k]; q->c[p.conn[k]].last_blocks = p.last_blocks[k]; }     // commit: the enqueue succeeded
    return KG_OK;
}

// kg_ft8_push on device memory, for kg_rxbank.hip: entry i's samples at d_in + in_off[i] (null: i * sample_stride), the slot records on
// the device too, slot k the k-th entry that ends one; slot_conn[k] names its connection.  Events are the host's schedule.  Enqueue only.
int kg_ft8_push_at_(kg_ft8 *q, const int32_t *conns, int nconn, const int32_t *ncb, const int64_t *in_off, int ns, const int16_t *d_in, size_t sample_stride,
                    const double *times, size_t time_stride, kg_ft8_ev *evs, int max_events, int32_t *nevents, kg_ft8_slot *d_slots, int max_slots, int32_t *slot_conn,
                    int32_t *nslots)
{
    KG_REQUIRE(q && conns && ncb && d_in && times && evs && nevents && d_slots && slot_conn && nslots, KG_ERR_INVALID, "kg_ft8_push: null argument");
    KG_TRY(kg_ctx_use(q->ctx));
    KG_REQUIRE(KG_ALIGNED(d_in, 2) && KG_ALIGNED(d_slots, 4), KG_ERR_INVALID, "kg_ft8_push: the samples must be 2-byte aligned, the slot records 4-byte aligned");
    f8_plan p;
    KG_TRY(f8_walk(q, conns, nconn, ncb, in_off, ns, sample_stride, times, time_stride, max_events, max_slots, p, "kg_ft8_push"));
    for (size_t k = 0; k < p.ends.size(); k++) slot_conn[k] = p.ends[k].conn;
    if (!p.evs.empty()) memcpy(evs, p.evs.data(), sizeof(kg_ft8_ev) * p.evs.size());
    *nevents = (int32_t) p.evs.size();
    *nslots = (int32_t) p.ends.size();
    return f8_enqueue(q, p, d_in, d_slots);
}

// what the table of a push over nconn connections of at most ncb callbacks each takes (and its alignment): a copy run a callback, two
// transforms a block -- a callback of 512 samples completes two FT4 blocks at most --, one tail and one slot end a connection
size_t kg_ft8_table_bytes_(size_t nconn, size_t ncb)
{
    return 64 + nconn * (sizeof(f8_copy) * (ncb + 1) + sizeof(f8_tail) + sizeof(f8_blk) * TIME_OSR * (2 * ncb + 2) + sizeof(f8_end));
}

int kg_ft8_inited_(const kg_ft8 *q, int conn) { return q->c[conn].st.inited; }

// connection conn as a new connection finds it: not initialised, last_frame zeroed.  Enqueue only.
int kg_ft8_reset_(kg_ft8 *q, int conn)
{
    KG_REQUIRE(q != nullptr && conn >= 0 && conn < q->nconn, KG_ERR_INVALID, "kg_ft8: connection %d", conn);
    KG_TRY(kg_ctx_use(q->ctx));
    KG_HIP(hipMemsetAsync(q->d_samp.p + (size_t) conn * 2 * F8_SAMP, 0, sizeof(float) * MAX_NFFT, q->ctx->stream));
    memset(&q->c[conn].st, 0, sizeof q->c[conn].st);
    q->c[conn].last_blocks = 0;
    return KG_OK;
}

extern "C" {

int kg_ft8_create(kg_ctx *ctx, int nconn, kg_ft8 **out)
{
    return kg_ext_create(ctx, nconn, F8_MAX_CONNS, "kg_ft8_create", "nconn", out, [=](kg_ft8 *q) -> int {
        q->nconn = nconn;
        q->snr_adj = -22.0f;                                            // FT8.cpp:312
        q->c.resize(nconn);
        for (f8_conn &c : q->c) memset(&c.st, 0, sizeof c.st);
        KG_TRY(q->d_samp.alloc((size_t) nconn * 2 * F8_SAMP, "kg_ft8_create: samples"));
        KG_TRY(q->d_wf.alloc((size_t) nconn * F8_NWF * F8_WF, "kg_ft8_create: waterfalls"));
        KG_TRY(q->d_wgmax.alloc((size_t) nconn * 2 * F8_WG, "kg_ft8_create: maxima"));
        KG_TRY(q->d_scores.alloc((size_t) nconn * F8_NHYP, "kg_ft8_create: scores"));
        KG_TRY(q->d_lists.alloc((size_t) nconn * F8_NHYP, "kg_ft8_create: lists"));
        KG_TRY(q->d_window.alloc((size_t) 2 * MAX_NFFT, "kg_ft8_create: windows"));
        KG_TRY(q->d_twid.alloc((size_t) 2 * MAX_NFFT, "kg_ft8_create: twiddles"));
        std::vector<float> win((size_t) 2 * MAX_NFFT, 0.0f);
        std::vector<float2> tw((size_t) 2 * MAX_NFFT, float2{0.0f, 0.0f});
        memset(&q->cfgs, 0, sizeof q->cfgs);
        for (int pr = 0; pr < 2; pr++) {
            const cfg_t c = cfg_of(pr, 12000);
            q->cfgs.c[pr] = c;
            KG_REQUIRE(c.nfft <= MAX_NFFT && c.num_bins <= MAX_BINS && c.max_blocks <= MAX_BLOCKS && c.slot_blocks <= c.max_blocks &&
                           c.slot_blocks * c.block_size + MAX_NS <= F8_SLOT_SAMPLES && c.max_blocks * c.block_stride <= KG_FT8_MAX_WF && num_hyp(c) <= F8_NHYP &&
                           c.min_bin * FREQ_OSR > 0 && c.max_bin * FREQ_OSR < c.nfft / 2,
                       KG_ERR_STATE, "kg_ft8_create: the sizes of protocol %d", pr);
            int n = c.nfft / 2, np = 0;
            for (int r : {4, 2, 3, 5})
                while (n % r == 0 && np < F8_MAX_PASS) { q->cfgs.radix[pr][np++] = r; n /= r; }
            KG_REQUIRE(n == 1, KG_ERR_STATE, "kg_ft8_create: nfft %d is not 2^a 3^b 5^c in %d passes", c.nfft, (int) F8_MAX_PASS);
            q->cfgs.npass[pr] = np;
            for (int i = 0; i < c.nfft; i++) {
                win[(size_t) pr * MAX_NFFT + i] = window_at(c, i);
                const double a = -2.0 * M_PI * (double) i / (double) c.nfft;
                tw[(size_t) pr * MAX_NFFT + i] = float2{(float) cos(a), (float) sin(a)};
            }
        }
        KG_HIP(hipMemcpyAsync(q->d_window.p, win.data(), sizeof(float) * win.size(), hipMemcpyHostToDevice, ctx->stream));
        KG_HIP(hipMemcpyAsync(q->d_twid.p, tw.data(), sizeof(float2) * tw.size(), hipMemcpyHostToDevice, ctx->stream));
        KG_HIP(hipStreamSynchronize(ctx->stream));                      // win and tw are this frame's
        KG_TRY(kg_ext_zero(ctx, q->d_wf.p, (size_t) nconn * F8_NWF * F8_WF, "kg_ft8_create"));
        KG_TRY(kg_ext_zero(ctx, q->d_wgmax.p, (size_t) nconn * 2 * F8_WG, "kg_ft8_create"));
        KG_TRY(kg_ext_zero(ctx, q->d_scores.p, (size_t) nconn * F8_NHYP, "kg_ft8_create"));
        KG_TRY(kg_ext_zero(ctx, q->d_lists.p, (size_t) nconn * F8_NHYP, "kg_ft8_create"));
        return kg_ext_zero(ctx, q->d_samp.p, (size_t) nconn * 2 * F8_SAMP, "kg_ft8_create");
    });
}

void kg_ft8_destroy(kg_ft8 *q) { kg_drain_delete(q); }

int kg_ft8_set_snr_adj(kg_ft8 *q, float snr_adj)
{
    KG_REQUIRE(q != nullptr, KG_ERR_INVALID, "kg_ft8_set_snr_adj: null handle");
    KG_REQUIRE(snr_adj - snr_adj == 0.0f, KG_ERR_INVALID, "kg_ft8_set_snr_adj: snr_adj %g is not finite", (double) snr_adj);
    q->snr_adj = snr_adj;
    return KG_OK;
}

int kg_ft8_init(kg_ft8 *q, int conn, int protocol, double snd_rate)
{
    KG_EXT_INDEX("kg_ft8_init", q, conn, q->nconn, "connection");
    state_t st;
    const int rc = cmd_init(st, protocol, snd_rate);
    KG_REQUIRE(rc != REFUSED_RATE, KG_ERR_INVALID, "kg_ft8_init: snd_rate %g (12000)", snd_rate);
    KG_REQUIRE(rc == 0, KG_ERR_INVALID, "kg_ft8_init: protocol %d (0 FT8, 1 FT4)", protocol);
    KG_TRY(kg_ctx_use(q->ctx));
    KG_HIP(hipMemsetAsync(q->d_samp.p + (size_t) conn * 2 * F8_SAMP, 0, sizeof(float) * MAX_NFFT, q->ctx->stream));        // last_frame of parity 0 (calloc, monitor.c:75)
    q->c[conn].st = st;
    q->c[conn].last_blocks = 0;
    return KG_OK;
}

int kg_ft8_push(kg_ft8 *q, const int32_t *conns, int nconn, const int32_t *ncb, int ns, const int16_t *samples, size_t sample_stride, const double *times,
                size_t time_stride, kg_ft8_ev *evs, int max_events, int32_t *nevents, kg_ft8_slot *slots, int max_slots, int32_t *nslots)
{
    KG_REQUIRE(q && conns && ncb && samples && times && nevents && nslots && (evs || max_events == 0) && (slots || max_slots == 0), KG_ERR_INVALID,
               "kg_ft8_push: null argument");
    KG_TRY(kg_ctx_use(q->ctx));
    f8_plan p;                                          // walked (on copies) ahead of the first copy: a push that will be refused enqueues nothing
    KG_TRY(f8_walk(q, conns, nconn, ncb, nullptr, ns, sample_stride, times, time_stride, max_events, max_slots, p, "kg_ft8_push"));
    size_t last = 0;
    for (int i = 0; i < nconn; i++)
        if (ncb[i] > 0) last = (size_t) i * sample_stride + (size_t) ns * ncb[i];
    int16_t *d_in = nullptr;
    kg_ft8_slot *d_slots = nullptr;
    hipStream_t s = q->ctx->stream;
    kg_scope tmp(q->ctx);                               // the caller's arrays and the temporaries are in use until it has drained the stream
    KG_TRY(tmp.alloc(&d_in, last ? last : 1, "kg_ft8_push: samples"));
    KG_TRY(tmp.alloc(&d_slots, p.ends.empty() ? 1 : p.ends.size(), "kg_ft8_push: slots"));
    for (int i = 0; i < nconn; i++)
        if (ncb[i] > 0)
            KG_HIP(hipMemcpyAsync(d_in + (size_t) i * sample_stride, samples + (size_t) i * sample_stride, sizeof(int16_t) * ns * (size_t) ncb[i], hipMemcpyHostToDevice, s));
    const size_t ne = p.ends.size();
    KG_TRY(f8_enqueue(q, p, d_in, d_slots));
    if (ne) KG_HIP(hipMemcpyAsync(slots, d_slots, sizeof(kg_ft8_slot) * ne, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    if (!p.evs.empty()) memcpy(evs, p.evs.data(), sizeof(kg_ft8_ev) * p.evs.size());
    *nevents = (int32_t) p.evs.size();
    *nslots = (int32_t) ne;
    return KG_OK;                                       // tmp drains the stream
}

int kg_ft8_plan(kg_ft8 *q, const int32_t *conns, int nconn, const int32_t *ncb, int ns, const double *times, size_t time_stride, int32_t *nblocks,
                int32_t *nevents, int32_t *nslots)
{
    KG_REQUIRE(q && conns && ncb && times, KG_ERR_INVALID, "kg_ft8_plan: null argument");
    f8_plan p;
    KG_TRY(f8_walk(q, conns, nconn, ncb, nullptr, ns, ~(size_t) 0 >> 8, times, time_stride, 0x7fffffff, 0x7fffffff, p, "kg_ft8_plan"));
    if (nblocks) *nblocks = (int32_t) (p.blks.size() / TIME_OSR);
    if (nevents) *nevents = (int32_t) p.evs.size();
    if (nslots) *nslots = (int32_t) p.ends.size();
    return KG_OK;
}

int kg_ft8_state(kg_ft8 *q, int conn, kg_ft8_info *info, float *last_frame, uint8_t *mag, int previous)
{
    KG_EXT_INDEX("kg_ft8_state", q, conn, q->nconn, "connection");
    KG_REQUIRE(previous == 0 || previous == 1, KG_ERR_INVALID, "kg_ft8_state: previous %d (0..1)", previous);
    KG_TRY(kg_ctx_use(q->ctx));
    const state_t &w = q->c[conn].st;
    const cfg_t &c = w.cfg;
    hipStream_t s = q->ctx->stream;
    float mx[2][F8_WG];
    KG_HIP(hipMemcpyAsync(mx, q->d_wgmax.p + (size_t) conn * 2 * F8_WG, sizeof mx, hipMemcpyDeviceToHost, s));
    if (last_frame && w.inited)                         // the nfft samples that end at frame_pos; between slots, the tail the next slot will find
        KG_HIP(hipMemcpyAsync(last_frame, q->d_samp.p + ((size_t) conn * 2 + w.parity) * F8_SAMP + (MAX_NFFT - c.nfft) + (w.tsync ? w.frame_pos : 0), sizeof(float) * c.nfft,
                              hipMemcpyDeviceToHost, s));
    const int which = previous ? w.parity ^ 1 : w.parity, nb = previous ? q->c[conn].last_blocks : w.num_blocks;
    if (mag && w.inited && nb > 0)
        KG_HIP(hipMemcpyAsync(mag, q->d_wf.p + ((size_t) conn * F8_NWF + which) * F8_WF, (size_t) nb * c.block_stride, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    if (info) {
        memset(info, 0, sizeof *info);
        info->inited = w.inited; info->protocol = w.protocol; info->tsync = w.tsync; info->in_pos = w.in_pos; info->frame_pos = w.frame_pos;
        info->num_blocks = w.num_blocks; info->parity = w.parity; info->last_blocks = q->c[conn].last_blocks;
        info->block_size = c.block_size; info->nfft = c.nfft; info->num_bins = c.num_bins; info->min_bin = c.min_bin; info->max_blocks = c.max_blocks;
        info->num_samples = c.num_samples; info->slot_blocks = c.slot_blocks; info->block_stride = c.block_stride;
        info->slot = w.slot; info->decode_time = w.decode_time; info->slot_start = w.slot_start;
        info->max_mag = info->last_max_mag = -120.0f;
        for (int t = 0; t < w.num_blocks * TIME_OSR; t++) info->max_mag = mx[w.parity][t] > info->max_mag ? mx[w.parity][t] : info->max_mag;
        for (int t = 0; t < q->c[conn].last_blocks * TIME_OSR; t++) info->last_max_mag = mx[w.parity ^ 1][t] > info->last_max_mag ? mx[w.parity ^ 1][t] : info->last_max_mag;
    }
    return KG_OK;
}

int kg_ft8_load_wf(kg_ft8 *q, int conn, int protocol, int num_blocks, const uint8_t *mag, int num_candidates, int min_score, kg_ft8_slot *slot)
{
    KG_EXT_INDEX("kg_ft8_load_wf", q, conn, q->nconn, "connection");
    KG_REQUIRE(mag && slot, KG_ERR_INVALID, "kg_ft8_load_wf: null argument");
    KG_REQUIRE(protocol == PROTO_FT8 || protocol == PROTO_FT4, KG_ERR_INVALID, "kg_ft8_load_wf: protocol %d (0 FT8, 1 FT4)", protocol);
    const cfg_t &c = q->cfgs.c[protocol];
    KG_REQUIRE(num_blocks >= 1 && num_blocks <= c.max_blocks, KG_ERR_INVALID, "kg_ft8_load_wf: num_blocks %d (1..%d)", num_blocks, c.max_blocks);
    KG_REQUIRE(num_candidates >= 1 && num_candidates <= MAX_CAND, KG_ERR_INVALID, "kg_ft8_load_wf: num_candidates %d (1..%d)", num_candidates, (int) MAX_CAND);
    KG_REQUIRE(min_score >= -32768 && min_score <= 32767, KG_ERR_INVALID, "kg_ft8_load_wf: min_score %d (-32768..32767)", min_score);
    KG_TRY(kg_ctx_use(q->ctx));
    hipStream_t s = q->ctx->stream;
    kg_ft8_slot *d_slot = nullptr;
    kg_scope tmp(q->ctx);
    KG_TRY(tmp.alloc(&d_slot, 1, "kg_ft8_load_wf: slot"));
    KG_HIP(hipMemcpyAsync(q->d_wf.p + ((size_t) conn * F8_NWF + 2) * F8_WF, mag, (size_t) num_blocks * c.block_stride, hipMemcpyHostToDevice, s));
    const f8_end e = {conn, 2, num_blocks, protocol, num_candidates, min_score, 0, 0, 0, {0, 0, 0}};
    void *d_tab = nullptr;
    KG_TRY(kg_ctx_stage(q->ctx, &e, sizeof e, &d_tab));
    KG_TRY(f8_chain(q, (const f8_end *) d_tab, 1, d_slot));
    KG_HIP(hipMemcpyAsync(slot, d_slot, sizeof(kg_ft8_slot), hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    return KG_OK;                                       // tmp drains the stream
}

}  // extern "C"
