// kg_nav.hip -- nav frame sync: the `holding` loop of CHANNEL::Tracking() with ParityCheck, L1_parity and E1B_subframe (kg_nav.h).
//
// A push runs three kinds of kernel over per-channel state in device memory:
//   stage 0  the window: a channel's held tail and its new bits, packed (from bytes, or from kg_trk_epoch rows through the nav-bit machine)
//   stage 1  every head offset of the window judged on its own: C/A one lane per offset; E1B the preamble pair per lane, then the wave
//            decodes each matching offset -- lane s is trellis state s, the old metrics come by cross-lane reads, a step's 64 decisions
//            are one __ballot, kept in two registers of lane t for the chainback
//   stage 2  one lane per channel walks the answers as the reference's loop does, writes the records and keeps the tail
#include "kg_common.h"
#include "kg_nav.h"

#include <new>
#include <vector>

using namespace kg_nav_cf;

static_assert(sizeof(frame) == sizeof(kg_nav_frame) && sizeof(frame) == 64 && offsetof(kg_nav_frame, data) == 24, "kg_nav_frame layout");
static_assert(MODE_L1 == KG_NAV_L1 && MODE_E1B == KG_NAV_E1B && ERR_PARITY == KG_NAV_ERR_PARITY && ERR_SLIP == KG_NAV_ERR_SLIP &&
              ERR_CRC == KG_NAV_ERR_CRC && ERR_ALERT == KG_NAV_ERR_ALERT && ERR_OOS == KG_NAV_ERR_OOS && ERR_PAGE == KG_NAV_ERR_PAGE, "constants");
static_assert(offsetof(kg_trk_epoch, flags) == 40 && sizeof(kg_trk_epoch) == 48, "kg_trk_epoch layout");

struct nav_ws {                           // stage 1's and the window's memory, strides per channel
    uint32_t *win; uint64_t *match; res *rs;
    uint32_t win_stride, match_stride, res_stride;
};

__global__ void nav_reset_kernel(chan *st, int ch, int mode)
{
    chan c;
    c.base = 0; c.pushed = 0; c.mode = mode; c.holding = 0; c.wlen = 0; c.nnew = 0;
    c.nav_ms = 0; c.nav_prev = 0; c.nav_glitch = 0; c.pad_ = 0;
    for (int j = 0; j < HELD_WORDS; j++) c.held[j] = 0;
    st[ch] = c;
}

// stage 0, bytes: one lane per window word
__global__ __launch_bounds__(256) void nav_window_bits_kernel(chan *__restrict__ st, const uint8_t *__restrict__ bits, size_t chan_stride,
                                                              const int32_t *__restrict__ nbits, nav_ws ws, uint32_t nwords)
{
    const uint32_t ch = blockIdx.y, wi = blockIdx.x * 256 + threadIdx.x;
    if (wi >= nwords) return;
    chan *sp = st + ch;
    const uint32_t holding = (uint32_t) sp->holding, n = (uint32_t) nbits[ch], W = holding + n;
    const uint8_t *row = bits + (size_t) ch * chan_stride;
    uint32_t v = 0;
    for (uint32_t b = 0; b < 32; b++) {
        const uint32_t i = 32 * wi + b;
        uint32_t bit = 0;
        if (i < holding) bit = (sp->held[i >> 5] >> (31 - (i & 31))) & 1;
        else if (i < W) bit = row[i - holding] & 1;
        v |= bit << (31 - b);
    }
    ws.win[(size_t) ch * ws.win_stride + wi] = v;
    if (wi == 0) { sp->wlen = (int32_t) W; sp->nnew = (int32_t) n; }
}

// stage 0, epoch rows: one wave per channel; 64 epochs' Inav flags are one ballot, the machine then runs over them in every lane alike
__global__ __launch_bounds__(64) void nav_window_epochs_kernel(chan *__restrict__ st, const kg_trk_epoch *__restrict__ ep, size_t chan_stride,
                                                               const int32_t *__restrict__ counts_in, int epoch_cap, nav_ws ws)
{
    const uint32_t ch = blockIdx.x, lane = threadIdx.x;
    chan *sp = st + ch;
    uint32_t *w = ws.win + (size_t) ch * ws.win_stride;
    const kg_trk_epoch *row = ep + (size_t) ch * chan_stride;
    int32_t cnt = counts_in[ch];
    if (cnt < 0) cnt = -1 - cnt;                                        // a stopped channel's count (kg_trk_process_bits_dev)
    if (cnt > epoch_cap) cnt = epoch_cap;
    const int32_t mode = sp->mode;
    const uint32_t holding = (uint32_t) sp->holding;
    uint32_t nav_ms = sp->nav_ms, nav_prev = sp->nav_prev, nav_glitch = sp->nav_glitch;
    if (lane < (holding >> 5)) w[lane] = sp->held[lane];               // the full words of the tail; the partial one continues in `cur`
    uint32_t p = holding, cur = (p & 31) ? sp->held[p >> 5] : 0u;
    for (int32_t k0 = 0; k0 < cnt; k0 += 64) {
        const int32_t k = k0 + (int32_t) lane;
        const uint32_t f = k < cnt ? row[k].flags : 0u;
        const uint64_t m = __ballot((f & KG_TRK_INAV) != 0);
        const int32_t nn = cnt - k0 < 64 ? cnt - k0 : 64;
        for (int32_t i = 0; i < nn; i++) {
            const uint32_t inav = (uint32_t) (m >> i) & 1;
            if (nav_bit_step(mode, &nav_ms, &nav_prev, &nav_glitch, inav)) {
                cur |= inav << (31 - (p & 31));
                p++;
                if (!(p & 31)) {
                    if (lane == 0) w[(p >> 5) - 1] = cur;
                    cur = 0;
                }
            }
        }
    }
    if (lane == 0) {
        w[p >> 5] = cur; w[(p >> 5) + 1] = 0; w[(p >> 5) + 2] = 0;
        sp->nav_ms = nav_ms; sp->nav_prev = nav_prev; sp->nav_glitch = nav_glitch;
        sp->wlen = (int32_t) p; sp->nnew = (int32_t) (p - holding);
    }
}

// stage 1, C/A: one lane per head offset
__global__ __launch_bounds__(256) void nav_l1_kernel(const chan *__restrict__ st, nav_ws ws)
{
    const uint32_t ch = blockIdx.y, o = blockIdx.x * 256 + threadIdx.x;
    const chan *sp = st + ch;
    if (sp->mode != MODE_L1) return;
    const int32_t W = sp->wlen;
    const uint32_t *w = ws.win + (size_t) ch * ws.win_stride;
    const uint32_t code = (int32_t) o + L1_BITS <= W ? l1_judge(w, o) : 0u;
    const uint64_t m = __ballot(code != 0);
    if (code) ws.rs[(size_t) ch * ws.res_stride + o].code = (int32_t) code;
    if ((threadIdx.x & 63) == 0) ws.match[(size_t) ch * ws.match_stride + (o >> 6)] = m;
}

__device__ inline uint64_t shfl64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t) __shfl((int) (uint32_t) v, src), hi = (uint32_t) __shfl((int) (uint32_t) (v >> 32), src);
    return ((uint64_t) hi << 32) | lo;
}

struct wave_decisions {                   // lane t holds the decision word of step t (lo) and of step 64 + t (hi)
    uint64_t lo, hi;
    __device__ uint64_t operator()(uint32_t t) const { return t < 64 ? shfl64(lo, (int) t) : shfl64(hi, (int) t - 64); }
};

// init_viterbi27_port(.., 0), update_viterbi27_blk_port(.., 120), chainback_viterbi27_port(.., 114, 0) on the half whose first symbol
// is window bit q; every lane returns the same words
__device__ inline void e1b_decode_half(const uint32_t *w, uint32_t q, uint32_t inv, uint32_t lane, uint64_t *o0, uint64_t *o1)
{
    uint32_t metric = lane == 0 ? 0u : 63u;
    wave_decisions d = {0, 0};
#pragma unroll
    for (uint32_t blk = 0; blk < 4; blk++) {                           // 64 encoded symbols = 32 steps at a time
        const uint32_t i = 64 * blk + lane;
        const uint64_t e = __ballot(i < 240 && e1b_enc(w, q, i, inv) != 0);
        const uint32_t steps = blk < 3 ? 32 : 24;
        for (uint32_t tt = 0; tt < steps; tt++) {
            const uint32_t t = 32 * blk + tt;
            const uint32_t sym0 = ((uint32_t) (e >> (2 * tt)) & 1) * 255u, sym1 = ((uint32_t) (e >> (2 * tt + 1)) & 1) * 255u;
            const uint32_t old_lo = (uint32_t) __shfl((int) metric, (int) (lane >> 1)), old_hi = (uint32_t) __shfl((int) metric, (int) (lane >> 1) + 32);
            uint32_t dec;
            metric = v27_step(lane, old_lo, old_hi, sym0, sym1, &dec);
            const uint64_t word = __ballot(dec != 0);
            if (lane == (t & 63)) { if (t < 64) d.lo = word; else d.hi = word; }
        }
    }
    v27_chainback(d, o0, o1);
}

// stage 1, E1B: one wave per 64 head offsets
__global__ __launch_bounds__(64) void nav_e1b_kernel(const chan *__restrict__ st, nav_ws ws)
{
    const uint32_t ch = blockIdx.y, lane = threadIdx.x, o0 = blockIdx.x * 64;
    const chan *sp = st + ch;
    if (sp->mode != MODE_E1B) return;
    const int32_t W = sp->wlen;
    const uint32_t *w = ws.win + (size_t) ch * ws.win_stride;
    const uint32_t pre = (int32_t) (o0 + lane) + E1B_BITS <= W ? e1b_pre(w, o0 + lane) : 0u;
    uint64_t m = __ballot(pre != 0);
    if (lane == 0) ws.match[(size_t) ch * ws.match_stride + blockIdx.x] = m;
    while (m) {
        const uint32_t j = ctz64(m);
        m &= m - 1;
        const uint32_t inv = (uint32_t) __shfl((int) pre, (int) j) - 1, o = o0 + j;
        uint64_t a0, a1, b0, b1;
        e1b_decode_half(w, o + 10, inv, lane, &a0, &a1);
        e1b_decode_half(w, o + 10 + E1B_HALF, inv, lane, &b0, &b1);
        int32_t id;
        const int32_t err = e1b_page(a0, a1, b0, b1, &id);
        if (lane == 0) {
            res r;
            r.code = 0x100 | (int32_t) (inv << 7) | err; r.id = id;
            r.w[0] = a0; r.w[1] = a1; r.w[2] = b0; r.w[3] = b1;
            ws.rs[(size_t) ch * ws.res_stride + o] = r;
        }
    }
}

// stage 2: one lane per channel
__global__ __launch_bounds__(64) void nav_walk_kernel(chan *__restrict__ st, int nchan, nav_ws ws, frame *__restrict__ out, size_t frame_stride,
                                                      int cap, int32_t *__restrict__ counts)
{
    const int ch = (int) threadIdx.x;
    if (ch >= nchan) return;
    counts[ch] = walk(st[ch], ws.win + (size_t) ch * ws.win_stride, ws.match + (size_t) ch * ws.match_stride, ws.rs + (size_t) ch * ws.res_stride,
                      out + (size_t) ch * frame_stride, cap);
}

struct kg_nav {
    kg_ctx *ctx;
    int nchan;
    std::vector<int> mode;              // the host's mirror (the cap bound, which stage 1 kernels to launch)
    kg_dbuf<chan> d_chan;
    kg_dbuf<uint32_t> d_win;            // the workspace: all three or none
    kg_dbuf<uint64_t> d_match;
    kg_dbuf<res> d_rs;
    nav_ws ws;                          // the kernels' view of the workspace
    uint32_t ws_bits;                   // the window length the workspace holds (published last)
};

// the workspace for windows of up to wbits bits: grows, never shrinks
static int nav_reserve(kg_nav *v, uint64_t wbits)
{
    if (wbits <= v->ws_bits) return KG_OK;
    KG_HIP(hipStreamSynchronize(v->ctx->stream));                       // kernels of earlier pushes still use the old one
    v->d_win.reset(); v->d_match.reset(); v->d_rs.reset();
    v->ws = nav_ws{nullptr, nullptr, nullptr, 0, 0, 0}; v->ws_bits = 0;
    const uint64_t bits = (wbits + 4095) & ~(uint64_t) 4095;
    const uint32_t win_stride = (uint32_t) (bits / 32 + 4), match_stride = (uint32_t) (bits / 64 + 4), res_stride = (uint32_t) bits;
    int rc;
    if ((rc = v->d_win.alloc((size_t) win_stride * v->nchan, "kg_nav: windows")) != KG_OK ||
        (rc = v->d_match.alloc((size_t) match_stride * v->nchan, "kg_nav: matches")) != KG_OK ||
        (rc = v->d_rs.alloc((size_t) res_stride * v->nchan, "kg_nav: results")) != KG_OK) {
        v->d_win.reset(); v->d_match.reset();
        return rc;
    }
    v->ws = nav_ws{v->d_win, v->d_match, v->d_rs, win_stride, match_stride, res_stride};
    v->ws_bits = (uint32_t) bits;
    return KG_OK;
}

// stages 1 and 2 over windows of at most wmax bits
static int nav_judge(kg_nav *v, uint64_t wmax, kg_nav_frame *d_frames, size_t frame_stride, int cap, int32_t *d_counts)
{
    bool l1 = false, e1b = false;
    for (int m : v->mode) (m == MODE_E1B ? e1b : l1) = true;
    hipStream_t s = v->ctx->stream;
    if (l1 && wmax >= L1_BITS)
        hipLaunchKernelGGL(nav_l1_kernel, dim3((unsigned) ((wmax - L1_BITS) / 256 + 1), v->nchan), dim3(256), 0, s, (const chan *) v->d_chan, v->ws);
    if (e1b && wmax >= E1B_BITS)
        hipLaunchKernelGGL(nav_e1b_kernel, dim3((unsigned) ((wmax - E1B_BITS) / 64 + 1), v->nchan), dim3(64), 0, s, (const chan *) v->d_chan, v->ws);
    hipLaunchKernelGGL(nav_walk_kernel, dim3(1), dim3(64), 0, s, v->d_chan, v->nchan, v->ws, (frame *) d_frames, frame_stride, cap, d_counts);
    KG_HIP(hipGetLastError());
    return KG_OK;
}

static int nav_check_out(const char *who, const kg_nav_frame *d_frames, size_t frame_stride, int cap, const int32_t *d_counts, int64_t need)
{
    KG_REQUIRE(cap >= 0 && (int64_t) cap >= need, KG_ERR_INVALID, "%s: cap %d below %lld (one record per 30 new bits of a C/A channel, per 250 of an E1B one)",
               who, cap, (long long) need);
    KG_REQUIRE(frame_stride >= (size_t) cap, KG_ERR_INVALID, "%s: frame_stride %zu below cap %d", who, frame_stride, cap);
    KG_REQUIRE(KG_ALIGNED(d_frames, 8) && KG_ALIGNED(d_counts, 4), KG_ERR_INVALID, "%s: d_frames needs 8-byte, d_counts 4-byte alignment", who);
    return KG_OK;
}

static int nav_init(kg_nav *v)
{
    v->mode.assign(v->nchan, MODE_L1);
    int rc = v->d_chan.alloc(v->nchan, "kg_nav_create: channels");
    if (rc) return rc;
    for (int ch = 0; ch < v->nchan; ch++) hipLaunchKernelGGL(nav_reset_kernel, dim3(1), dim3(1), 0, v->ctx->stream, v->d_chan.p, ch, (int) MODE_L1);
    KG_TRY(nav_reserve(v, 4096));
    KG_REQUIRE(hipGetLastError() == hipSuccess, KG_ERR_HIP, "kg_nav_create: launch failed");
    return KG_OK;
}

extern "C" {

int kg_nav_create(kg_ctx *ctx, int nchan, kg_nav **out)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "kg_nav_create: out is null");
    *out = nullptr;
    KG_REQUIRE(nchan >= 1 && nchan <= KG_TRK_MAX_CHANS, KG_ERR_INVALID, "kg_nav_create: nchan %d (1..%d)", nchan, KG_TRK_MAX_CHANS);
    kg_nav *v = new (std::nothrow) kg_nav();
    KG_REQUIRE(v != nullptr, KG_ERR_NOMEM, "kg_nav_create: alloc");
    v->ctx = ctx; v->nchan = nchan;
    rc = nav_init(v);
    if (rc) { kg_nav_destroy(v); return rc; }
    *out = v;
    return KG_OK;
}

void kg_nav_destroy(kg_nav *v) { kg_drain_delete(v); }

int kg_nav_set_mode(kg_nav *v, int ch, int mode)
{
    KG_REQUIRE(v != nullptr, KG_ERR_INVALID, "kg_nav_set_mode: null handle");
    KG_REQUIRE(ch >= 0 && ch < v->nchan, KG_ERR_INVALID, "kg_nav_set_mode: channel %d of %d", ch, v->nchan);
    KG_REQUIRE(mode == KG_NAV_L1 || mode == KG_NAV_E1B, KG_ERR_INVALID, "kg_nav_set_mode: mode %d", mode);
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(nav_reset_kernel, dim3(1), dim3(1), 0, v->ctx->stream, v->d_chan, ch, mode);
    KG_HIP(hipGetLastError());
    v->mode[ch] = mode;
    return KG_OK;
}

int kg_nav_push_bits_dev(kg_nav *v, const uint8_t *d_bits, size_t chan_stride, const int32_t *nbits, kg_nav_frame *d_frames,
                         size_t frame_stride, int cap, int32_t *d_counts)
{
    KG_REQUIRE(v && d_bits && nbits && d_frames && d_counts, KG_ERR_INVALID, "kg_nav_push_bits_dev: null argument");
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    int64_t need = 0, nmax = 0;
    for (int ch = 0; ch < v->nchan; ch++) {
        KG_REQUIRE(nbits[ch] >= 0 && nbits[ch] <= KG_NAV_MAX_PUSH, KG_ERR_INVALID, "kg_nav_push_bits_dev: nbits[%d] = %d outside 0..%d", ch, nbits[ch],
                   KG_NAV_MAX_PUSH);
        KG_REQUIRE((size_t) nbits[ch] <= chan_stride || v->nchan == 1, KG_ERR_INVALID, "kg_nav_push_bits_dev: nbits[%d] = %d beyond chan_stride %zu", ch,
                   nbits[ch], chan_stride);
        const int64_t r = max_records(v->mode[ch], nbits[ch]);
        if (r > need) need = r;
        if (nbits[ch] > nmax) nmax = nbits[ch];
    }
    rc = nav_check_out("kg_nav_push_bits_dev", d_frames, frame_stride, cap, d_counts, need);
    if (rc) return rc;
    const uint64_t wmax = (uint64_t) nmax + E1B_BITS - 1;
    rc = nav_reserve(v, wmax);
    if (rc) return rc;
    void *d_n = nullptr;
    rc = kg_ctx_stage(v->ctx, nbits, sizeof(int32_t) * v->nchan, &d_n);
    if (rc) return rc;
    KG_PLAN_ONLY(v->ctx);
    const uint32_t nwords = (uint32_t) (wmax / 32 + 3);
    hipLaunchKernelGGL(nav_window_bits_kernel, dim3((nwords + 255) / 256, v->nchan), dim3(256), 0, v->ctx->stream, v->d_chan, d_bits, chan_stride,
                       (const int32_t *) d_n, v->ws, nwords);
    return nav_judge(v, wmax, d_frames, frame_stride, cap, d_counts);
}

int kg_nav_push_epochs_dev(kg_nav *v, const kg_trk_epoch *d_epochs, size_t chan_stride, const int32_t *d_counts_in, int epoch_cap,
                           kg_nav_frame *d_frames, size_t frame_stride, int cap, int32_t *d_counts)
{
    KG_REQUIRE(v && d_epochs && d_counts_in && d_frames && d_counts, KG_ERR_INVALID, "kg_nav_push_epochs_dev: null argument");
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    KG_REQUIRE(epoch_cap >= 0 && epoch_cap <= KG_NAV_MAX_PUSH, KG_ERR_INVALID, "kg_nav_push_epochs_dev: epoch_cap %d outside 0..%d", epoch_cap, KG_NAV_MAX_PUSH);
    KG_REQUIRE(chan_stride >= (size_t) epoch_cap || v->nchan == 1, KG_ERR_INVALID, "kg_nav_push_epochs_dev: chan_stride %zu below epoch_cap %d", chan_stride,
               epoch_cap);
    KG_REQUIRE(KG_ALIGNED(d_epochs, 8) && KG_ALIGNED(d_counts_in, 4), KG_ERR_INVALID, "kg_nav_push_epochs_dev: d_epochs needs 8-byte, d_counts_in 4-byte alignment");
    int64_t need = 0, nmax = 0;
    for (int ch = 0; ch < v->nchan; ch++) {                             // E1B saves every epoch, C/A at most one bit per 20 epochs
        const int64_t nb = v->mode[ch] == MODE_E1B ? epoch_cap : (epoch_cap + 19) / 20;
        const int64_t r = max_records(v->mode[ch], nb);
        if (r > need) need = r;
        if (nb > nmax) nmax = nb;
    }
    rc = nav_check_out("kg_nav_push_epochs_dev", d_frames, frame_stride, cap, d_counts, need);
    if (rc) return rc;
    const uint64_t wmax = (uint64_t) nmax + E1B_BITS - 1;
    rc = nav_reserve(v, wmax);
    if (rc) return rc;
    hipLaunchKernelGGL(nav_window_epochs_kernel, dim3(v->nchan), dim3(64), 0, v->ctx->stream, v->d_chan, d_epochs, chan_stride, d_counts_in, epoch_cap,
                       v->ws);
    return nav_judge(v, wmax, d_frames, frame_stride, cap, d_counts);
}

int kg_nav_push_bits(kg_nav *v, const uint8_t *bits, size_t chan_stride, const int32_t *nbits, kg_nav_frame *frames, size_t frame_stride, int cap,
                     int32_t *counts)
{
    KG_REQUIRE(v && bits && nbits && frames && counts, KG_ERR_INVALID, "kg_nav_push_bits: null argument");
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    KG_REQUIRE(cap >= 0 && frame_stride >= (size_t) cap, KG_ERR_INVALID, "kg_nav_push_bits: cap %d, frame_stride %zu", cap, frame_stride);
    size_t in_bytes = 0;
    int64_t need = 0;
    for (int ch = 0; ch < v->nchan; ch++) {
        KG_REQUIRE(nbits[ch] >= 0 && nbits[ch] <= KG_NAV_MAX_PUSH, KG_ERR_INVALID, "kg_nav_push_bits: nbits[%d] = %d outside 0..%d", ch, nbits[ch], KG_NAV_MAX_PUSH);
        KG_REQUIRE((size_t) nbits[ch] <= chan_stride || v->nchan == 1, KG_ERR_INVALID, "kg_nav_push_bits: nbits[%d] = %d beyond chan_stride %zu", ch, nbits[ch],
                   chan_stride);                        // before anything is copied: a row must not run into the next one or past the buffer
        const int64_t r = max_records(v->mode[ch], nbits[ch]);
        if (r > need) need = r;
        if (nbits[ch]) in_bytes = (size_t) ch * chan_stride + (size_t) nbits[ch];
    }
    KG_REQUIRE((int64_t) cap >= need, KG_ERR_INVALID, "kg_nav_push_bits: cap %d below %lld (one record per 30 new bits of a C/A channel, per 250 of an E1B one)",
               cap, (long long) need);
    const size_t fcount = (frame_stride ? frame_stride : 1) * v->nchan;
    uint8_t *d_bits = nullptr;
    kg_nav_frame *d_fr = nullptr;
    int32_t *d_cnt = nullptr;
    hipStream_t s = v->ctx->stream;
    kg_scope tmp(v->ctx);
    KG_TRY(tmp.alloc(&d_bits, in_bytes ? in_bytes : 1, "kg_nav_push_bits: bits"));
    KG_TRY(tmp.alloc(&d_fr, fcount, "kg_nav_push_bits: frames"));
    KG_TRY(tmp.alloc(&d_cnt, v->nchan, "kg_nav_push_bits: counts"));
    for (int ch = 0; ch < v->nchan; ch++)
        if (nbits[ch]) KG_HIP(hipMemcpyAsync(d_bits + (size_t) ch * chan_stride, bits + (size_t) ch * chan_stride, (size_t) nbits[ch], hipMemcpyHostToDevice, s));
    KG_TRY(kg_nav_push_bits_dev(v, d_bits, chan_stride, nbits, d_fr, frame_stride, cap, d_cnt));
    KG_HIP(hipMemcpyAsync(counts, d_cnt, sizeof(int32_t) * v->nchan, hipMemcpyDeviceToHost, s));
    KG_HIP(hipStreamSynchronize(s));
    for (int ch = 0; ch < v->nchan; ch++)
        if (counts[ch] > 0)
            KG_HIP(hipMemcpy(frames + (size_t) ch * frame_stride, d_fr + (size_t) ch * frame_stride, sizeof(kg_nav_frame) * counts[ch], hipMemcpyDeviceToHost));
    return KG_OK;
}

int kg_nav_get_state(kg_nav *v, int ch, int32_t *holding, uint64_t *bit0, uint8_t *held, uint64_t *pushed, int32_t *nav)
{
    KG_REQUIRE(v != nullptr, KG_ERR_INVALID, "kg_nav_get_state: null handle");
    KG_REQUIRE(ch >= 0 && ch < v->nchan, KG_ERR_INVALID, "kg_nav_get_state: channel %d of %d", ch, v->nchan);
    KG_REQUIRE(holding && bit0 && held && pushed && nav, KG_ERR_INVALID, "kg_nav_get_state: null argument");
    int rc = kg_ctx_use(v->ctx);
    if (rc) return rc;
    chan c;
    KG_HIP(hipMemcpyAsync(&c, v->d_chan + ch, sizeof c, hipMemcpyDeviceToHost, v->ctx->stream));
    KG_HIP(hipStreamSynchronize(v->ctx->stream));
    *holding = c.holding; *bit0 = c.base; *pushed = c.pushed;
    for (int i = 0; i < c.holding; i++) held[i] = (uint8_t) ((c.held[i >> 5] >> (31 - (i & 31))) & 1);
    nav[0] = (int32_t) c.nav_ms; nav[1] = (int32_t) c.nav_prev; nav[2] = (int32_t) c.nav_glitch;
    return KG_OK;
}

}  // extern "C"
