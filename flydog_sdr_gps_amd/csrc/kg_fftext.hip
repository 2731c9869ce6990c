// kg_fftext.hip -- the FFT extension (extensions/FFT/FFT.cpp; csrc/kg_fftext.h is the one definition of its arithmetic).
//
// The schedule of fft_data (:72-101) depends on no sample, so the host runs it per call and hands the kernel a table: per listed
// channel a group {channel, its blocks' range in the op list, zero-first, integ, scale}, per taken block an op {where its spectrum
// is, bin, row}.  ONE launch per call: grid (4, groups), 64 lanes.  A lane owns four adjacent columns c0 .. c0 + 3 (c0 ^ 512 keeps
// them adjacent in the row): per block it reads 32 bytes of the spectrum, forms four bytes and stores ONE dword of the row; the four
// sums live in registers while consecutive blocks fall in the same bin, and move as one 16-byte load / store when the bin changes.
// The additions of a column happen in this one lane, in block order: no atomics, no reassociation.
// Block shape: 1024 columns at four a lane are 256 lanes a channel; as four workgroups of ONE wave64 they land on four compute units
// (14 channels: 56 units, not 14), each wave with its CU's whole issue rate -- the work per block is a chain of four log10f behind one
// load, so what hides its latency is other waves on other units, not more waves in a workgroup; nothing is exchanged between lanes,
// so the kernel has no LDS and no barrier.
#include "kg_ext.h"
#include "kg_fftext.h"
#include "kg_spec.h"

using namespace kg_fftext_cf;

static_assert(WIDTH == KG_FFTEXT_ROW && MAX_BINS == KG_FFTEXT_MAX_BINS && UPDATE_MS == KG_FFTEXT_UPDATE_MS && FUNC_OFF == KG_FFTEXT_OFF &&
              FUNC_WF == KG_FFTEXT_WF && FUNC_SPEC == KG_FFTEXT_SPEC && FUNC_INTEG == KG_FFTEXT_INTEG && PASSBAND == KG_SPEC_PASSBAND &&
              CHAN_NULL == KG_SPEC_CHAN_NULL && WIDTH == kg_spec::WIDTH, "constants");
static_assert(sizeof(kg_fftext_info) == 56 && offsetof(kg_fftext_info, fi) == 32, "kg_fftext_info layout");

enum { FX_ZERO = 1, FX_INTEG = 2 };
enum { FX_LANES = 64, FX_COLS = 4, FX_WGS = WIDTH / (FX_LANES * FX_COLS) };      // 4 workgroups a channel
enum { FX_MAX_CHANS = 1024, FX_MAX_LIST = 65536, FX_MAX_BLK = 4096 };
struct fx_group { int32_t ch, first, nops, flags; float scale; int32_t pad[3]; };
struct fx_op { int64_t off; int32_t bin, row; };                                  // off: complex samples from d_spec
static_assert(sizeof(fx_group) == 32 && sizeof(fx_op) == 16, "table layout");

// groups / ops: wave-uniform reads.  pwr: [channel][MAX_BINS][WIDTH].
__global__ __launch_bounds__(FX_LANES) void fftext_kernel(const fx_group *__restrict__ groups, const fx_op *__restrict__ ops,
                                                          const float2 *__restrict__ spec, unsigned char *__restrict__ rows, long row_stride,
                                                          float *__restrict__ pwr)
{
    const fx_group g = groups[blockIdx.y];
    const int c0 = (int) (blockIdx.x * FX_LANES + threadIdx.x) * FX_COLS;
    float4 *slab = reinterpret_cast<float4 *>(pwr + (size_t) g.ch * MAX_BINS * WIDTH + c0);      // bin b: slab[b * (WIDTH / 4)]
    if (g.flags & FX_ZERO)                                                  // the latched reset (:85), ahead of the first block
        for (int b = 0; b < MAX_BINS; b++) slab[b * (WIDTH / 4)] = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool integ = (g.flags & FX_INTEG) != 0;
    float acc[FX_COLS] = {0.f, 0.f, 0.f, 0.f};
    int cur = -1;
    for (int k = 0; k < g.nops; k++) {
        const fx_op op = ops[g.first + k];
        if (op.bin != cur) {                                                // this lane wrote what it now reads: program order holds
            if (cur >= 0) slab[cur * (WIDTH / 4)] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            cur = op.bin;
            if (integ) {
                const float4 v = slab[cur * (WIDTH / 4)];
                acc[0] = v.x; acc[1] = v.y; acc[2] = v.z; acc[3] = v.w;
            }
        }
        const float2 *s = spec + op.off + c0;
        unsigned d = 0;
#pragma unroll
        for (int j = 0; j < FX_COLS; j++) {
            const float2 x = s[j];
            const float p = power(x.x, x.y, integ);
            acc[j] = integ ? acc[j] + p : p;
            d |= (unsigned) bin_byte(acc[j], g.scale) << (8 * j);
        }
        *reinterpret_cast<unsigned *>(rows + (long) op.row * row_stride + unwrap(c0)) = d;
    }
    if (cur >= 0) slab[cur * (WIDTH / 4)] = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

struct fx_chan {
    state_t st;
    int32_t ncma[MAX_BINS];
    bool zero;                                  // the device sums are to be zeroed ahead of the next block taken
};

struct kg_fftext {
    kg_ctx *ctx;
    int nchan;
    double rate;                                // 0: not set
    std::vector<fx_chan> ch;
    kg_dbuf<float> d_pwr;                       // [nchan][MAX_BINS][WIDTH]
};

static void chan_fresh(fx_chan &c, bool zero)
{
    init(c.st);
    memset(c.ncma, 0, sizeof c.ncma);
    c.zero = zero;
}

// What a call does to the channels it lists, on copies; committed when nothing was refused.
struct fx_plan {
    std::vector<fx_chan> ch;                    // copies of the listed channels, in order of first appearance
    std::vector<int> slot, chan;                // channel -> index in ch, or -1; and back
    std::vector<std::vector<fx_op>> ops;        // per listed channel
    std::vector<int32_t> rx, ent, blk, bin;          // per row
};

static int fx_walk(kg_fftext *fx, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const int32_t *spec_row,
                   size_t spec_stride, int max_rows, fx_plan &p, const char *who)
{
    KG_REQUIRE(nch >= 1 && nch <= FX_MAX_LIST, KG_ERR_INVALID, "%s: nch %d (1..%d)", who, nch, FX_MAX_LIST);
    KG_REQUIRE(max_rows >= 0, KG_ERR_INVALID, "%s: max_rows %d", who, max_rows);
    p.slot.assign(fx->nchan, -1);
    for (int i = 0; i < nch; i++) {
        const int c = chans[i];
        KG_REQUIRE(c >= 0 && c < fx->nchan, KG_ERR_INVALID, "%s: chans[%d] = %d of %d", who, i, c, fx->nchan);
        KG_REQUIRE(nblk[i] >= 0 && nblk[i] <= FX_MAX_BLK, KG_ERR_INVALID, "%s: nblk[%d] = %d (0..%d)", who, i, nblk[i], FX_MAX_BLK);
        KG_REQUIRE(inst[i] == PASSBAND || inst[i] == CHAN_NULL, KG_ERR_INVALID, "%s: inst[%d] = %d", who, i, inst[i]);
        KG_REQUIRE(!spec_row || spec_row[i] >= 0, KG_ERR_INVALID, "%s: spectrum row %d of entry %d", who, spec_row ? spec_row[i] : 0, i);
        KG_REQUIRE(nblk[i] <= 0 || nch == 1 || spec_row || spec_stride >= (size_t) WIDTH * nblk[i], KG_ERR_INVALID, "%s: spec_stride %zu below the %d blocks of entry %d",
                   who, spec_stride, nblk[i], i);
        if (p.slot[c] < 0) {
            p.slot[c] = (int) p.ch.size();
            p.ch.push_back(fx->ch[c]);
            p.chan.push_back(c);
            p.ops.emplace_back();
        }
        fx_chan &w = p.ch[p.slot[c]];
        for (int b = 0; b < nblk[i]; b++) {
            int bin = 0, did_reset = 0;
            KG_REQUIRE(fx->rate > 0 || w.st.run == FUNC_OFF || inst[i] != w.st.instance || !w.st.reset, KG_ERR_STATE,
                       "%s: channel %d has a reset latched and no sample rate was set (kg_fftext_set_rate)", who, c);
            const int r = block(w.st, inst[i], fx->rate, &bin, &did_reset);
            KG_REQUIRE(r != REFUSED_TIME, KG_ERR_STATE, "%s: channel %d integrates over a period of %g s (kg_fftext_set_itime: finite, above 0)", who, c,
                       w.st.time);
            KG_REQUIRE(r >= 0, KG_ERR_STATE, "%s: channel %d: a period of %g s is not an int's worth of blocks", who, c, w.st.time);
            if (did_reset) {                                             // :85-86; blocks taken earlier in this call would be lost: there are none,
                memset(w.ncma, 0, sizeof w.ncma);                        // the latch is applied ahead of the channel's first block
                w.zero = true;
            }
            if (r == 0) continue;
            KG_REQUIRE(bin >= 0 && bin < MAX_BINS, KG_ERR_STATE, "%s: channel %d: bin %d", who, c, bin);
            if (w.st.run == FUNC_INTEG) w.ncma[bin]++;
            KG_REQUIRE((int) p.rx.size() < max_rows, KG_ERR_INVALID, "%s: more rows than max_rows = %d", who, max_rows);
            const fx_op op = {(int64_t) ((size_t) (spec_row ? spec_row[i] : i) * spec_stride + (size_t) WIDTH * b), bin, (int32_t) p.rx.size()};
            p.ops[p.slot[c]].push_back(op);
            p.rx.push_back(c); p.ent.push_back(i); p.blk.push_back(b); p.bin.push_back(bin);
        }
    }
    return KG_OK;
}

extern "C" {

int kg_fftext_create(kg_ctx *ctx, int nchan, kg_fftext **out)
{
    return kg_ext_create(ctx, nchan, FX_MAX_CHANS, "kg_fftext_create", "nchan", out, [=](kg_fftext *fx) {
        fx->nchan = nchan; fx->rate = 0;
        fx->ch.resize(nchan);
        for (fx_chan &c : fx->ch) chan_fresh(c, false);
        const size_t n = (size_t) nchan * MAX_BINS * WIDTH;
        KG_TRY(fx->d_pwr.alloc(n, "kg_fftext_create: sums"));
        return kg_ext_zero(ctx, fx->d_pwr.p, n, "kg_fftext_create");
    });
}

void kg_fftext_destroy(kg_fftext *fx) { kg_drain_delete(fx); }

int kg_fftext_set_rate(kg_fftext *fx, double sample_rate)
{
    KG_REQUIRE(fx != nullptr, KG_ERR_INVALID, "kg_fftext_set_rate: null handle");
    KG_REQUIRE(sample_rate > 0 && sample_rate <= 1e12, KG_ERR_INVALID, "kg_fftext_set_rate: sample rate %g", sample_rate);
    fx->rate = sample_rate;
    return KG_OK;
}

int kg_fftext_set_run(kg_fftext *fx, int ch, int run, int is_sam, int is_qam)
{
    KG_EXT_INDEX("kg_fftext_set_run", fx, ch, fx->nchan, "channel");
    KG_REQUIRE(cmd_run(fx->ch[ch].st, run, is_sam != 0, is_qam != 0) == 0, KG_ERR_INVALID, "kg_fftext_set_run: run %d (-1..2)", run);
    return KG_OK;
}

int kg_fftext_set_itime(kg_fftext *fx, int ch, double itime)
{
    KG_EXT_INDEX("kg_fftext_set_itime", fx, ch, fx->nchan, "channel");
    cmd_itime(fx->ch[ch].st, itime);
    return KG_OK;
}

int kg_fftext_clear(kg_fftext *fx, int ch)
{
    KG_EXT_INDEX("kg_fftext_clear", fx, ch, fx->nchan, "channel");
    cmd_clear(fx->ch[ch].st);
    return KG_OK;
}

int kg_fftext_restart(kg_fftext *fx, int ch)
{
    KG_EXT_INDEX("kg_fftext_restart", fx, ch, fx->nchan, "channel");
    chan_fresh(fx->ch[ch], true);
    return KG_OK;
}

int kg_fftext_due(kg_fftext *fx, int ch, uint32_t now_ms)
{
    KG_EXT_INDEX("kg_fftext_due", fx, ch, fx->nchan, "channel");
    return due(fx->ch[ch].st, now_ms);
}

int kg_fftext_process_dev(kg_fftext *fx, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const float *d_spec,
                          size_t spec_stride, uint8_t *d_rows, size_t row_stride, int max_rows, int32_t *rx_of_row, int32_t *ent_of_row,
                          int32_t *blk_of_row, int32_t *bin_of_row)
{
    return kg_fftext_process_rows_(fx, chans, nch, nblk, inst, nullptr, d_spec, spec_stride, d_rows, row_stride, max_rows, rx_of_row, ent_of_row,
                                   blk_of_row, bin_of_row);
}

}  // extern "C"

// kg_fftext_process_dev with the spectra placed by the caller: entry i's blocks from d_spec + 2 * spec_row[i] * spec_stride on (null: row i);
// rows the caller places may be any number of blocks long
int kg_fftext_process_rows_(kg_fftext *fx, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const int32_t *spec_row,
                            const float *d_spec, size_t spec_stride, uint8_t *d_rows, size_t row_stride, int max_rows, int32_t *rx_of_row,
                            int32_t *ent_of_row, int32_t *blk_of_row, int32_t *bin_of_row)
{
    KG_REQUIRE(fx && chans && nblk && inst && d_spec && d_rows, KG_ERR_INVALID, "kg_fftext_process_dev: null argument");
    int rc = kg_ctx_use(fx->ctx);
    if (rc) return rc;
    KG_REQUIRE(KG_ALIGNED(d_spec, 8) && KG_ALIGNED(d_rows, 4) && (row_stride & 3) == 0, KG_ERR_INVALID,
               "kg_fftext_process_dev: d_spec must be 8-byte aligned, d_rows and row_stride multiples of 4 bytes");
    KG_REQUIRE(row_stride >= (size_t) WIDTH || max_rows <= 1, KG_ERR_INVALID, "kg_fftext_process_dev: row_stride %zu < 1024", row_stride);
    fx_plan p;
    KG_TRY(fx_walk(fx, chans, nch, nblk, inst, spec_row, spec_stride, max_rows, p, "kg_fftext_process_dev"));
    // the table: groups, then ops.  A listed channel with nothing to add and nothing to zero gives no group.
    std::vector<int> of_group;
    size_t nops = 0;
    for (size_t k = 0; k < p.ch.size(); k++)
        if (!p.ops[k].empty() || p.ch[k].zero) { of_group.push_back((int) k); nops += p.ops[k].size(); }
    const int nrows = (int) p.rx.size();
    if (!of_group.empty()) {
        std::vector<unsigned char> tab(sizeof(fx_group) * of_group.size() + sizeof(fx_op) * nops);
        fx_group *g = reinterpret_cast<fx_group *>(tab.data());
        fx_op *o = reinterpret_cast<fx_op *>(tab.data() + sizeof(fx_group) * of_group.size());
        int32_t first = 0;
        for (size_t j = 0; j < of_group.size(); j++) {
            const int k = of_group[j];
            const state_t &st = p.ch[k].st;
            g[j] = fx_group{p.chan[k], first, (int32_t) p.ops[k].size(), (p.ch[k].zero ? FX_ZERO : 0) | (st.run == FUNC_INTEG ? FX_INTEG : 0),
                            row_scale(st.run, st.fft_scale, st.spectrum_scale), {0, 0, 0}};
            if (!p.ops[k].empty()) memcpy(o + first, p.ops[k].data(), sizeof(fx_op) * p.ops[k].size());
            first += (int32_t) p.ops[k].size();
        }
        void *d_tab = nullptr;
        if ((rc = kg_ctx_stage(fx->ctx, tab.data(), tab.size(), &d_tab))) return rc;
        KG_PLAN_ONLY(fx->ctx);
        hipLaunchKernelGGL(fftext_kernel, dim3(FX_WGS, (unsigned) of_group.size()), dim3(FX_LANES), 0, fx->ctx->stream, (const fx_group *) d_tab,
                           (const fx_op *) ((const unsigned char *) d_tab + sizeof(fx_group) * of_group.size()), (const float2 *) d_spec,
                           (unsigned char *) d_rows, (long) row_stride, fx->d_pwr.p);
        KG_HIP(hipGetLastError());
    } else {
        KG_PLAN_ONLY(fx->ctx);
    }
    for (int c = 0; c < fx->nchan; c++)                                  // commit: the schedule advanced, the zeroing is enqueued
        if (p.slot[c] >= 0) { fx->ch[c] = p.ch[p.slot[c]]; fx->ch[c].zero = false; }
    for (int r = 0; r < nrows; r++) {
        if (rx_of_row) rx_of_row[r] = p.rx[r];
        if (ent_of_row) ent_of_row[r] = p.ent[r];
        if (blk_of_row) blk_of_row[r] = p.blk[r];
        if (bin_of_row) bin_of_row[r] = p.bin[r];
    }
    return nrows;
}

extern "C" {

int kg_fftext_process(kg_fftext *fx, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst, const float *spec,
                      size_t spec_stride, uint8_t *rows, size_t row_stride, int max_rows, int32_t *rx_of_row, int32_t *ent_of_row,
                      int32_t *blk_of_row, int32_t *bin_of_row)
{
    KG_REQUIRE(fx && chans && nblk && inst && spec && rows, KG_ERR_INVALID, "kg_fftext_process: null argument");
    int rc = kg_ctx_use(fx->ctx);
    if (rc) return rc;
    KG_REQUIRE(nch >= 1 && nch <= FX_MAX_LIST && max_rows >= 1, KG_ERR_INVALID, "kg_fftext_process: nch %d (1..%d), max_rows %d", nch, FX_MAX_LIST, max_rows);
    KG_REQUIRE(row_stride >= (size_t) WIDTH || max_rows == 1, KG_ERR_INVALID, "kg_fftext_process: row_stride %zu < 1024", row_stride);
    size_t last = 0;
    for (int i = 0; i < nch; i++) {
        KG_REQUIRE(nblk[i] >= 0 && nblk[i] <= FX_MAX_BLK, KG_ERR_INVALID, "kg_fftext_process: nblk[%d] = %d (0..%d)", i, nblk[i], FX_MAX_BLK);
        KG_REQUIRE(nblk[i] <= 0 || nch == 1 || spec_stride >= (size_t) WIDTH * nblk[i], KG_ERR_INVALID, "kg_fftext_process: spec_stride %zu below the %d blocks of entry %d",
                   spec_stride, nblk[i], i);
        if (nblk[i] > 0) last = (size_t) i * spec_stride + (size_t) WIDTH * nblk[i];
    }
    const size_t rs = (row_stride + 3) & ~(size_t) 3, rbytes = rs * (size_t) (max_rows - 1) + WIDTH;
    float *d_spec = nullptr;
    uint8_t *d_rows = nullptr;
    hipStream_t s = fx->ctx->stream;
    kg_scope tmp(fx->ctx);                              // the caller's arrays and the temporaries are in use until it has drained the stream
    KG_TRY(tmp.alloc(&d_spec, 2 * (last ? last : 1), "kg_fftext_process: spectra"));
    KG_TRY(tmp.alloc(&d_rows, rbytes, "kg_fftext_process: rows"));
    for (int i = 0; i < nch; i++)
        if (nblk[i] > 0)
            KG_HIP(hipMemcpyAsync(d_spec + 2 * (size_t) i * spec_stride, spec + 2 * (size_t) i * spec_stride, sizeof(float) * 2 * WIDTH * (size_t) nblk[i],
                                  hipMemcpyHostToDevice, s));
    const int n = kg_fftext_process_dev(fx, chans, nch, nblk, inst, d_spec, spec_stride, d_rows, rs, max_rows, rx_of_row, ent_of_row, blk_of_row, bin_of_row);
    for (int r = 0; r < n; r++)
        KG_HIP(hipMemcpyAsync(rows + (size_t) r * row_stride, d_rows + (size_t) r * rs, WIDTH, hipMemcpyDeviceToHost, s));
    return n;                                           // tmp drains the stream: `rows` is filled when the caller sees it
}

int kg_fftext_state(kg_fftext *fx, int ch, kg_fftext_info *info, float *pwr, int32_t *ncma)
{
    KG_EXT_INDEX("kg_fftext_state", fx, ch, fx->nchan, "channel");
    const fx_chan &c = fx->ch[ch];
    if (info) {
        const state_t &e = c.st;
        *info = kg_fftext_info{e.run, e.instance, e.fft_scale, e.spectrum_scale, e.bins, e.reset, e.last_ms, 0, e.fi, e.fft_sec, e.time};
    }
    if (ncma) memcpy(ncma, c.ncma, sizeof c.ncma);
    if (pwr) {
        int rc = kg_ctx_use(fx->ctx);
        if (rc) return rc;
        const size_t n = (size_t) MAX_BINS * WIDTH;
        if (c.zero) {                                   // a restart whose zeroing waits for the channel's next block
            memset(pwr, 0, sizeof(float) * n);
        } else {
            KG_HIP(hipMemcpyAsync(pwr, fx->d_pwr.p + (size_t) ch * n, sizeof(float) * n, hipMemcpyDeviceToHost, fx->ctx->stream));
            KG_HIP(hipStreamSynchronize(fx->ctx->stream));
        }
    }
    return KG_OK;
}

}  // extern "C"
