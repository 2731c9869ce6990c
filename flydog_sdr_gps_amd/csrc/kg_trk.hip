// kg_trk.hip -- GPS tracking channels: DEMOD (verilog/gps/demod.v) and GPS_Method (e_cpu/kiwi.gps.asm) of up to 12 channels.
//
// One wave per channel.  The channel's control -- where the rates change, where ms1 falls, the loop service, the nav machine -- is
// sequential and runs in every lane with the same values (kg_trk.h, run()); between two such points the E/P/L replica bits, the LO
// bits and the sample bits of 64 clocks are one 64-bit word each per lane, XORed and counted, and the wave adds the counts up.
#include "kg_common.h"
#include "kg_trk.h"

#include <new>
#include <vector>

using namespace kg_trk_cf;

static_assert(sizeof(epoch) == sizeof(kg_trk_epoch) && sizeof(epoch) == 48, "kg_trk_epoch layout");
static_assert(offsetof(gps_chan, cg_freq) == 24 && offsetof(gps_chan, iq) == 40 && offsetof(gps_chan, cg_gain) == 64 &&
              offsetof(gps_chan, lo_polarity) == 76, "GPS_CHAN layout");
static_assert(CHAN_BYTES == KG_TRK_CHAN_BYTES && E1B_MODE == KG_TRK_E1B_MODE && G2_INIT == KG_TRK_G2_INIT, "constants");

struct wave_sum {
    __device__ seg_sums operator()(seg_sums v) const
    {
        for (int off = 32; off >= 1; off >>= 1) {
            for (int i = 0; i < 6; i++) v.cnt[i] += __shfl_xor(v.cnt[i], off);
            v.last |= __shfl_xor(v.last, off);
        }
        return v;
    }
};

__global__ __launch_bounds__(64) void trk_kernel(chan *__restrict__ st, const chan_tab *__restrict__ tabs, const uint8_t *__restrict__ bits,
                                                 uint64_t nbytes, uint32_t bit0, uint64_t nclocks, uint64_t clock0, uint32_t cg_cnt,
                                                 epoch *__restrict__ out, size_t chan_stride, int cap, int32_t *__restrict__ counts)
{
    __shared__ uint32_t tab[TABLE_WORDS];
    const uint32_t lane = threadIdx.x, ch = blockIdx.x;
    for (uint32_t i = lane; i < TABLE_WORDS; i += 64) tab[i] = tabs[ch].w[i];
    __syncthreads();
    chan c = st[ch];
    int n = 0;
    run(c, tab, bits, nbytes, (uint64_t) bit0, nclocks, clock0, cg_cnt, out + (size_t) ch * chan_stride, cap, &n, lane, 64u, wave_sum());
    if (lane == 0) {
        st[ch] = c;
        counts[ch] = n;
    }
}

struct kg_trk {
    kg_ctx *ctx;
    int nchan;
    std::vector<chan> h;            // the host's copy of the channels: current unless host_stale
    std::vector<chan_tab> tab;
    std::vector<chan_tab> e1b;      // the code memory's column of each channel
    kg_dbuf<chan> d_chan;
    kg_dbuf<chan_tab> d_tab;
    bool host_stale, dev_stale, tab_stale;
    uint32_t cg_cnt, mask;
    uint64_t clock;
};

static int trk_fetch(kg_trk *t)     // make the host's copy current
{
    int rc = kg_ctx_use(t->ctx);
    if (rc) return rc;
    if (!t->host_stale) return KG_OK;
    KG_HIP(hipMemcpyAsync(t->h.data(), t->d_chan, sizeof(chan) * t->nchan, hipMemcpyDeviceToHost, t->ctx->stream));
    KG_HIP(hipStreamSynchronize(t->ctx->stream));
    t->host_stale = false;
    return KG_OK;
}

#define TRK_CMD(t_, ch_, who_)                                                                              \
    KG_REQUIRE((t_) != nullptr, KG_ERR_INVALID, who_ ": null handle");                                      \
    KG_REQUIRE((ch_) >= 0 && (ch_) < (t_)->nchan, KG_ERR_INVALID, who_ ": channel %d of %d", (ch_), (t_)->nchan); \
    { int rc_ = trk_fetch(t_); if (rc_) return rc_; }

static int trk_init(kg_trk *t, int nchan, int lo_delay, int cg_delay)
{
    t->h.assign(nchan, chan());
    t->tab.assign(nchan, chan_tab());
    t->e1b.assign(nchan, chan_tab());
    for (chan &c : t->h) {
        memset(&c, 0, sizeof c);
        c.cg_en = 1; c.loop_on = 1;
        c.ms1_due = c.lo_due = c.cg_due = -1;
        c.lo_delay = lo_delay; c.cg_delay = cg_delay;
    }
    for (int i = 0; i < nchan; i++) { memset(&t->tab[i], 0, sizeof(chan_tab)); memset(&t->e1b[i], 0, sizeof(chan_tab)); }
    t->host_stale = false; t->dev_stale = true; t->tab_stale = true;
    t->cg_cnt = 0; t->mask = 0; t->clock = 0;
    KG_TRY(t->d_chan.alloc(nchan, "kg_trk_create: channels"));
    return t->d_tab.alloc(nchan, "kg_trk_create: code tables");
}

extern "C" {

int kg_trk_create(kg_ctx *ctx, int nchan, int lo_delay, int cg_delay, kg_trk **out)
{
    int rc = kg_ctx_use(ctx);
    if (rc) return rc;
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "kg_trk_create: out is null");
    *out = nullptr;
    KG_REQUIRE(nchan >= 1 && nchan <= KG_TRK_MAX_CHANS, KG_ERR_INVALID, "kg_trk_create: nchan %d (1..%d)", nchan, KG_TRK_MAX_CHANS);
    if (lo_delay == 0) lo_delay = KG_TRK_LO_DELAY;
    if (cg_delay == 0) cg_delay = KG_TRK_CG_DELAY;
    KG_REQUIRE(lo_delay >= 2 && lo_delay <= KG_TRK_MIN_EPOCH - 1 && cg_delay >= 2 && cg_delay <= KG_TRK_MIN_EPOCH - 1, KG_ERR_INVALID,
               "kg_trk_create: delays %d, %d outside 2..%d", lo_delay, cg_delay, KG_TRK_MIN_EPOCH - 1);
    KG_REQUIRE(lo_delay <= cg_delay, KG_ERR_INVALID, "kg_trk_create: lo_delay %d after cg_delay %d (GPS_Method closes the LO loop first)",
               lo_delay, cg_delay);
    kg_trk *t = new (std::nothrow) kg_trk();
    KG_REQUIRE(t != nullptr, KG_ERR_NOMEM, "kg_trk_create: alloc");
    t->ctx = ctx; t->nchan = nchan;
    rc = trk_init(t, nchan, lo_delay, cg_delay);
    if (rc) { kg_trk_destroy(t); return rc; }
    *out = t;
    return KG_OK;
}

void kg_trk_destroy(kg_trk *t) { kg_drain_delete(t); }

int kg_trk_set_sat(kg_trk *t, int ch, int codegen_init)
{
    TRK_CMD(t, ch, "kg_trk_set_sat");
    KG_REQUIRE(codegen_init >= 0 && codegen_init < 0x1000, KG_ERR_INVALID, "kg_trk_set_sat: word 0x%x is not 12 bits", codegen_init);
    if (!(codegen_init & (E1B_MODE | G2_INIT))) {
        const int t0 = (codegen_init >> 4) & 15, t1 = codegen_init & 15;
        KG_REQUIRE(!(codegen_init & 0x300) && t0 >= 1 && t0 <= 10 && t1 >= 1 && t1 <= 10, KG_ERR_INVALID,
                   "kg_trk_set_sat: taps %d, %d outside g2[10:1]", t0, t1);
    }
    chan &c = t->h[ch];
    c.sat = codegen_init;
    c.fw.e1b_mode = (uint16_t) (codegen_init & E1B_MODE);               // CmdSetSat stores sat & E1B_MODE
    c.have_sat = 1; c.seeded = 0;
    t->dev_stale = true;
    return KG_OK;
}

int kg_trk_set_e1b_code(kg_trk *t, int ch, const uint8_t *chips, int nchips)
{
    TRK_CMD(t, ch, "kg_trk_set_e1b_code");
    KG_REQUIRE(chips != nullptr && nchips == E1B_CODELEN, KG_ERR_INVALID, "kg_trk_set_e1b_code: %d chips (need %d)", nchips, E1B_CODELEN);
    for (int i = 0; i < nchips; i++) KG_REQUIRE(chips[i] <= 1, KG_ERR_INVALID, "kg_trk_set_e1b_code: chip %d is %d", i, chips[i]);
    chan_tab &m = t->e1b[ch];
    memset(&m, 0, sizeof m);
    for (int i = 0; i < nchips; i++) m.w[i >> 5] |= (uint32_t) chips[i] << (i & 31);
    t->h[ch].have_code = 1;
    if (t->h[ch].sat & E1B_MODE) { t->tab[ch] = m; t->tab_stale = true; }
    t->dev_stale = true;
    return KG_OK;
}

int kg_trk_set_rate_lo(kg_trk *t, int ch, uint32_t rate)
{
    TRK_CMD(t, ch, "kg_trk_set_rate_lo");
    t->h[ch].fw.lo_freq = (uint64_t) rate << 32;
    t->h[ch].lo_rate = rate;
    t->dev_stale = true;
    return KG_OK;
}

int kg_trk_set_rate_cg(kg_trk *t, int ch, uint32_t rate)
{
    TRK_CMD(t, ch, "kg_trk_set_rate_cg");
    KG_REQUIRE(rate >= (1u << 27) && rate < (1u << 29), KG_ERR_INVALID, "kg_trk_set_rate_cg: rate 0x%x outside [2^27, 2^29)", rate);
    KG_REQUIRE(!rate_would_hold_ms0(t->h[ch], rate), KG_ERR_STATE,
               "kg_trk_set_rate_cg: with this rate the paused channel %d would hold ms0 set: set it after the pause has ended", ch);
    t->h[ch].fw.cg_freq = (uint64_t) rate << 32;
    t->h[ch].cg_rate = rate;
    t->h[ch].fault = 0;
    t->dev_stale = true;
    return KG_OK;
}

static int trk_gain(kg_trk *t, int ch, int ki, int kpm, bool lo, const char *who)
{
    KG_REQUIRE(ki >= 0 && ki <= 63 && kpm >= 0 && kpm <= 63, KG_ERR_INVALID, "%s: ki %d, kp - ki %d outside 0..63", who, ki, kpm);
    uint16_t *g = lo ? t->h[ch].fw.lo_gain : t->h[ch].fw.cg_gain;
    g[0] = (uint16_t) ki; g[1] = (uint16_t) kpm;
    t->dev_stale = true;
    return KG_OK;
}

int kg_trk_set_gain_lo(kg_trk *t, int ch, int ki, int kp_minus_ki)
{
    TRK_CMD(t, ch, "kg_trk_set_gain_lo");
    return trk_gain(t, ch, ki, kp_minus_ki, true, "kg_trk_set_gain_lo");
}

int kg_trk_set_gain_cg(kg_trk *t, int ch, int ki, int kp_minus_ki)
{
    TRK_CMD(t, ch, "kg_trk_set_gain_cg");
    return trk_gain(t, ch, ki, kp_minus_ki, false, "kg_trk_set_gain_cg");
}

int kg_trk_set_polarity(kg_trk *t, int ch, int polarity)
{
    TRK_CMD(t, ch, "kg_trk_set_polarity");
    KG_REQUIRE(polarity >= 0 && polarity <= 2, KG_ERR_INVALID, "kg_trk_set_polarity: %d", polarity);
    t->h[ch].fw.lo_polarity = (uint16_t) polarity;
    t->dev_stale = true;
    return KG_OK;
}

int kg_trk_set_mask(kg_trk *t, uint32_t mask)
{
    KG_REQUIRE(t != nullptr, KG_ERR_INVALID, "kg_trk_set_mask: null handle");
    t->mask = mask;
    return KG_OK;
}

int kg_trk_sampler_reset(kg_trk *t)
{
    TRK_CMD(t, 0, "kg_trk_sampler_reset");
    for (int ch = 0; ch < t->nchan; ch++)
        KG_REQUIRE(((t->mask >> ch) & 1) || !reset_would_hold_ms0(t->h[ch]), KG_ERR_STATE,
                   "kg_trk_sampler_reset: the paused channel %d has a service due and would hold ms0 set at chip 0: process until its "
                   "pause has ended, or mask it", ch);
    for (int ch = 0; ch < t->nchan; ch++) {
        if ((t->mask >> ch) & 1) continue;
        chan &c = t->h[ch];
        c.cg_phase = 0; c.nchip = 0;
        if (c.have_sat) {
            if (c.sat & E1B_MODE) t->tab[ch] = t->e1b[ch];
            else ca_table(c.sat, &t->tab[ch]);
            c.seeded = 1;
            t->tab_stale = true;
        }
    }
    t->dev_stale = true;
    return KG_OK;
}

int kg_trk_pause(kg_trk *t, int ch, int count)
{
    TRK_CMD(t, ch, "kg_trk_pause");
    KG_REQUIRE(count >= 0 && count <= 0xFFFF, KG_ERR_INVALID, "kg_trk_pause: count %d", count);
    KG_REQUIRE(!pause_would_hold_ms0(t->h[ch]), KG_ERR_STATE,
               "kg_trk_pause: channel %d would stand where ms0 stays set (nchip 0 at a held half chip, or a service due in its first chip): "
               "process 16 clocks more first", ch);
    t->h[ch].cg_en = 0;
    t->cg_cnt = (uint32_t) count;
    t->dev_stale = true;
    return KG_OK;
}

int kg_trk_set_loop(kg_trk *t, int ch, int on)
{
    TRK_CMD(t, ch, "kg_trk_set_loop");
    t->h[ch].loop_on = on != 0;
    t->dev_stale = true;
    return KG_OK;
}

int kg_trk_process_bits_dev(kg_trk *t, const uint8_t *d_bits, size_t nclocks, kg_trk_epoch *d_epochs, size_t chan_stride, int cap,
                            int32_t *d_counts)
{
    KG_REQUIRE(t && d_bits && d_epochs && d_counts, KG_ERR_INVALID, "kg_trk_process_bits_dev: null argument");
    int rc = kg_ctx_use(t->ctx);
    if (rc) return rc;
    KG_REQUIRE(nclocks >= 1 && nclocks <= ((size_t) 1 << 40), KG_ERR_INVALID, "kg_trk_process_bits_dev: nclocks %zu", nclocks);
    KG_REQUIRE(cap >= 2 && (size_t) cap >= nclocks / KG_TRK_MIN_EPOCH + 2, KG_ERR_INVALID, "kg_trk_process_bits_dev: cap %d below %zu", cap,
               nclocks / KG_TRK_MIN_EPOCH + 2);
    KG_REQUIRE(chan_stride >= (size_t) cap, KG_ERR_INVALID, "kg_trk_process_bits_dev: chan_stride %zu below cap %d", chan_stride, cap);
    KG_REQUIRE(KG_ALIGNED(d_epochs, 8) && KG_ALIGNED(d_counts, 4), KG_ERR_INVALID, "kg_trk_process_bits_dev: d_epochs needs 8-byte, d_counts 4-byte alignment");
    if (t->dev_stale) {                                                 // commands came in: the host's copy is the current one
        for (int ch = 0; ch < t->nchan; ch++) {
            const chan &c = t->h[ch];
            KG_REQUIRE(c.have_sat, KG_ERR_INVALID, "kg_trk_process_bits_dev: channel %d has no satellite (kg_trk_set_sat)", ch);
            KG_REQUIRE(c.seeded, KG_ERR_INVALID, "kg_trk_process_bits_dev: channel %d was not reset since kg_trk_set_sat", ch);
            KG_REQUIRE(!(c.sat & E1B_MODE) || c.have_code, KG_ERR_INVALID, "kg_trk_process_bits_dev: channel %d is in E1B mode without a code", ch);
            KG_REQUIRE(!c.fault, KG_ERR_STATE, "kg_trk_process_bits_dev: channel %d: the code loop left [2^27, 2^29); set its rate again", ch);
            KG_REQUIRE(c.cg_rate >= (1u << 27) && c.cg_rate < (1u << 29), KG_ERR_INVALID, "kg_trk_process_bits_dev: channel %d has no code rate", ch);
            KG_REQUIRE(!holds_ms0(c), KG_ERR_STATE, "kg_trk_process_bits_dev: channel %d is paused where ms0 would stay set", ch);   // the commands refuse what leads here
        }
        KG_HIP(hipMemcpyAsync(t->d_chan, t->h.data(), sizeof(chan) * t->nchan, hipMemcpyHostToDevice, t->ctx->stream));
        if (t->tab_stale) KG_HIP(hipMemcpyAsync(t->d_tab, t->tab.data(), sizeof(chan_tab) * t->nchan, hipMemcpyHostToDevice, t->ctx->stream));
        KG_HIP(hipStreamSynchronize(t->ctx->stream));                   // the copies read pageable host memory the next command may change
        t->dev_stale = false; t->tab_stale = false;
    }
    const uint32_t bit0 = (uint32_t) (t->clock & 7);
    const uint64_t nbytes = (bit0 + (uint64_t) nclocks + 7) / 8;
    hipLaunchKernelGGL(trk_kernel, dim3(t->nchan), dim3(64), 0, t->ctx->stream, t->d_chan, (const chan_tab *) t->d_tab, d_bits, nbytes, bit0,
                       (uint64_t) nclocks, t->clock, t->cg_cnt, (epoch *) d_epochs, chan_stride, cap, d_counts);
    KG_HIP(hipGetLastError());
    t->host_stale = true;
    t->clock += nclocks;
    t->cg_cnt = (uint32_t) ((t->cg_cnt - (uint64_t) nclocks) & 0xFFFF);
    return KG_OK;
}

int kg_trk_process_bits(kg_trk *t, const uint8_t *bits, size_t nclocks, kg_trk_epoch *epochs, size_t chan_stride, int cap, int32_t *counts)
{
    KG_REQUIRE(t && bits && epochs && counts, KG_ERR_INVALID, "kg_trk_process_bits: null argument");
    int rc = kg_ctx_use(t->ctx);
    if (rc) return rc;
    KG_REQUIRE(nclocks >= 1 && cap >= 2 && chan_stride >= (size_t) cap, KG_ERR_INVALID, "kg_trk_process_bits: nclocks %zu, cap %d, chan_stride %zu",
               nclocks, cap, chan_stride);
    const size_t nbytes = ((t->clock & 7) + nclocks + 7) / 8, ebytes = sizeof(kg_trk_epoch) * chan_stride * t->nchan;
    uint8_t *d_bits = nullptr;
    kg_trk_epoch *d_ep = nullptr;
    int32_t *d_cnt = nullptr;
    kg_scope tmp(t->ctx);
    KG_TRY(tmp.alloc(&d_bits, nbytes, "kg_trk_process_bits: bits"));
    KG_TRY(tmp.alloc(&d_ep, chan_stride * t->nchan, "kg_trk_process_bits: epochs"));
    KG_TRY(tmp.alloc(&d_cnt, t->nchan, "kg_trk_process_bits: counts"));
    KG_HIP(hipMemcpyAsync(d_bits, bits, nbytes, hipMemcpyHostToDevice, t->ctx->stream));
    KG_HIP(hipMemsetAsync(d_ep, 0, ebytes, t->ctx->stream));
    KG_TRY(kg_trk_process_bits_dev(t, d_bits, nclocks, d_ep, chan_stride, cap, d_cnt));
    KG_HIP(hipMemcpyAsync(counts, d_cnt, sizeof(int32_t) * t->nchan, hipMemcpyDeviceToHost, t->ctx->stream));
    KG_HIP(hipStreamSynchronize(t->ctx->stream));
    for (int ch = 0; ch < t->nchan; ch++)
        if (counts[ch] > 0 || counts[ch] < -1)
            KG_HIP(hipMemcpy(epochs + (size_t) ch * chan_stride, d_ep + (size_t) ch * chan_stride,
                             sizeof(kg_trk_epoch) * (counts[ch] < 0 ? -1 - counts[ch] : counts[ch]), hipMemcpyDeviceToHost));
    return KG_OK;
}

int kg_trk_get_chan(kg_trk *t, int ch, uint8_t *out)
{
    TRK_CMD(t, ch, "kg_trk_get_chan");
    KG_REQUIRE(out != nullptr, KG_ERR_INVALID, "kg_trk_get_chan: out is null");
    KG_REQUIRE(!t->h[ch].fault, KG_ERR_STATE, "kg_trk_get_chan: channel %d stopped: the code loop wrote a word outside [2^27, 2^29)", ch);
    memcpy(out, &t->h[ch].fw, CHAN_BYTES);
    return KG_OK;
}

int kg_trk_get_clocks(kg_trk *t, uint64_t *clock, uint32_t *replicas)
{
    TRK_CMD(t, 0, "kg_trk_get_clocks");
    KG_REQUIRE(clock && replicas, KG_ERR_INVALID, "kg_trk_get_clocks: null argument");
    *clock = t->clock;
    for (int ch = 0; ch < t->nchan; ch++) replicas[ch] = replica(t->h[ch]);
    return KG_OK;
}

}  // extern "C"
