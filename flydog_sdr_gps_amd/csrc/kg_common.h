// kg_common.h -- host-side plumbing shared by the libkiwigpu translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/kiwigpu.h"

void kg_set_error(const char *fmt, ...);

#define KG_HIP(call)                                                               \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) {                                                    \
            kg_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call,            \
                         hipGetErrorString(e_));                                   \
            return KG_ERR_HIP;                                                     \
        }                                                                          \
    } while (0)

// A call of the library's own that answers a status: any failure is this function's answer too.
#define KG_TRY(call)                                                               \
    do {                                                                           \
        const int rc_ = (call);                                                    \
        if (rc_ != KG_OK) return rc_;                                              \
    } while (0)

#define KG_REQUIRE(cond, status, ...)                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            kg_set_error(__VA_ARGS__);                                             \
            return (status);                                                       \
        }                                                                          \
    } while (0)

// Device and pinned memory have ONE door (kg_ctx.hip): nothing else in csrc/ calls hipMalloc, hipHostMalloc, hipFree or
// hipHostFree.  The door turns hipErrorOutOfMemory into KG_ERR_NOMEM (bytes and `what` in kg_last_error), counts the live
// allocations (kg_dev_live_allocs) and, under KIWIGPU_TUNING=1, refuses its k-th call for KIWIGPU_FAIL_ALLOC=k.  The four
// rules of ownership: one door; one owner per buffer (kg_dbuf / kg_hbuf members, freed by `delete`); a
// grow-on-demand group is released whole, allocated whole and its capacity published last; a host convenience's temporaries
// belong to a kg_scope.
__attribute__((visibility("hidden"))) int kg_mem_alloc(void **p, size_t bytes, bool pinned, const char *what);
__attribute__((visibility("hidden"))) int kg_mem_free(void *p, bool pinned);        // null passes; KG_ERR_HIP for what the runtime will not free

template <typename T, bool PINNED> struct kg_buf {
    T *p = nullptr;
    kg_buf() = default;
    kg_buf(const kg_buf &) = delete;
    kg_buf &operator=(const kg_buf &) = delete;
    ~kg_buf() { reset(); }
    int alloc(size_t n, const char *what) { reset(); return kg_mem_alloc((void **) &p, sizeof(T) * n, PINNED, what); }
    void reset() { (void) kg_mem_free((void *) p, PINNED); p = nullptr; }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};
template <typename T> using kg_dbuf = kg_buf<T, false>;      // device memory
template <typename T> using kg_hbuf = kg_buf<T, true>;       // pinned host memory

// A caller's device pointer (NULL passes: optional buffers) sits at a multiple of `a` bytes, a power of two: the width of the
// widest load or store a kernel makes through it (include/kiwigpu.h states the rule per entry point).
#define KG_ALIGNED(p, a) ((((uintptr_t) (p)) & ((uintptr_t) (a) - 1)) == 0)

// One step's small tables of EVERY stage of a receiver bank in one pinned host block, uploaded with ONE transfer
// (kg_rxbank.hip).  While a context's `arena` is set and active, kg_ctx_stage / kg_ctx_stage_cached[_ways] neither copy
// nor cache: in the PLAN pass they append the table to the host block and answer the address it will have on the
// device (the entry point then returns before its first launch and before it advances its state: KG_PLAN_ONLY.  What it does
// in front of that line it does in the PLAN pass too: an entry point that grows a buffer or makes a stream wait for an
// earlier call's event there -- the waterfall DDC's push does both -- says at that place why a PLAN pass may); in the
// REPLAY pass -- the same calls with the same arguments, after the block's one upload was enqueued -- they answer the same
// addresses again, checking that the table is the one planned.
enum { KG_ARENA_OFF = 0, KG_ARENA_PLAN = 1, KG_ARENA_REPLAY = 2 };
#define KG_ARENA_MAX_ENTRIES 244     /* <= 16 tables per step + 5 per sound block of the step (kg_rxbank_create checks its step against it) */
struct kg_arena {
    int mode;
    unsigned char *h_base, *d_base;           // the current slot of the owner's ring (pinned host / device)
    size_t cap, used;
    int nent, cursor;
    size_t off[KG_ARENA_MAX_ENTRIES], len[KG_ARENA_MAX_ENTRIES];
};

struct kg_ctx {
    int device;
    hipStream_t stream;
    bool own_stream;
    int num_cus;
    char name[256];
    hipEvent_t ev_start, ev_stop;
    // twiddle tables shared by every transform, built in double on the host
    float2 *d_tab4096;    // exp(+2 pi i k / 4096),  k < 4096
    float2 *d_tab16384;   // exp(+2 pi i k / 16384), k < 16384
    float2 *d_tab8192;    // exp(+2 pi i k / 8192),  k < 8192
    // small per-call tables (descriptor lists) of entry points that own no object
    void *d_scratch;
    size_t scratch_bytes;
    // Staging ring for the small per-call tables of the enqueue-only entry points (channel lists,
    // per-channel counts): KG_RING_SLOTS pinned host slots and as many device slots.  A call copies
    // its table into the next host slot and enqueues the transfer to the matching device slot; the
    // kernels it then enqueues read the device slot.  A slot comes round again KG_RING_SLOTS uploads
    // later and waits (normally not at all) for the event recorded half a ring after its last use.
    unsigned char *h_ring, *d_ring;
    hipEvent_t ring_ev[32];
    unsigned long ring_next;
    kg_arena *arena;                          // a receiver bank's step tables (null: the ring / the caches above)
    // A receiver bank's buffers hold one row per RECEIVER while its calls list only the receivers that are active (or, for
    // the coders, that completed a sound block this step): on the bank's contexts the row of list entry li, in every
    // caller-visible buffer of the enqueue-only entry points, is chans[li] instead of li.
    int rows_by_chan;
};

// An enqueue-only entry point that stages its tables through kg_ctx_stage* puts this right behind the (last) staging
// call: in a bank's PLAN pass the call ends here -- nothing launched, no state advanced.
#define KG_PLAN_ONLY(ctx_) do { if ((ctx_)->arena && (ctx_)->arena->mode == KG_ARENA_PLAN) return KG_OK; } while (0)

#define KG_RING_SLOTS 32
#define KG_RING_SLOT_BYTES ((size_t) 512 * 1024)

// A device copy of src[0..bytes) for kernels enqueued on ctx->stream after this call (and before
// KG_RING_SLOTS / 2 further kg_ctx_stage calls).  Does not synchronise the stream in steady state.
// Tables larger than a slot take the synchronous scratch buffer.
int kg_ctx_stage(kg_ctx *ctx, const void *src, size_t bytes, void **d_out);

// The same for a table that is usually the SAME from call to call (a channel list, the frame ->
// channel map of a batch): the owner keeps a kg_stage_cache; an unchanged table (memcmp with the
// host copy) costs no transfer at all, a changed one goes through the ring and, in stream order, into
// the cache's own device buffer (kernels still reading the old contents were enqueued before it).
struct kg_stage_cache;
void kg_stage_cache_free(kg_stage_cache *sc);       // the caller has drained the stream
struct kg_stage_cache {
    unsigned char *host = nullptr; void *dev = nullptr; size_t cap = 0, bytes = 0;
    kg_stage_cache() = default;
    kg_stage_cache(const kg_stage_cache &) = delete;
    kg_stage_cache &operator=(const kg_stage_cache &) = delete;
    ~kg_stage_cache() { kg_stage_cache_free(this); }     // with its owner (whose destroy has drained the stream)
};
int kg_ctx_stage_cached(kg_ctx *ctx, kg_stage_cache *sc, const void *src, size_t bytes, void **d_out);
// The same with `ways` caches looked up in turn and replaced round robin: a caller whose table cycles through a few
// variants (the frame tables of a streaming waterfall: the slow channel's frame completes every fourth push, so four
// tables alternate) uploads each of them once.  With one way every push of bench.py's cfg2_chain re-uploaded 64 KiB:
// a pinned-ring copy + two enqueued transfers, ~34 us of copy engines in line with the kernels of a 0.58 ms step.
int kg_ctx_stage_cached_ways(kg_ctx *ctx, kg_stage_cache *sc, int ways, int *victim, const void *src, size_t bytes, void **d_out);

// Device scratch of at least `bytes`, filled from `src` before returning (synchronous: the
// previous user of the scratch is drained first).  Valid until the next call on this context.
int kg_ctx_scratch_upload(kg_ctx *ctx, const void *src, size_t bytes, void **d_out);

// The device temporaries of a host convenience (kg_pos_solve, kg_trk_process_bits ...): lent by alloc(), and freed by the
// destructor AFTER it has drained the stream -- the caller's host arrays and the temporaries are in use until then, on the
// failing paths too.
struct kg_scope {
    hipStream_t stream;
    void *lent[4] = {nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    explicit kg_scope(const kg_ctx *c) : stream(c->stream) {}
    kg_scope(const kg_scope &) = delete;
    kg_scope &operator=(const kg_scope &) = delete;
    ~kg_scope()
    {
        (void) hipStreamSynchronize(stream);
        while (n > 0) (void) kg_mem_free(lent[--n], false);
    }
    template <typename T> int alloc(T **p, size_t count, const char *what)
    {
        *p = nullptr;
        KG_REQUIRE(n < 4, KG_ERR_STATE, "kg_scope: more than 4 temporaries (%s)", what);
        KG_TRY(kg_mem_alloc(&lent[n], sizeof(T) * count, false, what));
        *p = (T *) lent[n++];
        return KG_OK;
    }
};

// The library's tuning switches (KIWIGPU_FAIL_ALLOC, KIWIGPU_DDC_RUNS, KIWIGPU_DDC_SIDE, KIWIGPU_DDC_STAGED, KIWIGPU_RXDDC_RUNS,
// KIWIGPU_WF_WGS_PER_CU, KIWIGPU_ACQ_WGS_PER_CU, KIWIGPU_ACQ_FRONT_STREAM) are A/B aids: they are read
// ONLY when KIWIGPU_TUNING=1 is set too -- a stray variable in a host's environment does not change what the library does.
static inline const char *kg_tuning_env(const char *name)
{
    const char *on = getenv("KIWIGPU_TUNING");
    return (on && on[0] == '1' && on[1] == 0) ? getenv(name) : nullptr;
}

// Make ctx's device current on the calling thread.
static inline int kg_ctx_use(kg_ctx *ctx)
{
    KG_REQUIRE(ctx != nullptr, KG_ERR_INVALID, "null context");
    KG_HIP(hipSetDevice(ctx->device));
    return KG_OK;
}

// The whole destroy of an object that owns nothing beyond its members (null passes): its context's stream is drained first,
// because kernels enqueued there may still use the device memory that `delete` releases.
template <typename T> static inline void kg_drain_delete(T *obj)
{
    if (!obj) return;
    (void) hipSetDevice(obj->ctx->device);
    (void) hipStreamSynchronize(obj->ctx->stream);
    delete obj;
}

// The DDCs' NCO reads: ph holds the 48-bit accumulator in its top bits, the table index is its top 13 (KG_NCO_* below).
// (What the table reads cost -- against no reads at all, and against the hardware's v_sin_f32 / v_cos_f32 -- was measured
// once with two builds that computed wrong values: profiles/r06_nco_knockout.txt)
#define KG_NCO_COS(tab_, ph_) ((int) (tab_)[((ph_) >> 51) + 2048])
#define KG_NCO_SIN(tab_, ph_) ((int) (tab_)[(ph_) >> 51])

// The DDCs' NCO table (frozen by us: the Xilinx DDS core of verilog/rx/iq_mixer.v is closed IP), as ONE 16-bit sine
// table of KG_NCO_TAB = 10240 entries: T[j] = round(16383 sin(2 pi j / 8192)) for j < 8192 and, BY CONSTRUCTION,
// T[j] = T[j - 8192] beyond.  sin(a) = T[a], cos(a) = T[a + 2048] for a < 8192: two sign-extending 16-bit LDS reads
// from one address.  That this equals round(16383 cos(2 pi a / 8192)) -- the oracle's definition -- is checked once in
// the CPU suite through kg_ddc_nco_table (tests/test_host_cpu.py), not at run time.
#define KG_NCO_TAB 10240
extern "C" __attribute__((visibility("hidden"))) void kg_nco_table_build(short *tab);        // kg_ctx.hip (not part of the ABI: kg_ddc_nco_table is)

// kg_ddc.hip, for kg_rxbank.hip (not part of the ABI): the DDC's second stream supplied by the owner.
struct kg_ddc;
__attribute__((visibility("hidden"))) int kg_ddc_use_side_stream(kg_ddc *ddc, hipStream_t stream);

// kg_snd.hip, for kg_rxbank.hip (not part of the ABI): kg_fir_process_spec_dev with the rows placed by the caller.  Per list entry
// i: inst[i]; the leading row_n[i] completed blocks give a row (null: all of them); block b's row goes to d_rows + row_base[i] *
// row_unit + 1024 b (null: entry i, or the channel on a bank's context); rows_bytes: the extent of d_rows.
struct kg_fir_spec_req {
    void *d_rows; size_t row_unit, rows_bytes;
    const int32_t *inst, *row_n, *row_base;
};
__attribute__((visibility("hidden"))) int kg_fir_process_rows_(kg_fir *f, const int32_t *chans, int nch, const void *d_in, size_t in_stride,
                                                               const int32_t *n_each, void *d_out, size_t out_stride, int32_t *nout,
                                                               const kg_fir_spec_req *req);

// the same with the filtered spectrum of every completed block stored too (kg_fir_process_taps_dev's d_post), rows or not (req may be null)
__attribute__((visibility("hidden"))) int kg_fir_process_post_(kg_fir *f, const int32_t *chans, int nch, const void *d_in, size_t in_stride,
                                                               const int32_t *n_each, void *d_out, size_t out_stride, int32_t *nout,
                                                               const kg_fir_spec_req *req, void *d_post, size_t tap_stride);

// kg_fftext.hip, for kg_rxbank.hip (not part of the ABI): kg_fftext_process_dev with entry i's spectra at row spec_row[i] of d_spec
struct kg_fftext;
__attribute__((visibility("hidden"))) int kg_fftext_process_rows_(kg_fftext *fx, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst,
                                                                  const int32_t *spec_row, const float *d_spec, size_t spec_stride, uint8_t *d_rows,
                                                                  size_t row_stride, int max_rows, int32_t *rx_of_row, int32_t *ent_of_row,
                                                                  int32_t *blk_of_row, int32_t *bin_of_row);

// kg_iqd.hip, for kg_rxbank.hip (not part of the ABI): kg_iqd_process_dev with entry i's samples at row iq_row[i] of d_iq
__attribute__((visibility("hidden"))) int kg_iqd_process_rows_(kg_iqd *q, const int32_t *chans, int nch, const int32_t *nblk, const int32_t *inst,
                                                               const int32_t *iq_row, int ns, const float *d_iq, size_t iq_stride, uint8_t *d_rows,
                                                               size_t rows_cap, kg_iqd_status *d_status, size_t status_cap, kg_iqd_row *row_map,
                                                               int max_rows, int32_t *status_sent);

// kg_lorc.hip, for kg_rxbank.hip (not part of the ABI): kg_lorc_process on device memory, entry i's samples at row in_row[i] of d_iq
// (null: row i), the rows packed into d_rows (16-byte aligned, each row at a multiple of 16); the bytes a call's table takes when no
// channel has more than runs_per_channel runs; kg_lorc_set_gri refusing a GRI of fewer than min_spg samples too
__attribute__((visibility("hidden"))) int kg_lorc_process_rows_(kg_lorc *q, const int32_t *conns, int nconn, const int32_t *nblk, const int32_t *in_row, int ns,
                                                                const float *d_iq, size_t iq_stride, uint8_t *d_rows, size_t rows_cap, kg_lorc_row *row_map,
                                                                int max_rows, int32_t *nrows);
__attribute__((visibility("hidden"))) size_t kg_lorc_table_bytes_(size_t nconn, size_t runs_per_channel);
__attribute__((visibility("hidden"))) int kg_lorc_set_gri_min_(kg_lorc *q, int conn, int ch, int gri, double min_spg);
// connection conn as a new connection finds it: all zero, stopped, not initialised
__attribute__((visibility("hidden"))) int kg_lorc_reset_(kg_lorc *q, int conn);

// kg_fax.hip, for kg_rxbank.hip (not part of the ABI): kg_fax_push on device memory, samples and outputs alike, entry i's samples at
// in_off[i] samples from d_s16 (null: i * stride), enqueue only; the bytes a push's table takes; connection conn as a new connection finds it: the zeroed object, not started
__attribute__((visibility("hidden"))) int kg_fax_push_at_(kg_fax *q, const int32_t *conns, int nconn, const int32_t *nblk, const int64_t *in_off, const int16_t *d_s16,
                                                          size_t stride, const double *srate, uint8_t *d_rows, size_t row_stride, kg_fax_rec *d_recs, int max_lines,
                                                          int32_t *d_counts);
__attribute__((visibility("hidden"))) size_t kg_fax_table_bytes_(size_t nconn);
__attribute__((visibility("hidden"))) int kg_fax_reset_(kg_fax *q, int conn);

// kg_cw.hip, for kg_rxbank.hip (not part of the ABI): kg_cw_push on device memory, samples and outputs alike, entry i's samples at
// in_off[i] samples from d_s16 (null: i * stride), enqueue only; the bytes a push's table takes; connection conn as a new connection finds it: the zeroed object, not started
__attribute__((visibility("hidden"))) int kg_cw_push_at_(kg_cw *q, const int32_t *conns, int nconn, const int32_t *nblk, const int64_t *in_off, const int16_t *d_s16,
                                                         size_t stride, const uint32_t *now_sec, kg_cw_ev *d_evs, int max_events, int32_t *d_counts);
__attribute__((visibility("hidden"))) size_t kg_cw_table_bytes_(size_t nconn);
__attribute__((visibility("hidden"))) int kg_cw_reset_(kg_cw *q, int conn);
// kg_ft8.hip, for kg_rxbank.hip (not part of the ABI): kg_ft8_push on device memory with the entries placed by offsets; what its table takes; a reset.
__attribute__((visibility("hidden"))) int kg_ft8_push_at_(kg_ft8 *q, const int32_t *conns, int nconn, const int32_t *ncb, const int64_t *in_off, int ns, const int16_t *d_in,
                                                          size_t sample_stride, const double *times, size_t time_stride, kg_ft8_ev *evs, int max_events, int32_t *nevents,
                                                          kg_ft8_slot *d_slots, int max_slots, int32_t *slot_conn, int32_t *nslots);
__attribute__((visibility("hidden"))) size_t kg_ft8_table_bytes_(size_t nconn, size_t ncb);
__attribute__((visibility("hidden"))) int kg_ft8_reset_(kg_ft8 *q, int conn);
__attribute__((visibility("hidden"))) int kg_ft8_inited_(const kg_ft8 *q, int conn);

// kg_wspr.hip, for kg_rxbank.hip (not part of the ABI): kg_wspr_push on device memory, samples and outputs alike, entry i's samples at row
// in_row[i] of d_iq (null: row i), rows at multiples of KG_WSPR_ROW_STRIDE in list order, cycles and counts an entry of the list each,
// enqueue only; the bytes a push's table takes when no connection has more than ops_per_conn ops; connection conn as a new connection
// finds it: the zeroed object, not initialised
struct kg_wspr;
__attribute__((visibility("hidden"))) int kg_wspr_push_rows_(kg_wspr *q, const int32_t *conns, int nconn, const int32_t *nblk, const int32_t *in_row, int ns,
                                                             const float *d_iq, size_t iq_stride, const int32_t *minute, const int32_t *second, size_t time_stride,
                                                             uint8_t *d_rows, size_t rows_cap, kg_wspr_row *row_map, int max_rows, int32_t *nrows, kg_wspr_ev *evs,
                                                             int max_events, int32_t *nevents, kg_wspr_cycle *d_cycles, int32_t *d_counts);
__attribute__((visibility("hidden"))) size_t kg_wspr_table_bytes_(size_t nconn, size_t ops_per_conn);
__attribute__((visibility("hidden"))) int kg_wspr_reset_(kg_wspr *q, int conn);
// stage 2: the device records and counts of the pushes' pass 0, [connection][12] and [connection]; whether a connection's decode is on
__attribute__((visibility("hidden"))) void kg_wspr_dec_buffers_(kg_wspr *q, kg_wspr_dec **d_decs, int32_t **d_ncand);
__attribute__((visibility("hidden"))) int kg_wspr_decode_on_(const kg_wspr *q, int conn);

// kg_post.hip, for kg_rxbank.hip: how many kg_post_set_mode / kg_post_set_sam_mparam calls channel ch has seen (each clears
// s->isChanNull, rx_sound_cmd.cpp:202-228), and its s->SAM_mparam
__attribute__((visibility("hidden"))) uint32_t kg_post_mode_cmds_(const kg_post *p, int ch);
__attribute__((visibility("hidden"))) int kg_post_sam_mparam_(const kg_post *p, int ch);

// The library's own streams come from a per-device pool and go back to it; they are never destroyed.  Which hardware queue a
// NEW stream lands on is the runtime's choice at that moment, and streams created after others had been destroyed were seen
// to get queues on which kernels take turns with other streams' instead of running beside them: an object
// that inherits a stream inherits its placement.  Synchronise a stream before giving it back.
int kg_stream_get(int device, hipStream_t *out);          // the device is current (kg_ctx_use) when this is called
void kg_stream_put(int device, hipStream_t s);

// kg_nb.hip, for kg_wf.hip (not part of the ABI): a set of CNoiseProc states on the device (kg_nb.h), one per channel, and the
// waterfall's blanker pre-pass over them.
struct kg_nb_store;
__attribute__((visibility("hidden"))) int kg_nb_store_create(int nchan, kg_nb_store **out);
__attribute__((visibility("hidden"))) void kg_nb_store_destroy(kg_nb_store *s);                // the caller has drained the stream
__attribute__((visibility("hidden"))) int kg_nb_store_was_setup(const kg_nb_store *s, int ch);
// SetupBlanker(ch, sample_rate, nb_param) in stream order (refusals as kg_nb_setup's, messages under `who`)
__attribute__((visibility("hidden"))) int kg_nb_store_setup(kg_ctx *ctx, kg_nb_store *s, int ch, float sample_rate, const float *nb_param,
                                                            const char *who);
__attribute__((visibility("hidden"))) int kg_nb_store_state(kg_ctx *ctx, kg_nb_store *s, const int32_t *chans, int nch, int32_t *ints,
                                                            float *flts, const char *who);
// ProcessBlankerOneShot on windowed frames: d_chl [nbch] {channel, first frame, frame count, window function}, d_fl [frames]
// {first iq_t of the frame in d_iq, row of d_out}; d_out rows of 8192 complex floats.  Enqueue only, no checks.
__attribute__((visibility("hidden"))) int kg_nb_wf_launch(kg_ctx *ctx, kg_nb_store *s, int nbch, const void *d_chl, const void *d_fl,
                                                          const void *d_iq, const float *d_windows, void *d_out);
// kg_nb.hip, for kg_rxbank.hip: whether channel ch of an audio blanker object was set up
struct kg_nb;
__attribute__((visibility("hidden"))) int kg_nb_was_setup(const kg_nb *nb, int ch);
